"""What an update of a growing recording costs: tools/stream_times.py [--out FILE] [--precision f32|x3]
The planted hour (synth, seed 1234; scores and embeddings planted as bench.py plants them) goes through an sd_stream in 10 s pieces with
turns() after each piece.  At prefixes of 1 min, 10 min and 1 h it reports the push and turns() times -- medians of five updates around each
size, host clock around calls that end in a device synchronise, after a warm-up pass over the same hour -- and, alternating with them in the
same process, diarize_dev of the same prefixes: the only way to the same answer without a stream.  Turn equality is checked at the three sizes."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd"))
import sdhip, synth, weightpack as nn      # noqa: E402

PIECE = 160000                              # 10 s
MARKS = (("1 min", 6), ("10 min", 60), ("1 h", 360))      # pieces pushed at the size; the five updates measured end at pieces k-2 .. k+2 (1 h: k-4 .. k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", default="f32", choices=["f32", "x3"])
    a = ap.parse_args()
    import torch
    tmp = tempfile.mkdtemp()
    nn.save_pack(tmp + "/s.sdw", nn.synth_segmentation_weights(4321))
    nn.save_pack(tmp + "/e.sdw", nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(tmp + "/s.sdw", tmp + "/e.sdw", 0)
    if a.precision == "x3":
        d.set_option("ecapa_precision", 3)
    sec = 3600.0
    pcm = synth.make_pcm(sec, seed=1234)
    n_all = len(pcm)
    nc = synth.num_chunks(n_all)
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(sec, 1234)), n_all, 0, nc)
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_sc, d_pe = torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
    torch.cuda.synchronize()
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    measured = {}
    for label, k in MARKS:
        for j in (range(k - 4, k + 1) if k * PIECE >= n_all else range(k - 2, k + 3)):
            measured[j] = label
    rows = {label: {"push": [], "turns": [], "whole": [], "whole_stages": [], "turn_stages": []} for label, _ in MARKS}
    equal = {}

    def one_pass(timed):
        with d.stream() as s:
            for j in range(1, n_all // PIECE + 1):
                n = j * PIECE
                t0 = time.perf_counter()
                s.push(pcm[n - PIECE:n])
                t1 = time.perf_counter()
                if not timed and j not in measured:
                    continue                                 # the warm-up pass asks only where the timed pass measures
                turns = s.turns()
                t2 = time.perf_counter()
                if j not in measured:
                    continue
                st = d.stage_ms()
                w0 = time.perf_counter()
                whole = d.diarize_dev(d_pcm.data_ptr(), n)
                w1 = time.perf_counter()
                if timed:
                    r = rows[measured[j]]
                    r["push"].append((t1 - t0) * 1e3); r["turns"].append((t2 - t1) * 1e3); r["whole"].append((w1 - w0) * 1e3)
                    r["turn_stages"].append(st); r["whole_stages"].append(d.stage_ms())
                    if (measured[j], j) in [(l, k) for l, k in MARKS]:
                        equal[measured[j]] = (turns == whole, len(turns), s.info())
    one_pass(False)
    one_pass(True)
    d.set_planted(0, 0, 0, 0)
    med = lambda v: float(np.median(np.array(v), axis=0)) if np.ndim(v) == 1 else [float(x) for x in np.median(np.array(v), axis=0)]
    lines = ["stream_times: planted hour (seed 1234), 10 s pieces, turns() after every piece, precision %s; medians of five updates around each size, ms" % a.precision,
             "%-7s %9s %9s %9s | %12s | turns() = pending seg + emb + finalize | diarize_dev = seg + emb + finalize | same turns" % ("prefix", "push", "turns()", "update", "diarize_dev")]
    for label, k in MARKS:
        r = rows[label]
        ts, wsg = med(r["turn_stages"]), med(r["whole_stages"])
        ok, nt, info = equal[label]
        lines.append("%-7s %9.2f %9.2f %9.2f | %12.2f | %.2f + %.2f + %.2f | %.2f + %.2f + %.2f | %s (%d turns, %d/%d chunks sealed)"
                     % (label, med(r["push"]), med(r["turns"]), med(r["push"]) + med(r["turns"]), med(r["whole"]), ts[0], ts[1], ts[2], wsg[0], wsg[1], wsg[2],
                        "yes" if ok else "NO", nt, info[1], info[2]))
        lines.append("        push of the five: %s; turns(): %s; diarize_dev: %s" % tuple(" ".join("%.1f" % x for x in r[q]) for q in ("push", "turns", "whole")))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    d.close()
    return 0 if all(v[0] for v in equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
