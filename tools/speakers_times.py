"""What the known-speaker entries cost: tools/speakers_times.py [--out FILE] [--parent-lib PATH]
All in one process, medians of five after a warm-up, host clock around calls that end in a device synchronise:
  * diarize_dev of the planted hour (synth, seed 1234; scores and embeddings planted as bench.py plants them) on this library and, alternating with it,
    on the library of the parent commit given with --parent-lib (built from that commit's tree): the only addition on that path is the K x 192 f64
    copy of the centroids, which rides a synchronisation run_clustering already performs.  The median of this library must lie inside the parent's own
    min - max of five;
  * voiceprint_dev of a 30 s span of that hour and of the whole hour (the embedding network over the windows the spans touch);
  * speaker_distances at K = 4 for M = 1 000 and M = 100 000 rows of 192: the call (uploads and the download included) and the kernel alone (event
    time under option "profile"), with the bytes per second the kernel time implies against the HBM figures of MI355X_MICROARCH.md."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd"))
import sdhip, synth, weightpack as nn      # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12     # bytes / s: float4 copy measured, data sheet


class ParentLib:
    """the parent commit's libsdhip.so through its C ABI: create, planted hook, sd_diarize_dev"""

    def __init__(self, path, seg, emb):
        L = C.CDLL(path)
        vp, i64 = C.c_void_p, C.c_int64
        L.sd_create.restype = vp
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [vp]
        L.sd_set_planted.argtypes = [vp, vp, vp, i64, i64]
        L.sd_diarize_dev.argtypes = [vp, vp, i64, C.POINTER(C.POINTER(sdhip.Turn)), C.POINTER(i64)]
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        self.L, self.h = L, L.sd_create(seg.encode(), emb.encode(), 0)
        if not self.h:
            raise RuntimeError("sd_create of the parent library failed")

    def set_planted(self, sc, pe, lo, n):
        assert self.L.sd_set_planted(self.h, C.c_void_p(sc or None), C.c_void_p(pe or None), lo, n) == 0

    def diarize_dev(self, ptr, n):
        p, nt = C.POINTER(sdhip.Turn)(), C.c_int64(0)
        rc = self.L.sd_diarize_dev(self.h, C.c_void_p(ptr), n, C.byref(p), C.byref(nt))
        assert rc == 0, rc
        out = [(p[i].start, p[i].end, int(p[i].label)) for i in range(nt.value)]
        self.L.sd_free_turns(p)
        return out

    def close(self):
        self.L.sd_destroy(self.h)


def timed(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    sec = 3600.0
    pcm = synth.make_pcm(sec, seed=1234)
    n = len(pcm)
    nc = synth.num_chunks(n)
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(sec, 1234)), n, 0, nc)
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_sc, d_pe = torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
    torch.cuda.synchronize()
    lines = ["speakers_times: planted hour (seed 1234, %d chunks); medians of five after a warm-up, ms" % nc]
    ok = True

    # ---- the plain job, this commit against its parent, alternating
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    parent = ParentLib(a.parent_lib, seg, emb) if a.parent_lib else None
    if parent:
        parent.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    runs = {"this": [], "parent": []}
    turns = {}
    for it in range(7):                                  # two warm-up rounds: the first call of a context plans the small arena
        for who, obj in (("parent", parent), ("this", d)):
            if obj is None:
                continue
            t0 = time.perf_counter()
            turns[who] = obj.diarize_dev(d_pcm.data_ptr(), n)
            if it >= 2:
                runs[who].append((time.perf_counter() - t0) * 1e3)
    K = len(d.last_speakers()[1])
    d.set_planted(0, 0, 0, 0)
    med = float(np.median(runs["this"]))
    lines.append("diarize_dev, this commit : median %.2f  (min %.2f, max %.2f)  five: %s; %d turns, K = %d" %
                 (med, min(runs["this"]), max(runs["this"]), " ".join("%.2f" % x for x in runs["this"]), len(turns["this"]), K))
    if parent:
        lo, hi = min(runs["parent"]), max(runs["parent"])
        inside = lo <= med <= hi
        ok = ok and inside and turns["this"] == turns["parent"]
        lines.append("diarize_dev, parent      : median %.2f  (min %.2f, max %.2f)  five: %s; same turns: %s" %
                     (float(np.median(runs["parent"])), lo, hi, " ".join("%.2f" % x for x in runs["parent"]), "yes" if turns["this"] == turns["parent"] else "NO"))
        lines.append("this commit's median inside the parent's min - max: %s" % ("yes" if inside else "NO"))
        parent.close()

    # ---- voiceprints
    for label, spans in (("30 s span", [(600.0, 630.0, 0)]), ("whole hour", None)):
        res = {}

        def f():
            res["v"] = d.voiceprint_dev(d_pcm.data_ptr(), n, spans)
        ms = timed(f)
        lines.append("voiceprint_dev, %-10s: median %.2f  five: %s; %d windows, embedding stage %.2f" %
                     (label, float(np.median(ms)), " ".join("%.2f" % x for x in ms), res["v"][1], d.stage_ms()[1]))

    # ---- distances
    rng = np.random.default_rng(1)
    cen = rng.standard_normal((4, sdhip.EMB_DIM))
    for M in (1000, 100000):
        gal = rng.standard_normal((M, sdhip.EMB_DIM))
        call = timed(lambda: d.speaker_distances(gal, cen))
        d.set_option("profile", 1)
        kern = []
        for _ in range(6):
            d.reset_stats()
            d.speaker_distances(gal, cen)
            kern.append(d.kernel_stats("speaker_dist")["ms"])
        d.set_option("profile", 0)
        d.reset_stats()
        k_ms = float(np.median(kern[1:]))
        nbytes = M * sdhip.EMB_DIM * 8.0 + 4 * M * 8.0
        bps = nbytes / (k_ms * 1e-3)
        lines.append("speaker_distances, K = 4, M = %6d: call median %.3f (uploads of %.1f MB included), kernel median %.4f  five: %s; %.1f MB -> %.3f TB/s = %.1f %% of the "
                     "measured HBM copy rate (6.29 TB/s), %.1f %% of the data sheet's 8.0" %
                     (M, float(np.median(call)), nbytes / 1e6, k_ms, " ".join("%.4f" % x for x in kern[1:]), nbytes / 1e6, bps / 1e12, 100.0 * bps / HBM_MEASURED, 100.0 * bps / HBM_SPEC))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(text)
    d.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
