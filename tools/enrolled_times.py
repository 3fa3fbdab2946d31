"""What enrolled speakers cost and save: tools/enrolled_times.py [--out FILE] [--seconds S]
All in one process on the planted hour (synth, seed 1234; scores and embeddings planted as bench.py plants them), medians of five after a warm-up, host
clock around calls that end in a device synchronise:
  * finalize_dev without a gallery, with the job's own centroids enrolled at speaker_match_threshold = 2 (every row claimed: no linkage), and with the
    first half of the centroids enrolled at the default threshold (the linkage shrinks to the rows nobody claimed);
  * nearest_speakers of N = 12 989 rows of 192 against M = 4 / 1 000 / 100 000 voiceprints: the call (uploads and downloads included) and the kernel
    alone (event time under option "profile"), with the f64 multiply-adds per second the kernel time implies;
  * stream.turns() with the whole hour pushed, with and without the gallery of the job's own centroids."""
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

N_ROWS = 12989


def timed(f, reps=5, warm=1):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def fmt(ms):
    return "median %.2f  five: %s" % (float(np.median(ms)), " ".join("%.2f" % x for x in ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=3600.0)
    a = ap.parse_args()
    import torch
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    sec = a.seconds
    pcm = synth.make_pcm(sec, seed=1234)
    n = len(pcm)
    nc = synth.num_chunks(n)
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(sec, 1234)), n, 0, nc)
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_sc, d_pe = torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, sdhip.EMB_DIM), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    lines = ["enrolled_times: planted %g s (seed 1234, %d chunks); medians of five after a warm-up, ms" % (sec, nc)]
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    d.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    fin = lambda: d.finalize_dev(d_seg.data_ptr(), d_emb.data_ptr(), nc, n)

    def launches():
        return " ".join("%s %d" % (k, d.kernel_stats(k)["launches"]) for k in ("nearest_gallery", "pdist", "linkage", "linkage_hx", "linkage_heap"))

    # ---- finalize_dev: no gallery, every row claimed, half of the people enrolled
    plain = fin()
    cen, cnt = d.last_speakers()
    n_train = int(cnt.sum())
    lines.append("finalize_dev, no gallery                 : %s; %d turns, K = %d, %d train rows" % (fmt(timed(fin)), len(plain), len(cen), n_train))
    d.set_enrolled(cen)
    d.set_option_f64("speaker_match_threshold", 2.0)
    d.reset_stats()
    turns = fin()
    lines.append("finalize_dev, own centroids, t = 2       : %s; %d turns, K = %d, same turns as the plain job: %s; launches of one job: %s" %
                 (fmt(timed(fin)), len(turns), len(d.last_enrolled()), "yes" if turns == plain else "no", launches()))
    d.set_option_f64("speaker_match_threshold", sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT)
    half = max(1, len(cen) // 2)
    d.set_enrolled(cen[:half])
    d.reset_stats()
    turns = fin()
    rows = d.last_enrolled()
    _, cnt2 = d.last_speakers()
    lines.append("finalize_dev, %d of %d centroids, default t: %s; %d turns, K = %d (%d enrolled), %d of %d train rows claimed; launches of one job: %s" %
                 (half, len(cen), fmt(timed(fin)), len(turns), len(rows), int((rows >= 0).sum()), int(cnt2[rows >= 0].sum()), n_train, launches()))
    d.set_enrolled(None)
    d.reset_stats()

    # ---- the kernel alone
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N_ROWS, sdhip.EMB_DIM))
    for M in (4, 1000, 100000):
        gal = rng.standard_normal((M, sdhip.EMB_DIM))
        call = timed(lambda: d.nearest_speakers(X, gal))
        d.set_option("profile", 1)
        kern = []
        for _ in range(6):
            d.reset_stats()
            d.nearest_speakers(X, gal)
            kern.append(d.kernel_stats("nearest_gallery")["ms"])
        d.set_option("profile", 0)
        d.reset_stats()
        k_ms = float(np.median(kern[1:]))
        fma = float(N_ROWS) * M * sdhip.EMB_DIM
        lines.append("nearest_speakers, N = %d, M = %6d: call median %.3f (uploads of %.1f MB included), kernel median %.4f  five: %s; %.3g f64 multiply-adds -> %.2f T/s" %
                     (N_ROWS, M, float(np.median(call)), (N_ROWS + M) * sdhip.EMB_DIM * 8.0 / 1e6, k_ms, " ".join("%.4f" % x for x in kern[1:]), fma, fma / (k_ms * 1e-3) / 1e12))

    # ---- the stream at the hour
    with d.stream() as s:
        s.push_dev(d_pcm.data_ptr(), n)
        ref = s.turns()
        lines.append("stream.turns(), no gallery               : %s; %d turns" % (fmt(timed(s.turns)), len(ref)))
        d.set_enrolled(cen)
        got = s.turns()
        lines.append("stream.turns(), own centroids, default t : %s; %d turns, %d of %d labels enrolled" %
                     (fmt(timed(s.turns)), len(got), int((d.last_enrolled() >= 0).sum()), len(d.last_enrolled())))
        d.set_option_f64("speaker_match_threshold", 2.0)
        s.turns()
        lines.append("stream.turns(), own centroids, t = 2     : %s" % fmt(timed(s.turns)))
    d.set_option_f64("speaker_match_threshold", sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT)
    d.set_enrolled(None)
    d.set_planted(0, 0, 0, 0)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(text)
    d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
