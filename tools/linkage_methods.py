#!/usr/bin/env python3
"""Linkage time per method on the clustering input of the bench's own planted hour (the embeddings of a real job, NaN rows dropped), and which
kernel ran: centroid / median / ward on the unit-normalised rows with euclidean distances, single / complete / average / weighted on the rows
as they are with the cosine metric -- what run_clustering does under option "clustering_method" (clustering/Clustering.py:317-333).
`reps` rounds after a warm-up round; prints every time and the medians.
    python tools/linkage_methods.py [reps]"""
import os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
sys.path.insert(0, ROOT); sys.path.insert(0, PKG)
import torch, sdhip, synth, weightpack as nn
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
tmp = tempfile.mkdtemp()
nn.save_pack(tmp + "/s.sdw", nn.synth_segmentation_weights(4321)); nn.save_pack(tmp + "/e.sdw", nn.synth_embedding_weights(4322))
d0 = sdhip.Diarizer(tmp + "/s.sdw", tmp + "/e.sdw", 0)
pcm = synth.make_pcm(3600, seed=1234)
n = len(pcm)
dev = torch.device("cuda", 0)
d_pcm = torch.from_numpy(pcm).to(dev)
nc = synth.num_chunks(n)
sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(3600, 1234)), n, 0, nc)
d_sc, d_pe = torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
d0.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
torch.cuda.synchronize()
turns = d0.diarize_dev(d_pcm.data_ptr(), n)
e = d0.read_ws("dz_emb", np.float32, nc * 3 * 192).reshape(-1, 192)
d0.close()
X = e[~np.isnan(e[:, 0])].astype(np.float64)
Xn = X / np.sqrt((X * X).sum(1)).astype(np.float32).astype(np.float64)[:, None]
N = len(X)
print("clustering input of the planted hour: N = %d rows (%d turns)" % (N, len(turns)), flush=True)
d = sdhip.Diarizer(None, None)
d.set_option("profile", 1)
KEYS = ("linkage", "linkage_hx", "linkage_heap", "pdist")
COUNTS = ("linkage_rg_launches", "linkage_hx_jobs", "linkage_fallbacks", "linkage_tie_fallbacks", "linkage_method_replays", "linkage_zero_phase_jobs")
res = {}
for r in range(reps + 1):
    for method in sdhip.LINKAGE_METHODS:
        euclid = method in ("centroid", "median", "ward")
        d.reset_stats()
        Z = d.linkage_ex(Xn if euclid else X, method, sdhip.METRIC_EUCLIDEAN if euclid else sdhip.METRIC_COSINE)
        ms = {k: d.kernel_stats(k)["ms"] for k in KEYS}
        cnt = {k: d.kernel_stats(k)["launches"] for k in COUNTS}
        route = "k_linkage_rg" if cnt["linkage_rg_launches"] and not cnt["linkage_fallbacks"] else \
                "k_linkage_rg -> tie -> " + ("zero phase + k_linkage_rg" if cnt["linkage_zero_phase_jobs"] else "k_linkage_hx") if cnt["linkage_rg_launches"] else \
                "k_linkage_hx" if cnt["linkage_hx_jobs"] else "k_linkage_heap"
        if r > 0:
            res.setdefault(method, []).append((ms["linkage"] + ms["linkage_hx"] + ms["linkage_heap"], ms["pdist"], route))
            print("round %d  %-9s %-9s linkage %8.2f ms (cooperative %7.2f, replay %7.2f, one workgroup %7.2f)  pdist %6.2f ms  %s  top height %.6f" % (
                r, method, "euclidean" if euclid else "cosine", ms["linkage"] + ms["linkage_hx"] + ms["linkage_heap"], ms["linkage"], ms["linkage_hx"], ms["linkage_heap"],
                ms["pdist"], route, Z[-1, 2]), flush=True)
print("medians over %d rounds, N = %d:" % (reps, N))
for method in sdhip.LINKAGE_METHODS:
    v = sorted(x[0] for x in res[method]); p = sorted(x[1] for x in res[method])
    print("  %-9s linkage median %8.2f ms  min %8.2f  max %8.2f  (%.2f us per merge)   pdist median %6.2f ms   %s" % (
        method, v[len(v) // 2], v[0], v[-1], v[len(v) // 2] * 1e3 / (N - 1), p[len(p) // 2], res[method][-1][2]))
