"""cluster_plan (csrc/cluster_host.h) -- the host arithmetic of one cut of a dendrogram that run_clustering and every cut of sd_cut_turns_many share --
against a Python restatement of clustering/Clustering.py:27-41 (set_num_clusters) and :305-399 (the cut, the size split, the constrained re-cut) on
scipy's fcluster.  No GPU and no libsdhip.so: tools/cluster_plan_check.cpp, which includes that header alone, is built with the address and
undefined-behaviour sanitizers and runs once over all cases.

Where the port differs from the Python on purpose, the restatement follows the port and says so: a re-cut only where the caller constrained the number
of clusters, and a clamp instead of the ValueError for min_clusters > max_clusters (no case here has it).  round(0.1 N): Python rounds a half to even,
the port away from zero (std::round, sd.cpp:2308); the two agree for every N used here (0, 1, 2 and about 405, where 0.1 N lies far above the option)."""
import functools
import itertools
import os
import subprocess

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (orc.THRESH_F32, 0.5, 1.0)
MIN_SIZES = (15, 1, 20)
COUNTS = [(nc, None, None) for nc in (None, 1, 3, 6)] + [(None, mn, mx) for mn, mx in ((2, 3), (5, None), (None, 2))]


@functools.lru_cache(maxsize=None)
def _dendrogram():
    """the train rows of test_clustering_hyperparams._stage_input() and scipy's centroid linkage of their f32-normalised form"""
    from test_clustering_hyperparams import _ref_linkage, _stage_input
    flat = _stage_input().reshape(-1, 192)
    X = flat[~np.isnan(flat[:, 0])]
    nrm = np.sqrt((X * X).sum(1)).astype(np.float32).astype(np.float64)      # the port's f32 norm (sd.cpp:332)
    Xn = X / nrm[:, None]
    Z = _ref_linkage(Xn, "centroid", "euclidean")
    Z2 = _ref_linkage(Xn[:2], "centroid", "euclidean")
    for z in (Z, Z2):
        z.setflags(write=False)
    return Z, Z2


def _plan_ref(Z, N, threshold, mcs_cfg, num_clusters, min_clusters, max_clusters):
    """-> trivial, mcs, nl, labels, large, small, labels of the first cut"""
    from scipy.cluster.hierarchy import fcluster
    constrained = not (num_clusters is None and min_clusters is None and max_clusters is None)
    # set_num_clusters, Clustering.py:27-41
    min_clusters = num_clusters or min_clusters or 1
    min_clusters = max(1, min(N, min_clusters))
    max_clusters = num_clusters or max_clusters or N
    max_clusters = max(1, min(N, max_clusters))
    min_clusters = min(min_clusters, max_clusters)                       # the port clamps where the Python raises
    if min_clusters == max_clusters:
        num_clusters = min_clusters
    mcs = min(mcs_cfg, max(1, round(0.1 * N)))                           # Clustering.py:309-311
    if N < 2 or max_clusters < 2:                                        # one cluster (sd.cpp:2081-2088; Clustering.py:314-315 for N = 1)
        zeros = [0] * N
        return 1, mcs, 1, zeros, [], [], zeros

    def cut(dendrogram, t):
        clusters = fcluster(dendrogram, t, criterion="distance") - 1
        cc = np.bincount(clusters)                                       # = np.unique(clusters, return_counts=True): fcluster leaves no label unused
        return clusters, np.arange(len(cc)), cc

    clusters, cu, cc = cut(Z, threshold)                                 # Clustering.py:333-342
    first = clusters.copy()
    nlarge = int((cc >= mcs).sum())
    if nlarge < min_clusters:                                            # :345-350
        num_clusters = min_clusters
    elif nlarge > max_clusters:
        num_clusters = max_clusters
    if not constrained:
        # the port re-cuts only where the caller constrained the count: with no large cluster the reference's release build takes the all-zero exit
        # (sd.cpp:2371-2375) where Clustering.py:345 would re-cut to one cluster -- every row in cluster 0 either way
        num_clusters = None
    if num_clusters is not None:                                         # :352-396
        _Z = np.copy(Z)
        _Z[:, 2] = np.arange(N - 1)
        best_it, best_nl = N - 1, 1
        for it in np.argsort(np.abs(Z[:, 2] - threshold), kind="stable"):
            if _Z[it, 3] < mcs:
                continue
            clusters, cu, cc = cut(_Z, it)
            nlarge = int((cc >= mcs).sum())
            if abs(nlarge - num_clusters) < abs(best_nl - num_clusters):
                best_it, best_nl = it, nlarge
            if nlarge == num_clusters:
                break
        if best_nl != num_clusters:
            clusters, cu, cc = cut(_Z, best_it)
    return 0, mcs, int(clusters.max()) + 1, clusters.tolist(), cu[cc >= mcs].tolist(), cu[cc < mcs].tolist(), first.tolist()


def _cases():
    Z, Z2 = _dendrogram()
    N = len(Z) + 1
    cases = [(Z, N, t, m) + c for t, m, c in itertools.product(THRESHOLDS, MIN_SIZES, COUNTS)]
    cases.append((Z, N, 0.0, 15, None, None, None))                      # every row a cluster of its own: no cluster is large
    cases.append((Z, N, 0.0, 15, None, 2, 3))                            # ... and the re-cut that a constraint asks for then
    for c in [(None, None, None), (1, None, None), (2, None, None), (None, 2, 3), (None, 5, None), (None, None, 2)]:
        cases.append((Z[:0], 0, orc.THRESH_F32, 15) + c)
        cases.append((Z[:0], 1, orc.THRESH_F32, 15) + c)
        for t in (orc.THRESH_F32, 0.0, 2.0):
            cases.append((Z2, 2, t, 15) + c)
    return cases


def test_cluster_plan_equals_the_python_restatement_under_the_sanitizers(tmp_path):
    exe = tmp_path / "cluster_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "cluster_plan_check.cpp"), "-o", str(exe)])
    Z, Z2 = _dendrogram()
    assert 380 <= len(Z) + 1 <= 430
    for t in THRESHOLDS:
        assert np.abs(Z[:, 2] - t).min() > 1e-9                          # no merge height a rounding away from the cut
    assert Z[:, 2].min() > 1e-9 and 1e-9 < Z2[0, 2] < 2.0 - 1e-9         # ... nor from the cuts at 0 and 2
    cases = _cases()
    u = lambda v: -1 if v is None else v
    text = []
    for Zc, N, t, m, nc, mn, mx in cases:
        text.append("%d %s %d %d %d %d" % (N, repr(float(t)), m, u(nc), u(mn), u(mx)))
        text.append(" ".join(repr(float(z)) for z in Zc.ravel()))
    out = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    seen = set()
    for (Zc, N, t, m, nc, mn, mx), line in zip(cases, lines):
        head, lab, large, small, first = [[int(x) for x in part.split()] for part in line.split("|")]
        trivial, mcs, nl, r_lab, r_large, r_small, r_first = _plan_ref(Zc, N, t, m, nc, mn, mx)
        what = (N, t, m, nc, mn, mx)
        assert head == [trivial, mcs, nl], what
        assert lab == r_lab and first == r_first, what
        assert large == r_large and small == r_small, what
        seen.add((bool(trivial), lab != first, not large, bool(small)))
    # the cases reach every branch: the trivial exit, a re-cut, no large cluster, small clusters next to large ones and none at all
    assert {s[0] for s in seen} == {True, False} and any(s[1] for s in seen) and any(s[2] and not s[0] for s in seen)
    assert any(s[3] and not s[2] for s in seen) and any(not s[3] and not s[2] and not s[0] for s in seen)
