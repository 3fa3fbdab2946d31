"""The three clustering hyper-parameters of clustering/Clustering.py:251-276 -- linkage method, threshold, minimum cluster size -- from the
kernels up: sd_linkage_ex / sd_cluster_ex (every kernel route, every method, both metrics, ties), the clustering stage and the whole path under
the option keys "clustering_method" / "clustering_threshold" / "min_cluster_size", the command-line flags.

Reference: the installed scipy.  Dendrograms are compared bit for bit (ties included) with scipy's generic algorithm,
scipy.cluster._hierarchy.fast_linkage, on a condensed matrix computed here: euclidean from orc.pdist, cosine from a numpy loop that adds dot,
m1 and m2 one dimension at a time (the reference's rule, sd.cpp:476-498).  A scipy without _hierarchy.fast_linkage falls back to the public
linkage(): exact for single / complete / centroid / median, merge structure + heights to rtol 1e-12 for average / ward / weighted (scipy runs
nn-chain for those: same merges, another rounding order; 8.9e-16 measured between scipy's two algorithms), tie cases skipped (with ties the
dendrogram is not unique and the public function does not follow the generic algorithm)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import sdhip
from oracle import orc

try:
    from scipy.cluster._hierarchy import fast_linkage as _fast_linkage
except Exception:                                            # pragma: no cover  (scipy builds without the private entry)
    _fast_linkage = None

METHODS = ("single", "complete", "average", "centroid", "median", "ward", "weighted")           # index = scipy's method code
EUCLIDEAN_ONLY = ("centroid", "median", "ward")
EXACT_IN_FALLBACK = ("single", "complete", "centroid", "median")
COMBOS = [(m, "euclidean") for m in METHODS] + [(m, "cosine") for m in METHODS if m not in EUCLIDEAN_ONLY]
METRIC = {"euclidean": sdhip.METRIC_EUCLIDEAN, "cosine": sdhip.METRIC_COSINE}
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
needs_generic = pytest.mark.skipif(_fast_linkage is None, reason="tie order is defined by scipy's generic algorithm only")


# ------------------------------------------------------------------ the reference
def _cos_pdist(X):
    """1 - dot / (sqrt(m1) * sqrt(m2)), the three sums sequential in d"""
    X = np.ascontiguousarray(X, np.float64)
    i, j = np.triu_indices(len(X), 1)
    dot = np.zeros(len(i)); m1 = np.zeros(len(i)); m2 = np.zeros(len(i))
    for q in range(X.shape[1]):
        a, b = X[i, q], X[j, q]
        dot += a * b
        m1 += a * a
        m2 += b * b
    return 1.0 - dot / (np.sqrt(m1) * np.sqrt(m2))


def _condensed(X, metric):
    return orc.pdist(X) if metric == "euclidean" else _cos_pdist(X)


def _ref_linkage(X, method, metric):
    y = _condensed(X, metric)
    if _fast_linkage is not None:
        return np.asarray(_fast_linkage(y.copy(), len(X), METHODS.index(method)))
    from scipy.cluster.hierarchy import linkage
    return linkage(y, method=method)


def _assert_same_dendrogram(Z, Z_ref, method):
    if _fast_linkage is not None or method in EXACT_IN_FALLBACK:
        assert np.array_equal(Z, Z_ref)
        return
    s = lambda A: np.column_stack([np.sort(A[:, :2], axis=1), A[:, 3]])
    assert np.array_equal(s(Z), s(Z_ref))
    np.testing.assert_allclose(Z[:, 2], Z_ref[:, 2], rtol=1e-12, atol=0)


def _blobs(seed, N, d, k):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((k, d)) * 3.0
    return cen[rng.integers(0, k, N)] + rng.standard_normal((N, d))


@functools.lru_cache(maxsize=None)
def _small():
    return _blobs(11, 300, 16, 5)


@functools.lru_cache(maxsize=None)
def _large():
    return _blobs(12, 1600, 8, 4)


@functools.lru_cache(maxsize=None)
def _ref(which, method, metric):
    X = {"small": _small, "large": _large, "dup400": _dup400, "dup1600": _dup1600, "lattice": _lattice}[which]()
    Z = _ref_linkage(X, method, metric)
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=None)
def _dup400():
    X = np.random.default_rng(21).standard_normal((200, 6)) + 2.0
    return np.vstack([X, X])


@functools.lru_cache(maxsize=None)
def _dup1600():
    X = _blobs(22, 800, 8, 4)
    return np.vstack([X, X])


@functools.lru_cache(maxsize=None)
def _lattice():
    g = np.arange(6, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_cosine_loop_matches_scipy_and_the_data_has_no_equal_distances():
    from scipy.spatial.distance import pdist
    for X in (_small(), _large()):
        y = _cos_pdist(X)
        assert np.abs(y - pdist(X, "cosine")).max() < 1e-14              # measured 2.2e-15: another summation order, nothing else
        for yy in (y, orc.pdist(X)):
            assert len(np.unique(yy)) == len(yy)                         # "clustered data, no two equal distances"


# ------------------------------------------------------------------ CPU: names, command line, the transcription
def test_linkage_method_names_are_scipys_codes():
    from scipy.cluster import hierarchy
    for code, name in enumerate(METHODS):
        assert sdhip.linkage_method_from_name(name) == code
    codes = getattr(hierarchy, "_LINKAGE_METHODS", None)
    if codes is not None:
        assert {n: sdhip.linkage_method_from_name(n) for n in METHODS} == {n: codes[n] for n in METHODS}
    for bad in ("", "Centroid", "wards", "mean", "centroid "):
        assert sdhip.linkage_method_from_name(bad) == -1
    assert tuple(sdhip.LINKAGE_METHODS) == METHODS and "sd_linkage_ex" in sdhip.EXPORTS and "sd_set_option_f64" in sdhip.EXPORTS


@pytest.mark.parametrize("flags", [["--clustering-method", "mean"], ["--clustering-threshold", "2.5"], ["--clustering-threshold", "nan"],
                                   ["--clustering-threshold", "0.5x"], ["--min-cluster-size", "0"], ["--clustering-method"]])
def test_cli_refuses_a_bad_hyperparameter_before_touching_the_gpu(flags, tmp_path):
    """the paths do not exist: a command line that got as far as opening a model or a device would say so instead of `usage`"""
    out = subprocess.run([EXE, str(tmp_path / "no_seg.sdw"), str(tmp_path / "no_emb.sdw"), str(tmp_path / "no.wav")] + flags,
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 0
    assert "usage" in out.stderr and "sd_create" not in out.stderr and "failed" not in out.stderr
    assert "Speaker_" not in out.stdout


def _py_spec(emb3, method="centroid", threshold=orc.THRESH_F32, mcs_cfg=15, num_clusters=None):
    """scipy transcription of clustering/Clustering.py:305-428 with its three hyper-parameters, followed by the assignment of every
    (chunk, speaker) row (Clustering.py:96-140 as the C++ port does it, sd.cpp:2119-2212) -- modelled on _py_spec of test_next_rows.py, with
    the port's quirks: f32 L2 norm (sd.cpp:332), centroids of the UN-normalised rows.  emb3 [chunks][3][d] with NaN rows -> hard [chunks][3]"""
    from scipy.cluster.hierarchy import fcluster
    from scipy.spatial.distance import cdist
    c, S, d = emb3.shape
    flat = emb3.reshape(c * S, d)
    emb = flat[~np.isnan(flat[:, 0])]
    N = len(emb)
    min_clusters = max(1, min(N, num_clusters or 1))
    max_clusters = max(1, min(N, num_clusters or N))
    if min_clusters == max_clusters:
        num_clusters = min_clusters
    mcs = min(mcs_cfg, max(1, round(0.1 * N)))
    if method in EUCLIDEAN_ONLY:                                                     # Clustering.py:317-324
        nrm = np.sqrt((emb * emb).sum(1)).astype(np.float32).astype(np.float64)
        Z = _ref_linkage(emb / nrm[:, None], method, "euclidean")
    else:                                                                            # Clustering.py:326-330
        Z = _ref_linkage(emb, method, "cosine")
    assert np.abs(Z[:, 2] - threshold).min() > 1e-9                                  # no height a rounding away from the cut
    clusters = fcluster(Z, threshold, criterion="distance") - 1
    cu, cc = np.unique(clusters, return_counts=True)
    large = cu[cc >= mcs]
    nlarge = len(large)
    if nlarge < min_clusters:
        num_clusters = min_clusters
    elif nlarge > max_clusters:
        num_clusters = max_clusters
    if num_clusters is not None:
        _Z = np.copy(Z)
        _Z[:, 2] = np.arange(N - 1)
        best_it, best_nl = N - 1, 1
        for it in np.argsort(np.abs(Z[:, 2] - threshold), kind="stable"):
            if _Z[it, 3] < mcs:
                continue
            clusters = fcluster(_Z, it, criterion="distance") - 1
            cu, cc = np.unique(clusters, return_counts=True)
            large = cu[cc >= mcs]
            nlarge = len(large)
            if abs(nlarge - num_clusters) < abs(best_nl - num_clusters):
                best_it, best_nl = it, nlarge
            if nlarge == num_clusters:
                break
        if best_nl != num_clusters:
            clusters = fcluster(_Z, best_it, criterion="distance") - 1
            cu, cc = np.unique(clusters, return_counts=True)
            large = cu[cc >= mcs]
            nlarge = len(large)
    if nlarge == 0:
        clusters[:] = 0
    else:
        small = cu[cc < mcs]
        if len(small):
            lc = np.vstack([emb[clusters == k].mean(0) for k in large])
            sc = np.vstack([emb[clusters == k].mean(0) for k in small])
            for sk, lk in enumerate(np.argmin(cdist(lc, sc, metric="cosine"), axis=0)):
                clusters[clusters == small[sk]] = large[lk]
            clusters = np.unique(clusters, return_inverse=True)[1]
    K = clusters.max() + 1
    cen = np.vstack([emb[clusters == k].mean(0) for k in range(K)])
    hard = np.zeros(c * S, np.int32)
    ok = ~np.isnan(flat[:, 0])
    hard[ok] = np.argmax(2.0 - cdist(flat[ok], cen, metric="cosine"), axis=1)        # rows without an embedding stay in cluster 0
    return hard.reshape(c, S), clusters


def _stage_input():
    rng = np.random.default_rng(4)                                       # the _data-style input of test_next_rows.py, 10 % NaN rows
    cen = rng.standard_normal((5, 192)) * 2
    X = cen[rng.integers(0, 5, 450)] + 0.9 * rng.standard_normal((450, 192))
    emb = X.astype(np.float32).astype(np.float64).reshape(150, 3, 192)
    emb[np.random.default_rng(3).random((150, 3)) < 0.1] = np.nan
    return emb


THRESHOLDS = (orc.THRESH_F32, 0.5, 1.0)
MIN_SIZES = (15, 1, 20)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("mcs", MIN_SIZES)
def test_transcription_equals_the_oracle_for_centroid(threshold, mcs):
    emb = _stage_input()
    flat = emb.reshape(-1, 192)
    X = flat[~np.isnan(flat[:, 0])]
    hard, train = _py_spec(emb.copy(), "centroid", threshold, mcs)
    lab, K = orc.cluster_embeddings(X, threshold, mcs)
    assert np.array_equal(train, lab) and K == train.max() + 1
    h_ref, K_ref, _ = orc.clustering(emb, threshold=threshold, min_cluster_size=mcs)
    assert np.array_equal(hard, h_ref)


# ------------------------------------------------------------------ GPU 1: every kernel route, every method
ROUTES = {
    "heap": ("small", {}),                                   # N = 300: k_linkage_heap
    "cooperative": ("large", {}),                            # N = 1600, default options: k_linkage_rg, never left
    "replay": ("large", {"linkage_force_heap": 1}),          # k_linkage_hx
    "condensed_kernel": ("large", {"linkage_kernel": 0}),    # k_linkage_mw's place: centroid runs there, the other methods go through the replay
}
STATS = ("linkage_fallbacks", "linkage_rg_launches", "linkage_hx_jobs", "linkage_method_replays", "linkage_zero_phase_jobs")


def _stats(d):
    return {k: d.kernel_stats(k)["launches"] for k in STATS}


@pytest.mark.gpu
@pytest.mark.parametrize("method,metric", COMBOS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_linkage_every_route_every_method(diarizer, route, method, metric):
    which, opts = ROUTES[route]
    X = {"small": _small, "large": _large}[which]()
    Z_ref = _ref(which, method, metric)
    s0 = _stats(diarizer)
    for k, v in opts.items():
        diarizer.set_option(k, v)
    try:
        Z = diarizer.linkage_ex(X, method, METRIC[metric])
    finally:
        diarizer.set_option("linkage_force_heap", 0)
        diarizer.set_option("linkage_kernel", -1)
    s1 = _stats(diarizer)
    delta = {k: s1[k] - s0[k] for k in STATS}
    _assert_same_dendrogram(Z, Z_ref, method)
    if route == "heap":
        assert delta == dict.fromkeys(STATS, 0)
    elif route == "cooperative":            # the job never left the cooperative kernel
        assert delta["linkage_fallbacks"] == 0 and delta["linkage_rg_launches"] == 1 and delta["linkage_hx_jobs"] == 0 and delta["linkage_method_replays"] == 0
    elif route == "replay":
        assert delta["linkage_hx_jobs"] == 1 and delta["linkage_rg_launches"] == 0
    else:
        assert delta["linkage_rg_launches"] == 0
        if method == "centroid":
            assert delta["linkage_fallbacks"] == 0 and delta["linkage_hx_jobs"] == 0
        else:
            assert delta["linkage_method_replays"] == 1 and delta["linkage_hx_jobs"] == 1


# ------------------------------------------------------------------ GPU 2: ties
TIE_CASES = [("dup400", m, "euclidean") for m in METHODS] + [("dup1600", m, "euclidean") for m in METHODS] + \
            [("dup1600", m, "cosine") for m in METHODS if m not in EUCLIDEAN_ONLY] + [("lattice", m, "euclidean") for m in METHODS]


@needs_generic
@pytest.mark.gpu
@pytest.mark.parametrize("which,method,metric", TIE_CASES)
def test_linkage_with_ties_follows_the_generic_algorithm(diarizer, which, method, metric):
    """rows stacked twice: ties at height 0 -- at N = 1600 the zero phase and the hand-over back to k_linkage_rg; the 6 x 6 x 6 integer
    lattice: ties at positive heights, the whole job through the heap replay"""
    X = {"dup400": _dup400, "dup1600": _dup1600, "lattice": _lattice}[which]()
    Z_ref = _ref(which, method, metric)
    assert not np.isnan(Z_ref).any()
    s0 = _stats(diarizer)
    Z = diarizer.linkage_ex(X, method, METRIC[metric])
    s1 = _stats(diarizer)
    assert np.array_equal(Z, Z_ref)
    if which == "dup1600" and metric == "euclidean":                         # (a cosine distance of two equal rows is 0 only up to rounding)
        assert s1["linkage_fallbacks"] - s0["linkage_fallbacks"] == 1          # the cooperative kernel met the tie and handed over
        # the zero phase took the duplicates and k_linkage_rg<METHOD> resumed from that state (sizes and last-rewrite indices handed over): two launches of it
        assert s1["linkage_zero_phase_jobs"] - s0["linkage_zero_phase_jobs"] == 1 and s1["linkage_hx_jobs"] == s0["linkage_hx_jobs"]
        assert s1["linkage_rg_launches"] - s0["linkage_rg_launches"] == 2


# ------------------------------------------------------------------ GPU 3: sd_cluster_ex
@pytest.mark.gpu
@pytest.mark.parametrize("method,metric", COMBOS)
def test_cluster_ex_equals_fcluster_of_the_reference_dendrogram(diarizer, method, metric):
    from scipy.cluster.hierarchy import fcluster
    X = _small()
    Z_ref = _ref("small", method, metric)
    h = np.sort(Z_ref[:, 2])
    for cutoff in (0.5 * h[0], 0.5 * (h[len(h) // 2] + h[len(h) // 2 + 1]), 0.5 * (h[-2] + h[-1]), 2.0 * h[-1]):
        assert np.abs(h - cutoff).min() > 1e-9 * max(1.0, cutoff)
        assert np.array_equal(diarizer.cluster_ex(X, method, METRIC[metric], cutoff), fcluster(Z_ref, cutoff, "distance"))


@pytest.mark.gpu
def test_ex_entries_refuse_bad_method_metric_and_zero_rows(diarizer):
    X = _small()
    for method, metric in ((m, sdhip.METRIC_COSINE) for m in EUCLIDEAN_ONLY):
        for call in (lambda: diarizer.linkage_ex(X, method, metric), lambda: diarizer.cluster_ex(X, method, metric, 1.0)):
            with pytest.raises(sdhip.SdError) as e:
                call()
            assert e.value.code == 1                                        # SD_ERR_ARG, as scipy refuses the combination
    for method, metric in ((7, 0), (-1, 0), ("mean", 0), ("average", 2), ("average", -1)):
        for call in (lambda: diarizer.linkage_ex(X, method, metric), lambda: diarizer.cluster_ex(X, method, metric, 1.0)):
            with pytest.raises(sdhip.SdError) as e:
                call()
            assert e.value.code == 1
    Xz = X.copy()
    Xz[17] = 0.0
    with pytest.raises(sdhip.SdError) as e:
        diarizer.linkage_ex(Xz, "average", sdhip.METRIC_COSINE)
    assert e.value.code == 5                                                # SD_ERR_NUMERIC: zero-norm row
    assert len(diarizer.linkage_ex(Xz, "average", sdhip.METRIC_EUCLIDEAN)) == len(X) - 1
    for key, v in (("clustering_method", 7), ("clustering_method", -1), ("min_cluster_size", 0)):
        with pytest.raises(sdhip.SdError):
            diarizer.set_option(key, v)
    for v in (-0.01, 2.01, float("nan")):
        with pytest.raises(sdhip.SdError):
            diarizer.set_option_f64("clustering_threshold", v)
    with pytest.raises(sdhip.SdError):
        diarizer.set_option_f64("no_such_key", 1.0)


# ------------------------------------------------------------------ GPU 4: the clustering stage
@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_clustering_stage_follows_the_python_spec(diarizer, method):
    """ward / 0.5 has no cluster that reaches the size: the all-zero branch"""
    emb = _stage_input()
    zero_branch = 0
    try:
        for threshold in THRESHOLDS:
            for mcs in MIN_SIZES:
                for nc in (None, 3):
                    diarizer.set_clustering(method, threshold, mcs)
                    h, K = diarizer.clustering(emb, num_clusters=nc if nc else -1)
                    h_ref, train = _py_spec(emb.copy(), method, threshold, mcs, nc)
                    zero_branch += int(not train.any() and nc is None)
                    assert np.array_equal(h, h_ref), (method, threshold, mcs, nc)
                    assert K == train.max() + 1
                    if method == "centroid":
                        h_orc, K_orc, _ = orc.clustering(emb, threshold=threshold, min_cluster_size=mcs, num_clusters=nc if nc else -1)
                        assert np.array_equal(h, h_orc) and K == K_orc
    finally:
        diarizer.set_clustering()
    if method == "ward":
        assert zero_branch >= 1


# ------------------------------------------------------------------ GPU 5: the whole path
def _wav_bytes(pcm):
    import struct
    data = pcm.astype(np.int16).tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, 16000, 32000, 2, 16)
    return b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data


@pytest.mark.gpu
def test_whole_path_and_cli_use_the_configured_hyperparameters(diarizer, weights, tmp_path):
    import synth
    from oracle import pipeline_oracle
    pcm = synth.make_pcm(22.0, seed=9)
    wav = pcm.astype(np.float32) / 32768.0
    try:
        diarizer.set_clustering("average", 0.6, 5)
        turns = diarizer.diarize(pcm)
        seg = diarizer.segment(wav)
        nb, masks, count = diarizer.postseg(seg)
        emb = diarizer.embed(wav, masks)
        hard, K = diarizer.clustering(emb.astype(np.float64).reshape(len(seg), 3, 192))
        staged = diarizer.reconstruct(seg, nb, hard, count, len(pcm))
    finally:
        diarizer.set_clustering()
    assert turns == staged and len(turns) >= 1
    p = tmp_path / "a.wav"
    p.write_bytes(_wav_bytes(pcm))
    out = subprocess.run([EXE, weights[0], weights[1], str(p), "--clustering-method", "average", "--clustering-threshold", "0.6", "--min-cluster-size", "5"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert [l for l in out.stdout.splitlines() if l.startswith("[")] == [sdhip.format_turn(t) for t in turns]
    # the three keys back at their defaults: the parent's behaviour, i.e. the oracle's turns behind the networks
    t_default = diarizer.diarize(pcm)
    t_ref = pipeline_oracle.diarize_ref(None, weights[2], weights[3], seg_override=seg, emb_override=emb, wav=wav)
    assert t_default == t_ref


# ------------------------------------------------------------------ GPU 6: defaults untouched
@pytest.mark.gpu
def test_centroid_euclidean_ex_is_sd_linkage(diarizer):
    X = _large()
    Z = diarizer.linkage(X)
    assert np.array_equal(diarizer.linkage_ex(X, "centroid", sdhip.METRIC_EUCLIDEAN), Z)
    assert np.array_equal(Z, orc.ahc(X, orc.THRESH_F32)[1])
    assert np.array_equal(diarizer.cluster_ex(X, "centroid", sdhip.METRIC_EUCLIDEAN, 2.5), diarizer.cluster(X, 2.5))
