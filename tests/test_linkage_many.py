"""GPU tests of sd_linkage_many (csrc/linkage_batch.hip): the dendrogram of every job of a call is, byte for byte, what sd_linkage_ex gives for that job
alone -- whatever else is in the call, in whatever order, in however many groups, on either side of the route boundary.  The only tolerance is equality."""
import ctypes as C

import numpy as np
import pytest

import sdhip
from oracle import orc

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 33, 63, 64, 65, 130, 257)
EUCLID = ("centroid", "median", "ward")
ERR_ARG, ERR_NUMERIC = 1, 5


def metric_of(method):
    return sdhip.METRIC_EUCLIDEAN if method in EUCLID else sdhip.METRIC_COSINE


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def rows(sizes, d, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, d)) for n in sizes]


def lattice(n, seed):
    """points with coordinates 1 .. 4 in three dimensions, duplicates included: every distance occurs many times"""
    return np.random.default_rng(seed).integers(1, 5, (n, 3)).astype(np.float64)


def raw_call(diarizer, Xs, d, method, metric, Z, status, N=None, J=None, hX=True, hN=True, hZ=True, hS=True):
    """sd_linkage_many on buffers the test owns; returns the code"""
    allX = np.ascontiguousarray(np.concatenate([np.asarray(X, np.float64).reshape(-1, d) for X in Xs]))
    N = np.array([len(X) for X in Xs] if N is None else N, np.int64)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
    return sdhip.lib().sd_linkage_many(diarizer._h, p(allX, hX), p(N, hN), len(N) if J is None else J, d, method, metric, p(Z, hZ), p(status, hS))


@pytest.fixture(scope="module")
def singles(diarizer):
    """sd_linkage_ex per job, computed once per (seed, sizes, d, method)"""
    memo = {}

    def get(Xs, key, method):
        k = (key, method)
        if k not in memo:
            memo[k] = [diarizer.linkage_ex(X, method, metric_of(method)) if len(X) >= 2 else np.zeros((0, 4)) for X in Xs]
        return memo[k]
    return get


@pytest.mark.parametrize("d", [192, 1, 33])
@pytest.mark.parametrize("method", sdhip.LINKAGE_METHODS)
def test_every_size_and_method_matches_the_single_entry(diarizer, singles, method, d):
    Xs = rows(SIZES, d, 100 + d)
    if d == 1 and metric_of(method) == sdhip.METRIC_COSINE:
        Xs = [np.abs(X) + 0.5 for X in Xs]            # (cosine in one dimension: every distance 0 or 2 -- all ties; keep the rows away from zero)
    ref = singles(Xs, ("sizes", d), method)
    Z, st = diarizer.linkage_many(Xs, method, metric_of(method))
    assert not st.any()
    for n, z, r in zip(SIZES, Z, ref):
        assert same(z, r), (method, d, n)


@pytest.mark.parametrize("method", ["centroid", "average"])
def test_a_job_does_not_depend_on_its_company_or_its_place(diarizer, singles, method):
    Xs = rows(SIZES, 192, 292)
    ref = singles(Xs, ("sizes", 192), method)
    Z, _ = diarizer.linkage_many(Xs[::-1], method, metric_of(method))
    for z, r in zip(Z[::-1], ref):
        assert same(z, r)
    for X, r in zip(Xs, ref):
        (z,), st = diarizer.linkage_many([X], method, metric_of(method))
        assert same(z, r) and st[0] == 0


@pytest.mark.parametrize("method", ["centroid", "single", "complete", "average"])
def test_exact_ties_take_the_merge_order_of_the_heap(diarizer, method):
    Xs = [lattice(n, 7 + n) for n in (40, 64, 100)]
    Z, st = diarizer.linkage_many(Xs, method, metric_of(method))
    assert not st.any()
    for X, z in zip(Xs, Z):
        assert same(z, diarizer.linkage_ex(X, method, metric_of(method))), (method, len(X))
        assert len(np.unique(X, axis=0)) < len(X) and (method != "centroid" or (z[:, 2] == 0).any())      # the case is what it claims to be: duplicate rows
    if method == "centroid":
        assert same(Z[1], orc.linkage_centroid(orc.pdist(Xs[1]), len(Xs[1])))


@pytest.mark.parametrize("metric", [sdhip.METRIC_EUCLIDEAN, sdhip.METRIC_COSINE])
@pytest.mark.parametrize("N,d", [(65, 33), (129, 192), (64, 1)])
def test_the_three_distance_kernels_agree(diarizer, N, d, metric):
    """k_pdist (one job, condensed), k_pdist_jobs (a job among others) and k_pdist_sq (one job, the square matrix) share their tile loop and the value of
    a pair: the dendrogram of the same rows is the same bytes behind each of them.  A tile edge, a row length that is no multiple of the 32-wide stage,
    a single tile.  (The square matrix is the cooperative kernels': two workgroups, centroid.)"""
    method = "centroid" if metric == sdhip.METRIC_EUCLIDEAN else "average"
    rng = np.random.default_rng(1000 * N + d)
    X, *others = [rng.standard_normal((n, d)) for n in (N, 40, 130, 7)]
    if d == 1 and metric == sdhip.METRIC_COSINE:
        X, others = np.abs(X) + 0.5, [np.abs(Y) + 0.5 for Y in others]      # (as above: all ties, rows away from zero)
    ks = lambda name: diarizer.kernel_stats(name)["launches"]
    diarizer.reset_stats()
    alone = diarizer.linkage_ex(X, method, metric)
    assert ks("pdist") == 1 and ks("linkage_heap") == 1 and ks("pdist_jobs") == 0
    Z, st = diarizer.linkage_many([others[0], X, others[1], others[2]], method, metric)
    assert not st.any() and ks("pdist_jobs") == 1 and ks("pdist") == 1
    assert same(Z[1], alone)
    if method == "centroid":
        rg0 = ks("linkage_rg_launches")
        try:
            diarizer.set_option("linkage_wgs", 2)
            diarizer.set_option("linkage_square", 1)
            square = diarizer.linkage_ex(X, method, metric)
        finally:
            diarizer.set_option("linkage_wgs", -1)
            diarizer.set_option("linkage_square", -1)
        assert ks("linkage_rg_launches") == rg0 + 1 and ks("pdist") == 2 and ks("linkage_heap") == 1
        assert same(square, alone)


def test_more_workgroups_than_compute_units(diarizer):
    rng = np.random.default_rng(300)
    sizes = rng.integers(2, 25, 300)
    Xs = [rng.standard_normal((n, 8)) for n in sizes]
    diarizer.reset_stats()
    Z, st = diarizer.linkage_many(Xs, "centroid")
    assert not st.any() and diarizer.kernel_stats("linkage_heap_jobs")["launches"] == 1
    for X, z in zip(Xs, Z):
        assert same(z, diarizer.linkage_ex(X, "centroid"))


def test_route_boundary_1499_is_batched_1500_is_not(diarizer):
    Xs = rows((1499, 1500, 7), 16, 1500)
    ref = [diarizer.linkage_ex(X, "centroid") for X in Xs]
    diarizer.reset_stats()
    Z, st = diarizer.linkage_many(Xs, "centroid")
    assert not st.any()
    for z, r in zip(Z, ref):
        assert same(z, r)
    ks = diarizer.kernel_stats
    assert ks("linkage_heap_jobs")["launches"] == 1 and ks("pdist_jobs")["launches"] == 1 and ks("row_nn_jobs")["launches"] == 1
    assert ks("linkage_heap")["launches"] == 0 and ks("pdist")["launches"] >= 1                      # the 1500 rows went the single route, and not to the heap kernel
    assert ks("linkage")["launches"] + ks("linkage_hx_jobs")["launches"] >= 1                        # ... but to the cooperative kernel or the replay


@pytest.mark.parametrize("threads", [256, 1024])
def test_group_budget_and_thread_count_do_not_change_a_byte(diarizer, singles, threads):
    Xs = rows(SIZES, 192, 292)
    ref = singles(Xs, ("sizes", 192), "centroid")
    per = [8 * (n * (n - 1) // 2) + 12 * (n + n % 2) + 8 * n + 32 * (n - 1) for n in SIZES]
    try:
        diarizer.set_option("linkage_batch_bytes", per[-2] + per[-3] // 2)      # three groups: 257 alone (a job over the budget is a group of one), 130 alone, the rest
        diarizer.set_option("linkage_batch_threads", threads)
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, "centroid")
        assert diarizer.kernel_stats("linkage_heap_jobs")["launches"] == 3
    finally:
        diarizer.set_option("linkage_batch_bytes", 2 << 30)
        diarizer.set_option("linkage_batch_threads", 0)
    for z, r in zip(Z, ref):
        assert same(z, r)


def test_a_group_whose_workspaces_cannot_be_allocated_is_halved(weights):
    """six jobs of 300 rows need 2.1 MB of condensed matrices; under a 1 MB limit the six fail, each half of three (1.03 MB) fails, and the jobs run in
    groups of one and two -- a context of its own, so that no workspace is large enough from an earlier call"""
    d = sdhip.Diarizer(weights[0], weights[1])
    try:
        Xs = rows((300,) * 6, 8, 77)
        ref = [d.linkage_ex(X, "centroid") for X in Xs]
        try:
            d.set_option("ws_limit_mb", 1)
            d.reset_stats()
            Z, st = d.linkage_many(Xs, "centroid")
            failed, launches = d.kernel_stats("linkage_batch_alloc_failed")["launches"], d.kernel_stats("linkage_heap_jobs")["launches"]
        finally:
            d.set_option("ws_limit_mb", 0)
        assert not st.any() and failed == 3 and launches == 4 and d.kernel_stats("linkage_heap")["launches"] == 0
        for z, r in zip(Z, ref):
            assert same(z, r)
    finally:
        d.close()


def test_zero_norm_row_fails_its_own_job_only(diarizer):
    Xs = rows((20, 33, 25, 64, 9), 12, 55)
    Xs[2][11] = 0.0
    nz = sum(len(X) - 1 for X in Xs)
    Z = np.full((nz, 4), np.nan)
    mark = Z.tobytes()
    st = np.full(5, -1, np.int32)
    assert raw_call(diarizer, Xs, 12, 2, sdhip.METRIC_COSINE, Z, st) == 0
    assert st.tolist() == [0, 0, ERR_NUMERIC, 0, 0]
    off = np.concatenate([[0], np.cumsum([len(X) - 1 for X in Xs])])
    for j, X in enumerate(Xs):
        z = Z[off[j]:off[j + 1]]
        if j == 2:
            assert z.tobytes() == mark[:z.nbytes]                          # untouched: still the NaN pattern
            with pytest.raises(sdhip.SdError) as e:
                diarizer.linkage_ex(X, "average", sdhip.METRIC_COSINE)
            assert e.value.code == ERR_NUMERIC
        else:
            assert same(z, diarizer.linkage_ex(X, "average", sdhip.METRIC_COSINE))
    # the euclidean metric knows no such failure
    Z2, st2 = diarizer.linkage_many(Xs, "centroid")
    assert not st2.any() and same(Z2[2], diarizer.linkage_ex(Xs[2], "centroid"))


def test_edge_sizes_and_the_canary_behind_the_output(diarizer):
    rng = np.random.default_rng(3)
    Xs = [np.zeros((0, 5)), rng.standard_normal((1, 5)), rng.standard_normal((2, 5))]
    Z = np.full((1 + 4, 4), np.nan)
    Z[1:] = 1234.5
    st = np.full(3, -1, np.int32)
    assert raw_call(diarizer, Xs, 5, 3, 0, Z, st) == 0
    assert st.tolist() == [0, 0, 0]
    assert same(Z[:1], diarizer.linkage_ex(Xs[2], "centroid")) and (Z[1:] == 1234.5).all()
    # a longer list: the rows behind the last job stay what they were
    Xs = rows((5, 0, 33, 1, 65), 7, 9)
    nz = 4 + 32 + 64
    Z = np.full((nz + 8, 4), -7.25)
    st = np.full(5, -1, np.int32)
    assert raw_call(diarizer, Xs, 7, 5, 0, Z, st) == 0 and not st.any()
    assert (Z[nz:] == -7.25).all()
    assert same(Z[:4], diarizer.linkage_ex(Xs[0], "ward")) and same(Z[4:36], diarizer.linkage_ex(Xs[2], "ward")) and same(Z[36:nz], diarizer.linkage_ex(Xs[4], "ward"))


def test_refusals_leave_the_output_untouched(diarizer):
    Xs = rows((4, 6), 3, 1)
    Z = np.full((8, 4), 99.0)
    st = np.full(2, -3, np.int32)
    bad = [dict(hX=False), dict(hN=False), dict(hZ=False), dict(hS=False), dict(J=0), dict(J=-2), dict(N=[4, -1]), dict(d=0), dict(d=-3),
           dict(N=[2 ** 31 - 1, 1], J=2), dict(N=[2 ** 30, 2 ** 30], J=2), dict(method=7), dict(method=-1), dict(metric=2), dict(metric=-1),
           dict(method=3, metric=1), dict(method=4, metric=1), dict(method=5, metric=1)]
    for kw in bad:
        kw = dict(kw)
        d, method, metric = kw.pop("d", 3), kw.pop("method", 0), kw.pop("metric", 0)
        allX = np.ascontiguousarray(np.concatenate(Xs))
        N = np.array(kw.get("N", [4, 6]), np.int64)
        p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
        rc = sdhip.lib().sd_linkage_many(diarizer._h, p(allX, kw.get("hX", True)), p(N, kw.get("hN", True)), kw.get("J", 2), d, method, metric,
                                         p(Z, kw.get("hZ", True)), p(st, kw.get("hS", True)))
        assert rc == ERR_ARG, kw
        assert (Z == 99.0).all() and (st == -3).all(), kw
    # and the call that is fine
    assert raw_call(diarizer, Xs, 3, 0, 0, Z, st) == 0 and not st.any() and same(Z[:3], diarizer.linkage_ex(Xs[0], "single"))
