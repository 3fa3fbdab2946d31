"""GPU tests of the jobs sd_linkage_many runs one per XCD (option "linkage_batch_xcd"; k_linkage_rg_jobs, linkage_rg.hip; run_linkage_many, linkage_batch.hip):
the dendrogram of every job of a call is, byte for byte, what sd_linkage_ex gives for that job alone under the same options -- whatever else is in the call, in
whatever order, in however many launches and groups, ties, failures and refused allocations included.  The only tolerance is equality.  Most cases are kept
small by forcing the geometry ("linkage_wgs", "linkage_square" = 1): every job of two rows and more is then of the class."""
import contextlib

import numpy as np
import pytest

import sdhip
import synth
from stream_cases import pcm75
from test_linkage_many import ERR_ARG, ERR_NUMERIC, lattice, metric_of, raw_call, rows, same

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 33, 64, 65, 130, 257, 513, 1025)
DEFAULTS = {"linkage_wgs": -1, "linkage_square": -1, "linkage_batch_xcd": 0, "linkage_batch_bytes": 2 << 30, "linkage_batch": 0}


@contextlib.contextmanager
def options(d, **kw):
    """set the keys, and put every one of them back"""
    try:
        for k, v in kw.items():
            d.set_option(k, v)
        yield
    finally:
        for k in kw:
            d.set_option(k, DEFAULTS[k])


def forced(d, wgs, **kw):
    return options(d, linkage_wgs=wgs, linkage_square=1, linkage_batch_xcd=1, **kw)


def launches(d, *names):
    return [d.kernel_stats(n)["launches"] for n in names]


def xcd_bytes(n, G):
    return 8 * n * n + 4 * 2 * (n + n % 2) + 2 * 8 * n + 32 * (n - 1) + 2 * G * 40 * 8 + 32 * 4


@pytest.fixture(scope="module")
def singles(diarizer):
    """sd_linkage_ex per job under the forced geometry, computed once per (key, workgroups, method)"""
    memo = {}

    def get(Xs, key, wgs, method):
        k = (key, wgs, method)
        if k not in memo:
            with options(diarizer, linkage_wgs=wgs, linkage_square=1):
                memo[k] = [diarizer.linkage_ex(X, method, metric_of(method)) for X in Xs]
        return memo[k]
    return get


@pytest.mark.parametrize("d", [192, 1, 33])
@pytest.mark.parametrize("wgs", [2, 3, 32])
@pytest.mark.parametrize("method", sdhip.LINKAGE_METHODS)
def test_every_size_and_method_matches_the_single_entry(diarizer, singles, method, wgs, d):
    """one register slot per thread and three (1 025 rows on 2 workgroups), workgroups that own no column (N < G), a last workgroup with a short range, and
    jobs of different cap in one launch"""
    Xs = rows(SIZES, d, 100 + d)
    cos1 = d == 1 and metric_of(method) == sdhip.METRIC_COSINE
    if cos1:
        Xs = [np.abs(X) + 0.5 for X in Xs]            # (cosine in one dimension: every distance 0 or 2 -- all ties; keep the rows away from zero)
    ref = singles(Xs, ("sizes", d), wgs, method)
    with forced(diarizer, wgs):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, method, metric_of(method))
        rg_jobs, done, redone = launches(diarizer, "linkage_rg_jobs", "linkage_xcd_jobs", "linkage_xcd_redone")
    assert not st.any()
    for n, z, r in zip(SIZES, Z, ref):
        assert same(z, r), (method, wgs, d, n)
    assert rg_jobs == 2 and done + redone == len(SIZES)          # ten jobs: eight and two
    if d != 1:
        assert redone == 0                                        # (random rows in 33 and 192 dimensions: no two distances equal)


@pytest.mark.parametrize("J,want", [(1, 0), (2, 1), (7, 1), (8, 1), (9, 2), (17, 3)])
def test_number_of_jobs_and_launches(diarizer, singles, J, want):
    sizes = tuple((33, 5, 64, 130, 9, 65, 257, 17)[j % 8] + j // 8 for j in range(17))
    Xs = rows(sizes, 24, 17)
    ref = singles(Xs, "count", 2, "centroid")
    with forced(diarizer, 2):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs[:J], "centroid")
        rg_jobs, done, prep, single = launches(diarizer, "linkage_rg_jobs", "linkage_xcd_jobs", "pdist_sq_jobs", "linkage_rg_launches")
    assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
    assert rg_jobs == want and done == (J if J > 1 else 0) and prep == (1 if J > 1 else 0) and single == (1 if J == 1 else 0)


@pytest.mark.parametrize("method", ["centroid", "average"])
def test_a_job_does_not_depend_on_its_company_or_its_place(diarizer, singles, method):
    Xs = rows(SIZES, 192, 292)
    ref = singles(Xs, ("sizes", 192), 3, method)
    with forced(diarizer, 3):
        Z, _ = diarizer.linkage_many(Xs[::-1], method, metric_of(method))
        assert all(same(z, r) for z, r in zip(Z[::-1], ref))
        order = np.random.default_rng(5).permutation(len(Xs))
        Z, _ = diarizer.linkage_many([Xs[i] for i in order], method, metric_of(method))
        assert all(same(z, ref[i]) for z, i in zip(Z, order))
        # the 130 rows among other company: two strangers, then three
        other = rows((40, 77, 300), 192, 9)
        for company in ([other[0], Xs[6], other[1]], [Xs[6]] + other):
            Z, st = diarizer.linkage_many(company, method, metric_of(method))
            k = 1 if len(company) == 3 else 0
            assert not st.any() and same(Z[k], ref[6])


def test_automatic_geometry_nine_jobs_beside_three_small_ones(diarizer):
    sizes = (1500, 1575, 100, 1650, 1725, 1800, 700, 1875, 1950, 2025, 1499, 2100)
    Xs = rows(sizes, 16, 2100)
    ref = [diarizer.linkage_ex(X, "centroid") for X in Xs]
    names = ("linkage_rg_jobs", "linkage_heap_jobs", "linkage_xcd_jobs", "linkage_xcd_redone", "pdist_sq_jobs", "row_nn_sq_jobs", "linkage_rg_launches")
    with options(diarizer, linkage_batch_xcd=1):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, "centroid")
        got = launches(diarizer, *names)
    assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
    assert got == [2, 1, 9, 0, 1, 1, 0], dict(zip(names, got))
    diarizer.reset_stats()
    Z, st = diarizer.linkage_many(Xs, "centroid")                  # the key at 0: launch for launch what it was
    got = launches(diarizer, *names)
    assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
    assert got == [0, 1, 0, 0, 0, 0, 9], dict(zip(names, got))


def tie_above_zero(n, seed):
    """random rows far from each other (three dimensions, as lattice()), and two pairs of rows exactly 1 apart: the closest pair is not unique at height 1"""
    X = np.random.default_rng(seed).standard_normal((n, 3)) * 100.0
    X[:4] = 0.0
    X[0, 0], X[1, 0], X[2, 1], X[3, 1] = 100.0, 101.0, 100.0, 101.0
    return X


@pytest.mark.parametrize("method", ["centroid", "single", "average"])
def test_exact_ties_are_redone_alone(diarizer, method):
    Xs = [rows((70,), 3, 1)[0], lattice(40, 47), rows((33,), 3, 2)[0], tie_above_zero(50, 3), lattice(100, 107), rows((129,), 3, 4)[0]]
    metric = metric_of(method)
    if metric == sdhip.METRIC_COSINE:
        Xs[3] = Xs[3] / np.linalg.norm(Xs[3], axis=1, keepdims=True)
        Xs[3][2:4] = Xs[3][0:2]                                    # (cosine: two pairs of equal rows elsewhere do it; the tie is at 0 then)
    with options(diarizer, linkage_wgs=2, linkage_square=1):
        ref = [diarizer.linkage_ex(X, method, metric) for X in Xs]
    with forced(diarizer, 2):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, method, metric)
        rg_jobs, done, redone = launches(diarizer, "linkage_rg_jobs", "linkage_xcd_jobs", "linkage_xcd_redone")
    assert not st.any()
    for X, z, r in zip(Xs, Z, ref):
        assert same(z, r), (method, len(X))
    assert (rg_jobs, done, redone) == (1, 3, 3)
    if method == "centroid":
        assert Z[3][0, 2] == 1.0 and Z[3][1, 2] == 1.0 and (Z[1][:, 2] == 0).any() and (Z[4][:, 2] == 0).any()      # the cases are what they claim to be


def test_zero_norm_row_fails_its_own_job_only(diarizer):
    Xs = rows((20, 33, 25, 64, 9), 12, 55)
    Xs[2][11] = 0.0
    Z = np.full((sum(len(X) - 1 for X in Xs), 4), np.nan)
    mark = Z.tobytes()
    st = np.full(5, -1, np.int32)
    with forced(diarizer, 2):
        diarizer.reset_stats()
        assert raw_call(diarizer, Xs, 12, 2, sdhip.METRIC_COSINE, Z, st) == 0
        rg_jobs, done, redone = launches(diarizer, "linkage_rg_jobs", "linkage_xcd_jobs", "linkage_xcd_redone")
    assert st.tolist() == [0, 0, ERR_NUMERIC, 0, 0] and (rg_jobs, done, redone) == (1, 4, 0)
    off = np.concatenate([[0], np.cumsum([len(X) - 1 for X in Xs])])
    with options(diarizer, linkage_wgs=2, linkage_square=1):
        for j, X in enumerate(Xs):
            z = Z[off[j]:off[j + 1]]
            if j == 2:
                assert z.tobytes() == mark[:z.nbytes]                          # untouched: still the NaN pattern
            else:
                assert same(z, diarizer.linkage_ex(X, "average", sdhip.METRIC_COSINE))


def test_group_budget_and_a_job_over_it(diarizer, singles):
    Xs = rows((65,) * 4 + (130,) + (65,) * 3, 24, 65)
    ref = singles(Xs, "budget", 2, "centroid")
    assert xcd_bytes(130, 2) > 3 * xcd_bytes(65, 2) + 8
    with forced(diarizer, 2, linkage_batch_bytes=3 * xcd_bytes(65, 2) + 8):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, "centroid")
        got = launches(diarizer, "linkage_rg_jobs", "pdist_sq_jobs", "linkage_xcd_jobs", "linkage_rg_launches")
    assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
    assert got == [3, 3, 7, 1]          # seven jobs in groups of three, three and one; the 130 rows, alone over the budget, went through run_linkage


def test_workspaces_that_cannot_be_allocated_are_halved(weights):
    """six jobs of 300 rows need 4.3 MB of square matrices; under a 1 MB limit the six fail, each half of three fails, of each half the one job runs and the two
    fail and run one by one -- a context of its own, so that no workspace is large enough from an earlier call"""
    d = sdhip.Diarizer(weights[0], weights[1])
    try:
        Xs = rows((300,) * 6, 8, 77)
        with options(d, linkage_wgs=2, linkage_square=1):
            ref = [d.linkage_ex(X, "centroid") for X in Xs]
        try:
            with forced(d, 2):
                d.set_option("ws_limit_mb", 1)
                d.reset_stats()
                Z, st = d.linkage_many(Xs, "centroid")
                got = launches(d, "linkage_batch_alloc_failed", "linkage_rg_jobs", "linkage_xcd_jobs", "linkage_rg_launches")
        finally:
            d.set_option("ws_limit_mb", 0)
        assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
        assert got == [5, 6, 6, 0]
    finally:
        d.close()


def job_bytes(d, j, g):
    d.many_select(j)
    cen, cnt = d.last_speakers()
    return np.array([(s, e, l) for s, e, l in g], np.float64).tobytes(), d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes()


def group_both(d, call):
    """a group call under linkage_batch = 1 and the forced geometry, the key at 1 and at 0 -> (bytes per job, k_linkage_rg_jobs launches) of each"""
    res = {}
    for key in (1, 0):
        with options(d, linkage_batch=1, linkage_wgs=2, linkage_square=1, linkage_batch_xcd=key):
            d.reset_stats()
            out = [job_bytes(d, j, g) if isinstance(g, list) else g for j, g in enumerate(call())]
            res[key] = (out, d.kernel_stats("linkage_rg_jobs")["launches"], d.kernel_stats("linkage_rg_launches")["launches"])
    return res


def test_group_calls_give_the_same_bytes(diarizer):
    recs = [synth.make_pcm(s + 1.0, seed=5300 + r)[:int(s * 16000) + 17 * r].copy() for r, s in enumerate((20.0, 33.0, 45.0, 60.0))]
    res = group_both(diarizer, lambda: diarizer.diarize_many(recs))
    assert res[1][0] == res[0][0] and all(isinstance(r, tuple) and len(r[0]) > 0 for r in res[1][0])
    assert res[1][1] > 0 and res[0][1] == 0 and res[0][2] >= 2          # with the key: shared launches; without: each job's own cooperative launch
    pcm = pcm75()
    streams = [diarizer.stream() for _ in range(3)]
    try:
        for rnd in range(2):
            diarizer.stream_push_many(streams, [pcm[96000 * i + rnd * 200000 + 13 * i * rnd:96000 * i + (rnd + 1) * 200000 + 31 * i] for i in range(3)])
        res = group_both(diarizer, lambda: diarizer.stream_turns_many(streams))
        assert res[1][0] == res[0][0] and all(isinstance(r, tuple) and len(r[0]) > 0 for r in res[1][0])
        assert res[1][1] > 0 and res[0][1] == 0
    finally:
        for s in streams:
            s.close()


def test_the_key_takes_zero_and_one(diarizer):
    for bad in (2, -1):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.set_option("linkage_batch_xcd", bad)
        assert e.value.code == ERR_ARG
    diarizer.set_option("linkage_batch_xcd", 1)
    diarizer.set_option("linkage_batch_xcd", 0)
