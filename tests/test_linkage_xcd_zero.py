"""GPU tests of option "linkage_batch_xcd_zero": a job of an XCD launch of sd_linkage_many (option "linkage_batch_xcd") that stops at a tie at height 0 in front
of its first merge -- duplicate rows -- stays in the batch (k_linkage_hx_jobs, k_prepare_zero_jobs, k_row_nn_mid_jobs, k_linkage_rg_jobs<M, true>;
run_linkage_many, linkage_batch.hip).  The dendrogram of every job of a call is, byte for byte, what sd_linkage_ex gives for that job alone under
the same options; the only tolerance is equality.  Where a job must land (done by the first launch, finished by the zero launches, redone alone) is read from
the counters of its run alone, and for centroid written out as well.  Cases are kept small by the forced geometry of tests/test_linkage_xcd.py ("linkage_wgs",
"linkage_square" = 1).  Every case sets the key and fails where the key is refused."""
import contextlib

import numpy as np
import pytest

import sdhip
import synth
from stream_cases import pcm75
from test_linkage_many import ERR_ARG, ERR_NUMERIC, lattice, metric_of, raw_call, rows, same
from test_linkage_xcd import job_bytes, tie_above_zero

pytestmark = pytest.mark.gpu

SIZES = (3, 4, 5, 33, 65, 130, 257, 513, 1025)
DEFAULTS = {"linkage_wgs": -1, "linkage_square": -1, "linkage_batch_xcd": 0, "linkage_batch_xcd_zero": 0, "linkage_batch_bytes": 2 << 30, "linkage_batch": 0,
            "linkage_zero_phase": 1, "linkage_tie_kernel": 1, "linkage_hx_wide": 0}
NAMES = ("linkage_rg_jobs", "linkage_hx_zero_jobs", "linkage_rg_cont_jobs", "linkage_xcd_jobs", "linkage_xcd_zero_jobs", "linkage_xcd_redone")
DONE, ZERO_ALL, ZERO_CONT, ZERO_REDO, REDO = "done by the first launch", "all merges at height 0", "zero launch and continuation", "zero launch, then redone", "redone"


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


def forced(d, wgs, zero=1, **kw):
    return options(d, linkage_wgs=wgs, linkage_square=1, linkage_batch_xcd=1, linkage_batch_xcd_zero=zero, **kw)


def launches(d, *names):
    return [d.kernel_stats(n)["launches"] for n in names]


def duplicates(n, d, seed, wgs=2, exact=True):
    """random normal rows, some of them copied into others: a pair at rows 0 and n - 1, a pair on both sides of a workgroup's column boundary, a triple around a
    worker's column boundary (31 workers) and a five-fold anywhere.  3 rows: all equal; 4: two pairs; 5: one pair only (the closest pair is unique)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    if n == 3:
        groups = [[0, 1, 2]]
    elif n == 4:
        groups = [[0, 3], [1, 2]]
    elif n == 5:
        groups = [[1, 4]]
    elif n < 16:
        groups = [[0, n - 1], [1, 2]]
    else:
        b, hb = -(-n // wgs), -(-n // 31)
        used, groups = set(), []
        for want in ([0, n - 1], [b - 1, b], [hb - 1, hb, n // 3], [int(v) for v in rng.choice(n, 5, replace=False)]):
            g = []
            for i in want:
                while i % n in used:
                    i += 1
                used.add(i % n)
                g.append(i % n)
            groups.append(g)
    for g in groups:
        while exact and not cosine_zero(X[g[0]]):
            X[g[0]] = rng.standard_normal(d)
        X[g[1:]] = X[g[0]]
    return X


def cosine_zero(x):
    """is the cosine distance of a row to its copy exactly 0?  The rule of cosine_rule.h on the sum the distance kernels form, sequential in the element index:
    1 - m / (sqrt(m) * sqrt(m)), which is 0 for about every second row and +-1.1e-16 for the others.  Copied rows are drawn until it is 0, so that the copies
    tie at height 0 under both metrics (under the euclidean one any row does)"""
    m = 0.0
    for v in x.tolist():
        m += v * v
    s = float(np.sqrt(np.float64(m)))
    return 1.0 - m / (s * s) == 0.0


def alone(d, X, method):
    """sd_linkage_ex of one job (the caller has forced the geometry) -> (Z, where the job must land in a batch): read from the counters of this run.
    No tie fallback: done by the first launch.  Zero phase completed, or every merge at height 0: finished by the zero launches.  Anything else: redone.
    One more counter tells the tie in front of the first merge, which the batch keeps, from the tie at height 0 that shows behind a merge (one row with two
    neighbours at the merge height and no other row at that bound: k_linkage_rg sees it after the merge's stores), which is redone alone by design: alone
    the matrix is then built again before the zero phase, one "pdist" more than the job needs otherwise (1 with a completed zero phase, 2 with a whole
    replay behind it)."""
    d.reset_stats()
    Z = d.linkage_ex(X, method, metric_of(method))
    tie, zero_done, pdist = launches(d, "linkage_tie_fallbacks", "linkage_zero_phase_jobs", "pdist")
    merges = d.kernel_stats("linkage_zero_phase_merges")["flops"]
    route = DONE if not tie else ZERO_CONT if zero_done else ZERO_ALL if merges == len(X) - 1 else ZERO_REDO if merges > 0 else REDO
    if route in (ZERO_CONT, ZERO_ALL, ZERO_REDO) and pdist != (2 if route == ZERO_REDO else 1):
        route = REDO
    return Z, route


def expected(sizes, routes):
    """the six counters of NAMES for a call whose jobs (one group, one key) land as `routes` say: launches of at most eight in plan order (descending N, stable)"""
    order = sorted(range(len(sizes)), key=lambda j: -sizes[j])
    zero = [routes[j] for j in order if routes[j] in (ZERO_ALL, ZERO_CONT, ZERO_REDO)]
    chunks = [zero[i:i + 8] for i in range(0, len(zero), 8)]
    return [-(-len(sizes) // 8), len(chunks), sum(any(r != ZERO_ALL for r in ch) for ch in chunks),
            sum(r == DONE for r in routes), sum(r in (ZERO_ALL, ZERO_CONT) for r in routes), sum(r in (ZERO_REDO, REDO) for r in routes)]


@pytest.fixture(scope="module")
def singles(diarizer):
    """(Z, route) per job alone under the forced geometry, computed once per (key, workgroups, method)"""
    memo = {}

    def get(Xs, key, wgs, method):
        k = (key, wgs, method)
        if k not in memo:
            with options(diarizer, linkage_wgs=wgs, linkage_square=1):
                memo[k] = [alone(diarizer, X, method) for X in Xs]
        return memo[k]
    return get


def check(diarizer, Xs, ref, method, wgs, **kw):
    """one call with the key at 1: every Z the bytes of the job alone, the six counters what the routes alone say"""
    with forced(diarizer, wgs, **kw):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, method, metric_of(method))
        got = launches(diarizer, *NAMES)
    assert not st.any()
    for X, z, (r, route) in zip(Xs, Z, ref):
        assert same(z, r), (method, wgs, len(X), route)
    want = expected([len(X) for X in Xs], [route for _, route in ref])
    print(method, wgs, "got", got, "want", want, [(len(X), route) for X, (_, route) in zip(Xs, ref)])
    assert got == want, "got %s, want %s of %s" % (got, want, NAMES)
    return got


@pytest.mark.parametrize("d", [192, 33])
@pytest.mark.parametrize("wgs", [2, 3, 32])
@pytest.mark.parametrize("method", sdhip.LINKAGE_METHODS)
def test_every_size_and_method_matches_the_single_entry(diarizer, singles, method, wgs, d):
    """3 rows all equal (every merge at height 0, no continuation), 4 rows in two pairs, 5 rows with one pair (done by the first launch), workgroups and workers
    that own no column, a short last range, three register slots per thread (1 025 rows on 2 workgroups), and jobs of different cap and lc in one zero launch"""
    Xs = [duplicates(n, d, 1000 * d + n, wgs) for n in SIZES]
    ref = singles(Xs, ("sizes", d), wgs, method)
    got = check(diarizer, Xs, ref, method, wgs)
    routes = [route for _, route in ref]
    # equal rows are at distance exactly 0 (euclidean: always; cosine: duplicates() draws such rows): the routes, written out
    assert routes == [ZERO_ALL, ZERO_CONT, DONE] + [ZERO_CONT] * 6
    assert got == [2, 1, 1, 1, 8, 0]
    # the cases are what they claim: merges at height 0 = rows - distinct rows
    for X, (z, _) in zip(Xs, ref):
        assert int((z[:, 2] == 0).sum()) == len(X) - len(np.unique(X, axis=0))
    assert [int((z[:, 2] == 0).sum()) for z, _ in ref] == [2, 2, 1] + [8] * 6


@pytest.mark.parametrize("method", ["single", "complete", "average", "weighted"])
def test_cosine_copies_that_are_not_at_exactly_zero(diarizer, method):
    """any row: the copies of about every second one lie 1.1e-16 from each other, or -1.1e-16 -- ties above 0, below 0, at 0 behind a merge.  Where each job
    lands is what its run alone says"""
    Xs = [duplicates(n, 33, 4400 + n, 2, exact=False) for n in SIZES[3:]] + [duplicates(n, 33, 5500 + n, 2, exact=False) for n in (40, 77, 200)]
    with options(diarizer, linkage_wgs=2, linkage_square=1):
        ref = [alone(diarizer, X, method) for X in Xs]
    check(diarizer, Xs, ref, method, 2)


def centroid_case(key, n, seed):
    return {"free": lambda: rows((n,), 3, seed)[0], "dup": lambda: duplicates(n, 3, seed), "above": lambda: tie_above_zero(n, seed),
            "lattice": lambda: lattice(n, seed)}[key]()


def test_a_mixed_call_every_job_lands_where_it_must(diarizer):
    """tie-free jobs, jobs with duplicates, a tie above 0 (redone), a lattice (merges at height 0, then more ties: zero launch, continuation, redone)"""
    kinds = [("free", 70), ("dup", 40), ("above", 50), ("lattice", 100), ("dup", 129), ("free", 33), ("lattice", 47), ("dup", 3)]
    Xs = [centroid_case(k, n, 11 + n) for k, n in kinds]
    with options(diarizer, linkage_wgs=2, linkage_square=1):
        ref = [alone(diarizer, X, "centroid") for X in Xs]
    want = {"free": DONE, "dup": ZERO_CONT, "above": REDO, "lattice": ZERO_REDO}
    assert [r for _, r in ref] == [want[k] if n > 3 else ZERO_ALL for k, n in kinds]
    assert ref[2][0][0, 2] == 1.0 and ref[2][0][1, 2] == 1.0 and all((ref[j][0][:, 2] == 0).any() for j in (1, 3, 4, 6, 7))
    got = check(diarizer, Xs, ref, "centroid", 2)
    assert got == [1, 1, 1, 2, 3, 3]


def test_a_zero_norm_row_fails_its_own_job_only(diarizer):
    """cosine metric: the failed job's Z is untouched, the duplicate jobs beside it land where their run alone says"""
    Xs = [duplicates(n, 12, 70 + n) for n in (40, 33, 25, 64)] + rows((9,), 12, 5)
    Xs[2][11] = 0.0
    Z = np.full((sum(len(X) - 1 for X in Xs), 4), np.nan)
    mark = Z.tobytes()
    st = np.full(5, -1, np.int32)
    with options(diarizer, linkage_wgs=2, linkage_square=1):
        ref = [alone(diarizer, X, "average") if j != 2 else (None, None) for j, X in enumerate(Xs)]
    with forced(diarizer, 2):
        diarizer.reset_stats()
        assert raw_call(diarizer, Xs, 12, 2, sdhip.METRIC_COSINE, Z, st) == 0
        got = launches(diarizer, *NAMES)
    assert st.tolist() == [0, 0, ERR_NUMERIC, 0, 0]
    off = np.concatenate([[0], np.cumsum([len(X) - 1 for X in Xs])])
    for j, (r, _) in enumerate(ref):
        z = Z[off[j]:off[j + 1]]
        assert z.tobytes() == mark[:z.nbytes] if j == 2 else same(z, r)
    live = [j for j in range(5) if j != 2]
    want = expected([len(Xs[j]) for j in live], [ref[j][1] for j in live])
    assert got[1:] == want[1:] and got[0] == 1 and got[3] + got[4] + got[5] == 4


@pytest.mark.parametrize("method", ["centroid", "average"])
def test_a_job_does_not_depend_on_its_company_or_its_place(diarizer, singles, method):
    Xs = [duplicates(n, 192, 192000 + n, 3) for n in SIZES]
    ref = singles(Xs, ("sizes", 192), 3, method)
    Zs = [z for z, _ in ref]
    with forced(diarizer, 3):
        Z, _ = diarizer.linkage_many(Xs[::-1], method, metric_of(method))
        assert all(same(z, r) for z, r in zip(Z[::-1], Zs))
        order = np.random.default_rng(5).permutation(len(Xs))
        Z, _ = diarizer.linkage_many([Xs[i] for i in order], method, metric_of(method))
        assert all(same(z, Zs[i]) for z, i in zip(Z, order))
        # the 130 rows alone among tie-free strangers: two, then three
        other = rows((40, 77, 300), 192, 9)
        for company in ([other[0], Xs[5], other[1]], [Xs[5]] + other):
            diarizer.reset_stats()
            Z, st = diarizer.linkage_many(company, method, metric_of(method))
            k = 1 if len(company) == 3 else 0
            assert not st.any() and same(Z[k], Zs[5])
            if method == "centroid":
                assert launches(diarizer, *NAMES) == [1, 1, 1, len(company) - 1, 1, 0]


@pytest.mark.parametrize("J,want", [(9, 2), (17, 3)])
def test_zero_launches_of_eight(diarizer, singles, J, want):
    sizes = tuple((33, 6, 64, 130, 9, 65, 257, 17)[j % 8] + j // 8 for j in range(17))
    Xs = [duplicates(n, 24, 17 + 100 * j) for j, n in enumerate(sizes)]
    ref = singles(Xs, "count", 2, "centroid")
    got = check(diarizer, Xs[:J], ref[:J], "centroid", 2)
    assert got == [want, want, want, 0, J, 0]


def test_the_key_at_zero_redoes_every_tie_alone(diarizer):
    """linkage_batch_xcd = 1 with the new key at 0: the counters of test_linkage_xcd.py::test_exact_ties_are_redone_alone, none of the new ones"""
    Xs = [rows((70,), 3, 1)[0], lattice(40, 47), rows((33,), 3, 2)[0], tie_above_zero(50, 3), duplicates(100, 3, 107), rows((129,), 3, 4)[0]]
    with options(diarizer, linkage_wgs=2, linkage_square=1):
        ref = [diarizer.linkage_ex(X, "centroid") for X in Xs]
    for zero, want in ((0, [1, 0, 0, 3, 0, 3]), (1, [1, 1, 1, 3, 1, 2])):
        with forced(diarizer, 2, zero=zero):
            diarizer.reset_stats()
            Z, st = diarizer.linkage_many(Xs, "centroid")
            got = launches(diarizer, *NAMES)
            merges = diarizer.kernel_stats("linkage_xcd_zero_merges")["flops"]
        assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
        assert got == want and (merges > 0) == (zero == 1), (zero, dict(zip(NAMES, got)), merges)


@pytest.mark.parametrize("off", [{"linkage_zero_phase": 0}, {"linkage_tie_kernel": 0}, {"linkage_hx_wide": 1}])
def test_options_that_close_the_zero_phase_send_every_tie_home(diarizer, off):
    Xs = [duplicates(n, 3, 300 + n) for n in (40, 65, 129)] + rows((70,), 3, 1)
    with options(diarizer, linkage_wgs=2, linkage_square=1, **off):
        ref = [diarizer.linkage_ex(X, "centroid") for X in Xs]
    with forced(diarizer, 2, **off):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, "centroid")
        got = launches(diarizer, *NAMES)
    assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
    assert got == [1, 0, 0, 1, 0, 3]


def test_workspaces_that_cannot_be_allocated(weights):
    """six duplicate jobs of 300 rows under a 1 MB limit, in a context of its own: the group is halved down to single jobs as in test_linkage_xcd.py, every job
    then ties in a launch of its own and goes through a zero launch of one.  (The zero workspaces of jobs this small stay below the smallest limit the option
    can express; their own refusal takes the same path to the redo list as a refused launch.)"""
    d = sdhip.Diarizer(weights[0], weights[1])
    try:
        Xs = [duplicates(300, 8, 77 + j) for j in range(6)]
        with options(d, linkage_wgs=2, linkage_square=1):
            ref = [d.linkage_ex(X, "centroid") for X in Xs]
        try:
            with forced(d, 2):
                d.set_option("ws_limit_mb", 1)
                d.reset_stats()
                Z, st = d.linkage_many(Xs, "centroid")
                failed = d.kernel_stats("linkage_batch_alloc_failed")["launches"]
                got = launches(d, *NAMES)
        finally:
            d.set_option("ws_limit_mb", 0)
        assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
        assert failed == 5 and got == [6, 6, 6, 0, 6, 0]
    finally:
        d.close()


def test_the_key_takes_zero_and_one(diarizer):
    for bad in (2, -1):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.set_option("linkage_batch_xcd_zero", bad)
        assert e.value.code == ERR_ARG
    diarizer.set_option("linkage_batch_xcd_zero", 1)
    diarizer.set_option("linkage_batch_xcd_zero", 0)


def test_automatic_geometry_three_duplicate_jobs_beside_a_tie_free_one(diarizer):
    rng = np.random.default_rng(1600)
    Xs = []
    for n in (1500, 1600, 1700):
        X = rng.standard_normal((n, 16))
        src = rng.choice(n, n // 20, replace=False)
        X[(src + 1) % n] = X[src]                       # about 5 % of the rows are copies
        Xs.append(X)
    Xs.append(rng.standard_normal((1550, 16)))
    ref = [diarizer.linkage_ex(X, "centroid") for X in Xs]
    assert all((z[:, 2] == 0).sum() >= 50 for z in ref[:3]) and not (ref[3][:, 2] == 0).any()
    with options(diarizer, linkage_batch_xcd=1, linkage_batch_xcd_zero=1):
        diarizer.reset_stats()
        Z, st = diarizer.linkage_many(Xs, "centroid")
        got = launches(diarizer, *NAMES)
    assert not st.any() and all(same(z, r) for z, r in zip(Z, ref))
    assert got == [1, 1, 1, 1, 3, 0], dict(zip(NAMES, got))


def group_runs(d, call):
    """a group call: the sequential flow, then linkage_batch = 1 on the forced geometry with the key at 1 and at 0 -> bytes per job and the class counters"""
    res = {}
    for name, kw in (("seq", {}), (1, dict(linkage_batch=1, linkage_batch_xcd=1, linkage_batch_xcd_zero=1)), (0, dict(linkage_batch=1, linkage_batch_xcd=1))):
        with options(d, linkage_wgs=2, linkage_square=1, **kw):
            d.reset_stats()
            out = [job_bytes(d, j, g) if isinstance(g, list) else g for j, g in enumerate(call())]
            res[name] = (out, launches(d, "linkage_xcd_jobs", "linkage_xcd_zero_jobs", "linkage_xcd_redone", "linkage_rg_jobs"))
    return res


def test_group_calls_give_the_same_bytes(diarizer):
    recs = [synth.make_pcm(s + 1.0, seed=5300 + r)[:int(s * 16000) + 17 * r].copy() for r, s in enumerate((20.0, 33.0, 45.0, 60.0))]
    pcm = pcm75()
    streams = [diarizer.stream() for _ in range(3)]
    try:
        for rnd in range(2):
            diarizer.stream_push_many(streams, [pcm[96000 * i + rnd * 200000 + 13 * i * rnd:96000 * i + (rnd + 1) * 200000 + 31 * i] for i in range(3)])
        for call in (lambda: diarizer.diarize_many(recs), lambda: diarizer.stream_turns_many(streams)):
            res = group_runs(diarizer, call)
            assert res[1][0] == res["seq"][0] and res[0][0] == res["seq"][0] and all(isinstance(r, tuple) and len(r[0]) > 0 for r in res[1][0])
            assert res[1][1][3] > 0 and res["seq"][1] == [0, 0, 0, 0] and res[0][1][1] == 0
            assert sum(res[1][1][:3]) == sum(res[0][1][:3]) > 0          # done + zero + redone = the jobs of the class, with the key and without
    finally:
        for s in streams:
            s.close()
