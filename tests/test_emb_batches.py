"""The embedding stage's batch planner (ecapa.hip: ecapa_plan_batches behind sd_test_emb_batches) against a transcription of the two loops it
replaced: the greedy loop sd_ecapa and sd_embed_signals each carried, and run_embed's loop with the tile-round search.  The transcription below
was written from those loops as they stood before the planner existed, line by line; it shares nothing with the C++ function.  Host arithmetic
only: no GPU, except the last test, which counts the launches of a real sd_ecapa call."""
import ctypes as C

import numpy as np
import pytest

import sdhip

T, ROWTAB_MAX_ITEMS = 501, 4095
EC_MARGIN = (65, 49, 28, 0)


# ---- the parent's code, transcribed
def space_offsets(nvalid, skip_dead_rows):
    """ecapa_row_plan / ec_space_rows: prefix sums [n + 1] of the rows per item in each of the four row spaces"""
    off = []
    for m in EC_MARGIN:
        rows = np.clip(np.asarray(nvalid, np.int64) + m, 1, T) if skip_dead_rows else np.full(len(nvalid), T, np.int64)
        off.append([0] + [int(v) for v in np.cumsum(rows)])
    return off


def round_items(nb):
    nb = (nb // 96) * 96
    return 96 if nb < 96 else nb


def greedy_loop(off, n, cap_rows):
    """the loop of sd_ecapa and sd_embed_signals"""
    rowoff, ends, a0 = off[0], [], 0
    while a0 < n:
        a1 = a0
        while a1 < n and a1 - a0 < ROWTAB_MAX_ITEMS and rowoff[a1 + 1] - rowoff[a0] <= cap_rows:
            a1 += 1
        if a1 == a0:
            a1 = a0 + 1
        ends.append(a1)
        a0 = a1
    return ends


LAYERS = ((0, 400), (0, 1024), (1, 1024), (1, 1024), (2, 1024), (2, 1024), (3, 1024), (3, 3 * 3072), (3, 2 * 128))


def batch_efficiency(off, a0, a1):
    ideal = actual = 0.0
    for sp, w in LAYERS:
        M = off[sp][a1] - off[sp][a0]
        ideal += float(w) * float(M) / 16384.0
        actual += float(w) * float((M + 16383) // 16384)
    return ideal / actual if actual > 0.0 else 0.0


def balanced_loop(off, n, cap_rows, balance):
    """run_embed's loop; `balance` stands where the loop read the context's skip_dead_rows"""
    rowoff = off[0]
    rows_all = rowoff[n]
    n_batches = (rows_all + cap_rows - 1) // cap_rows
    ends, a0, k = [], 0, 1
    while a0 < n:
        a_max = a0
        while a_max < n and a_max - a0 < ROWTAB_MAX_ITEMS and rowoff[a_max + 1] - rowoff[a0] <= cap_rows:
            a_max += 1
        if a_max == a0:
            a_max = a0 + 1
        a1 = a_max
        if a_max < n and balance:
            left_batches = n_batches - k + 1 if n_batches - k + 1 > 1 else 1
            aim_rows = rowoff[a0] + (rows_all - rowoff[a0] + left_batches - 1) // left_batches
            aim = a0 + 1
            while aim < a_max and rowoff[aim + 1] <= aim_rows:
                aim += 1
            aim = aim + 80 if aim + 80 < a_max else a_max
            best, cand = -1.0, aim
            while cand > a0 and cand + 160 > aim:
                e = batch_efficiency(off, a0, cand)
                if e > best:
                    best, a1 = e, cand
                cand -= 1
        ends.append(a1)
        a0 = a1
        k += 1
    return ends


# ---- inputs
MIXES = ("uniform", "all_full", "all_one", "planted_hour")


def make_nvalid(mix, n, seed):
    rng = np.random.default_rng(seed)
    if mix == "uniform":
        return rng.integers(1, T + 1, n).astype(np.int32)
    if mix == "all_full":
        return np.full(n, T, np.int32)
    if mix == "all_one":
        return np.ones(n, np.int32)
    nv = rng.integers(1, T + 1, n).astype(np.int32)          # planted-hour-like: 60 % of the items at full length
    nv[rng.random(n) < 0.6] = T
    return nv


@pytest.mark.parametrize("n", [1, 95, 96, 97, 700, 13000])
@pytest.mark.parametrize("mix", MIXES)
def test_planner_equals_the_loops_it_replaced(mix, n):
    nvalid = make_nvalid(mix, n, 1000 * MIXES.index(mix) + n)
    for skip in (0, 1):
        off = space_offsets(nvalid, skip)
        item_rows = np.diff(off[0])
        for batch_items in (96, 768, 3072):
            cap_rows = round_items(batch_items) * T
            for balance in (0, 1):
                case = (mix, n, skip, batch_items, balance)
                ends = sdhip.emb_batches(nvalid, batch_items, skip, balance)
                want = balanced_loop(off, n, cap_rows, balance)
                if not balance:
                    assert want == greedy_loop(off, n, cap_rows), case          # the parent's two loops agree where neither balances
                assert ends == want, case
                starts = [0] + ends[:-1]
                assert ends[-1] == n and all(b > a for a, b in zip(starts, ends)), case
                for a, b in zip(starts, ends):
                    assert b - a <= ROWTAB_MAX_ITEMS, case
                    assert off[0][b] - off[0][a] <= cap_rows or b - a == 1, case
                    if not balance and b < n:
                        assert b - a == ROWTAB_MAX_ITEMS or off[0][b] - off[0][a] + item_rows[b] > cap_rows, case
                if mix == "all_one" and n == 13000 and skip and batch_items == 3072 and not balance:
                    # 66 rows per item: 4 095 items are 270 270 rows, far below the 3 072 x 501 budget -- the item limit binds
                    assert item_rows.max() == 66 and ROWTAB_MAX_ITEMS in [b - a for a, b in zip(starts, ends)], case


def test_batch_items_are_rounded_as_the_stage_rounds_them():
    nvalid = make_nvalid("planted_hour", 700, 5)
    for skip in (0, 1):
        for balance in (0, 1):
            at96 = sdhip.emb_batches(nvalid, 96, skip, balance)
            assert len(at96) >= 2
            assert sdhip.emb_batches(nvalid, 100, skip, balance) == at96
            assert sdhip.emb_batches(nvalid, 50, skip, balance) == at96
            assert sdhip.emb_batches(nvalid, 192, skip, balance) != at96


def test_bad_arguments_are_refused():
    f = sdhip.lib().sd_test_emb_batches
    nv = np.full(300, T, np.int32)
    out = np.zeros(300, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert f(p(nv), 300, 96, 1, 0, p(out), 300) == 4 and list(out[:4]) == [96, 192, 288, 300]
    assert f(p(nv), -1, 96, 1, 0, p(out), 300) == -1              # -SD_ERR_ARG
    assert f(None, 300, 96, 1, 0, p(out), 300) == -1
    assert f(p(nv), 300, 96, 1, 0, None, 300) == -1
    assert f(p(nv), 300, 96, 1, 0, p(out), 3) == -1               # four batches do not fit three slots
    assert f(p(nv), 300, 96, 1, 0, p(out), -1) == -1
    assert f(None, 0, 96, 1, 0, None, 0) == 0                     # no items: no batches, nothing read or written
    with pytest.raises(sdhip.SdError):
        sdhip.emb_batches(np.full(1_100_000, T, np.int32), 96, 0, 0)      # more rows than the stage's int offsets may hold


@pytest.mark.gpu
def test_sd_ecapa_launches_the_planned_batches_and_the_bits_do_not_move(weights):
    """230 items whose lengths are spread over 1 .. 501 frames (every fifth at full length) cross the 96 x 501-row budget: sd_ecapa at
    emb_batch_items = 96 runs the network once per planned batch (block0 is launched once per run_ecapa call) and gives the bits of the
    single batch at 3072.  A context of its own: the explicit batch option and the profile level do not leak into the session's."""
    rng = np.random.default_rng(230)
    n = 230
    frames = rng.integers(1, T + 1, n)
    frames[::5] = T
    lens = (frames / float(T)).astype(np.float32)
    nvalid = np.clip(np.ceil(lens * np.float32(T)), 1, T).astype(np.int32)          # sd_ecapa's own float32 rule
    assert nvalid.min() < 50 and nvalid.max() == T
    feats = rng.standard_normal((n, T, 80)).astype(np.float32)
    d = sdhip.Diarizer(weights[0], weights[1])
    try:
        d.set_option("profile", 2)
        emb, launches = {}, {}
        for batch_items in (96, 3072):
            d.set_option("emb_batch_items", batch_items)
            before = d.kernel_stats("conv_gemm:block0")["launches"]
            emb[batch_items] = d.ecapa(feats, lens)
            launches[batch_items] = d.kernel_stats("conv_gemm:block0")["launches"] - before
            assert launches[batch_items] == len(sdhip.emb_batches(nvalid, batch_items, True, False)), batch_items
        assert launches[3072] == 1 and launches[96] >= 2, launches
        assert np.isfinite(emb[96]).all() and np.array_equal(emb[96], emb[3072])
    finally:
        d.set_option("emb_batch_items", 3072)
        d.set_option("profile", 0)
        d.close()
