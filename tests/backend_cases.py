"""Operands and expected buffers of tests/test_backend_kernels.py (GPU), built here so that tests/test_backend_ref.py can show on the CPU what each case
is for.  Nothing here touches the GPU.  Per family: NAMES (the cases), case(name) -> the operands (cached), expected(name, mistake=None) -> the WHOLE
buffers the hook returns, slack included, as the reference of tests/backend_ref.py gives them (`mistake`: one of backend_ref.MISTAKES planted in it).

Shapes are the smallest that reach the edge they aim at: 16-row unrolling of k_cluster_means (1, 15, 16, 17, 31, 32, 33, 100 members), the 1 024-score
LDS tile of k_assign / k_assign_cuts (K = 1 023, 1 024, 1 025, 2 049; cuts that straddle one edge and two), the 64-lane stride over cuts (65, 130 cuts),
128- and 256-thread blocks (127 .. 129 rows, 255 .. 257 elements, 65 chunks), the +-2 chunk bracket of the gather kernels (11 .. 13 and 40 chunks).
"""
import functools

import numpy as np

import backend_ref as R
from oracle import orc

SLACK = 256
FCANARY, ICANARY, BCANARY = -7776.0, -7776, 0xA5
F, S = R.FRAMES, R.SPEAKERS


def rng(*key):
    return np.random.default_rng([ord(ch) for ch in "backend"] + [int(k) for k in key])


def whole(a, slack_shape, canary):
    """the array, then the slack of the hook's buffer"""
    a = np.ascontiguousarray(a)
    return np.concatenate([a.reshape(-1), np.full(int(np.prod(slack_shape)), canary, a.dtype)])


# ---------------------------------------------------------------- binarize
BINARIZE = ("c1_all_on", "c2_edges", "c65")
BINARIZE_WANTS = (("bin", "masks", "nact"), ("masks",), ("bin", "nact"))      # finalize_front asks for bin + nact, shard_infer for masks alone


@functools.lru_cache(None)
def binarize_case(name):
    if name == "c1_all_on":                      # all three speakers on throughout: every clean mask is empty, the raw masks are used
        return np.full((1, F, S), 0.9, np.float32)
    if name == "c2_edges":
        seg = np.full((2, F, S), 0.1, np.float32)
        on = np.float32(0.9)
        # chunk 0: speaker 0 alone in 3 frames (clean sum exactly 3: the raw mask stays), speaker 1 alone in 4 (exactly 4: the clean mask is taken), both
        # also on together in frames 100 .. 119, which is what the two masks differ in; speaker 2 is never on
        seg[0, 10:13, 0] = on
        seg[0, 20:24, 1] = on
        seg[0, 100:120, :2] = on
        # chunk 1: NaN, +-inf, float32(ONSET) and its neighbours, beside a talker who is on throughout
        o = np.float32(R.ONSET)
        seg[1, :, 2] = on
        seg[1, 5:60:6, 0] = [np.nan, np.inf, -np.inf, o, np.nextafter(o, np.float32(1)), np.nextafter(o, np.float32(0)), np.nan, o, np.inf, 0.5]
        seg[1, 200:206, 1] = [np.nextafter(o, np.float32(1)), o, np.nan, np.inf, np.nextafter(o, np.float32(0)), 1.0]
        return seg
    g = rng(1)
    seg = g.random((65, F, S), dtype=np.float32)
    seg = (seg + np.roll(seg, 1, 1) + np.roll(seg, 2, 1)) / np.float32(3)      # runs of a few frames
    seg[7, :, 1] = 0.0                           # a column that is never on
    seg[9] = 0.95                                # all on
    seg[64, 3:290, :] = 0.2                      # the last chunk: three frames on at most
    seg[3, 50, 0] = np.nan
    return seg


def binarize_expected(name, mistake=None):
    b, masks, nact = R.binarize(binarize_case(name), mistake)
    return {"bin": whole(b, (SLACK, F, S), np.uint8(BCANARY)), "masks": whole(masks, (SLACK * S, F), np.float32(FCANARY)),
            "nact": whole(nact, (SLACK * S,), np.int32(ICANARY))}


# ---------------------------------------------------------------- count
COUNT = ("c1", "c2", "c9_zeros", "c10_ones", "c12", "c40", "c2_half_05", "c2_half_15", "c2_half_25", "c40_half")
_HALF = {"c2_half_05": ((1, 0, 0), (0, 0, 0)), "c2_half_15": ((1, 1, 0), (0, 0, 1)), "c2_half_25": ((1, 1, 1), (1, 0, 1))}


@functools.lru_cache(None)
def count_case(name):
    chunks = int(name.split("_")[0][1:])
    if name in _HALF:                            # two chunks cover a frame: sums 1, 3, 5 of 2 give exactly 0.5, 1.5, 2.5
        return np.broadcast_to(np.array(_HALF[name], np.uint8)[:, None, :], (2, F, S)).copy()
    if name == "c40_half":                       # eight chunks cover a frame, four of them even: 4 / 8, and 12 / 8 in the second half
        b = np.zeros((40, F, S), np.uint8)
        b[0::2, :, 0] = 1
        b[20:, :, 1] = 1
        return b
    if name.endswith("zeros"):
        return np.zeros((chunks, F, S), np.uint8)
    if name.endswith("ones"):
        return np.ones((chunks, F, S), np.uint8)
    return (rng(2, chunks).random((chunks, F, S)) < 0.5).astype(np.uint8)


def count_expected(name, mistake=None):
    cnt, avg = R.count(count_case(name), mistake)
    return whole(cnt, (SLACK,), np.int32(ICANARY)), whole(avg, (SLACK,), np.float64(FCANARY))


# ---------------------------------------------------------------- gather_normalize
GATHER = tuple("N%d_d%d" % (N, d) for N in (1, 127, 128, 129) for d in (1, 3, 192))
GATHER_ROWS = 140


@functools.lru_cache(None)
def gather_case(name):
    """-> X [140][d], tidx [N] descending with a repeat, want_xout.  Rows 130 .. 136: zeros; 1e-30 (a float32 norm that is still a number); 1e30 (the same);
    1e-50 (the float32 norm underflows to 0: the row is copied, where a float64 norm would divide); 1e39 (the float32 norm is inf: a row of zeros);
    2.5e38 (a norm that float32 holds for d = 1 and rounds to inf for d > 1); a row of NaN"""
    N, d = (int(p[1:]) for p in name.split("_"))
    g = rng(3, N, d)
    X = g.standard_normal((GATHER_ROWS, d)) * 10.0 ** g.uniform(-3, 3, (GATHER_ROWS, 1))
    X[130], X[131], X[132], X[133], X[134] = 0.0, 1e-30, 1e30, 1e-50, 1e39
    X[135] = 2.5e38
    X[136] = np.nan
    tidx = (GATHER_ROWS - 1 - np.arange(N)).astype(np.int32)
    if N > 3:
        tidx[3] = tidx[2]
        tidx[-1] = tidx[0]
    if N == 1:
        tidx[0] = 133
    return X, tidx, N != 128                     # N = 128: Xout null, as linkage_rows launches it


def gather_expected(name, mistake=None):
    X, tidx, want = gather_case(name)
    xo, xn = R.gather_normalize(X, tidx, mistake)
    d = X.shape[1]
    return (whole(xo, (SLACK, d), np.float64(FCANARY)) if want else None), whole(xn, (SLACK, d), np.float64(FCANARY))


# ---------------------------------------------------------------- cluster_means
MEANS = tuple("d%d" % d for d in (1, 63, 64, 65, 192, 1025))
MEANS_SIZES = (1, 15, 16, 17, 31, 32, 33, 100)


@functools.lru_cache(None)
def means_case(name):
    """-> X [260][d] of magnitudes 1e-8 .. 1e8, order, off: eight clusters whose members interleave (ascending inside a cluster, as group_by_label leaves them)"""
    d = int(name[1:])
    g = rng(4, d)
    rows = sum(MEANS_SIZES) + 15
    X = g.standard_normal((rows, d)) * 10.0 ** g.uniform(-8, 8, (rows, d))
    lab = np.repeat(np.arange(len(MEANS_SIZES) + 1), MEANS_SIZES + (15,))      # label 8: rows of no cluster
    g.shuffle(lab)
    order = np.concatenate([np.flatnonzero(lab == k) for k in range(len(MEANS_SIZES))]).astype(np.int32)
    return X, order, np.concatenate([[0], np.cumsum(MEANS_SIZES)]).astype(np.int32)


def means_expected(name, mistake=None):
    X, order, off = means_case(name)
    return whole(R.cluster_means(X, order, off, mistake), (SLACK, X.shape[1]), np.float64(FCANARY))


# ---------------------------------------------------------------- assign
ASSIGN = ("M1_d4_K1", "M7_d4_K2_neg", "M7_d4_K1023", "M7_d4_K1024", "M7_d4_K1025", "M7_d4_K2049", "M7_d1_K5", "M7_d192_K5", "M7_d192_K5_zero", "M7_d4_K1025_zero")


def _negative_pair(g, d):
    """e and two centroids opposite to it whose scores 2 - (1 - cos) both round BELOW zero: cos comes out two units in the last place beyond -1"""
    scales = np.linspace(0.3, 9.7, 48)
    for _ in range(5000):
        e = g.standard_normal(d)
        cen = -scales[:, None] * e
        neg = np.flatnonzero(R.soft_scores(e[None], cen)[0][0] < 0)
        if len(neg) >= 2:
            return e, cen[neg[:2]]
    raise AssertionError("no vector with two negative scores found")


@functools.lru_cache(None)
def assign_case(name):
    """-> E [M][d], cen [K][d].  Duplicate centroids (3, 5) inside a tile and (3, 1030) / (3, K - 1) across the tile edge; row 0 = 2.5 x centroid 3 (the
    duplicates are its maximum), row 1 = 0.5 x the last centroid, row 2 NaN; `zero`: row 3 and centroid 1 are zeros; `neg`: every score of row 0 negative"""
    p = name.split("_")
    M, d, K = int(p[0][1:]), int(p[1][1:]), int(p[2][1:])
    g = rng(5, M, d, K)
    E, cen = g.standard_normal((M, d)), g.standard_normal((K, d))
    if "neg" in p:
        E[0], cen = _negative_pair(g, d)
        return E, cen
    if K >= 6:
        cen[5] = cen[3]
    if K >= 1031:
        cen[1030] = cen[3]
    elif K >= 1023:
        cen[K - 1] = cen[3]
    if K >= 4:
        E[0] = 2.5 * cen[3]
    if M > 2:
        E[1] = 0.5 * cen[K - 1]
        E[2] = np.nan
    if "zero" in p:
        E[3] = 0.0
        cen[1] = 0.0
    return E, cen


def assign_expected(name, mistake=None):
    E, cen = assign_case(name)
    hard, err, soft, best = R.assign(E, cen, mistake)
    return {"hard": whole(hard, (SLACK,), np.int32(ICANARY)), "err": whole(np.array([err], np.int32), (SLACK,), np.int32(ICANARY)),
            "soft": whole(soft, (SLACK, cen.shape[0]), np.float64(FCANARY)), "best": whole(best, (SLACK,), np.float64(FCANARY))}


# ---------------------------------------------------------------- constrained_argmax
CONSTRAINED = tuple("K%d_c%d" % (K, c) for K in (1, 2, 3, 4, 64) for c in (1, 63, 64, 65))


@functools.lru_cache(None)
def constrained_case(name):
    """-> soft [chunks][3][K]: by (chunk + K) % 7: one, two, three NaN rows; constant rows; rows equal to each other on a coarse grid (exact ties); a NaN
    row beside two equal rows; plain scores"""
    K, chunks = (int(p[1:]) for p in name.split("_"))
    g = rng(6, K, chunks)
    soft = g.uniform(0.0, 2.0, (chunks, S, K))
    for c in range(chunks):
        kind = (c + K) % 7
        if kind in (1, 2, 3):
            soft[c, g.permutation(S)[:kind]] = np.nan
        elif kind == 4:
            soft[c] = g.uniform(0, 2, (S, 1))
        elif kind == 5:
            soft[c] = np.round(g.uniform(0, 2, (1, K)) * 4) / 4
        elif kind == 6:
            soft[c, 1:] = np.round(g.uniform(0, 2, (1, K)) * 2) / 2
            soft[c, 0] = np.nan
    return soft


def constrained_expected(name):
    return whole(R.constrained_argmax(constrained_case(name)), (SLACK, S), np.int32(ICANARY))


# ---------------------------------------------------------------- activations
ACTIVATIONS = tuple("c%d_K%d" % (c, K) for c in (1, 2, 11, 12, 13, 40) for K in (1, 3, 7))


@functools.lru_cache(None)
def activations_case(name):
    """-> seg [chunks][293][3] with -inf and NaN scores, hard [chunks][3] by chunk % 4: plain; a -2; the same cluster twice; all three the same.  Cluster
    K - 1 (K > 1) belongs to nobody"""
    chunks, K = (int(p[1:]) for p in name.split("_"))
    g = rng(7, chunks, K)
    seg = g.random((chunks, F, S), dtype=np.float32)
    seg[g.random((chunks, F, S)) < 0.01] = -np.inf
    seg[g.random((chunks, F, S)) < 0.01] = np.nan
    top = max(K - 1, 1)
    hard = g.integers(0, top, (chunks, S)).astype(np.int32)
    for c in range(chunks):
        if c % 4 == 1:
            hard[c, g.integers(0, S)] = -2
        elif c % 4 == 2:
            hard[c, 1] = hard[c, 0]
        elif c % 4 == 3:
            hard[c] = hard[c, 2]
    return seg, hard, K


def activations_expected(name, mistake=None):
    seg, hard, K = activations_case(name)
    return whole(R.activations(seg, hard, K, mistake), (SLACK, K), np.float64(FCANARY))


# ---------------------------------------------------------------- topk
TOPK = ("K1", "K3", "K7", "K3_origin")


@functools.lru_cache(None)
def topk_case(name):
    """-> act [310][K], count [300], ar0, cr0, rows (more than one 256-thread block), crow < rows.  Counts cycle through 0, 1, K, K + 2; rows by i % 5:
    all equal; pairs of equal values; +0.0 against -0.0; two plain"""
    K = int(name.split("_")[0][1:])
    g = rng(8, K)
    act = g.uniform(-1, 3, (310, K))
    for i in range(310):
        if i % 5 == 0:
            act[i] = act[i, 0]
        elif i % 5 == 1:
            act[i, 1::2] = act[i, 0:K - 1:2]
        elif i % 5 == 2:
            act[i] = np.where(g.random(K) < 0.5, 0.0, -0.0)
    count = np.array([(0, 1, K, K + 2)[(i // 3) % 4] for i in range(300)], np.int32)
    if name.endswith("origin"):
        return act, count, 0, 0, 300, 300
    return act, count, 3, 2, 290, 281


def topk_expected(name, mistake=None):
    act, count, ar0, cr0, rows, crow = topk_case(name)
    out = R.topk(act, count, ar0, cr0, rows, crow, mistake, slack=SLACK)
    out[rows:][out[rows:] == 0] = BCANARY       # (a mistake that writes behind the last row leaves ones there)
    return out.reshape(-1)


# ---------------------------------------------------------------- assign_cuts
CUTS = ("T1", "T2", "T65", "T130", "table_1023", "table_1024", "table_1025", "straddle", "two_edges")
CUTS_D = 4


def _rows_at(cen, E, at):
    """row i of E = a multiple of centroid at[i]: its maximum (cosine 1)"""
    for i, j in enumerate(at):
        E[i] = (1.5 + i) * cen[j]


@functools.lru_cache(None)
def cuts_case(name):
    """-> E [M][4], cen [total][4], coff, slot (a permutation into n_slots = Tn + 2 rows), n_slots, nact (zeros among it)"""
    g = rng(9, CUTS.index(name))
    M = 7
    if name[0] == "T":
        Tn = int(name[1:])
        sizes = g.integers(1, 10, Tn)
        sizes[::5] = 1
    elif name.startswith("table"):
        sizes = np.array([1000, int(name.split("_")[1]) - 1000])
    elif name == "straddle":
        sizes = np.array([990, 70, 40])          # cut 1 = rows [990, 1060): 34 in front of the edge, 36 behind it
    else:
        sizes = np.array([3, 2100, 5])           # cut 1 = rows [3, 2103): the edges 1 024 and 2 048 lie inside it
    coff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    Tn, total = len(sizes), int(coff[-1])
    cen, E = g.standard_normal((total, CUTS_D)), g.standard_normal((M, CUTS_D))
    if name == "table_1025":
        cen[1024] = cen[1010]                    # tied across the edge: the maximum of row 0; row 1: the last row in front of the edge
        _rows_at(cen, E, [1010, 1023])
    elif name == "table_1024":
        cen[1023] = cen[1001]
        _rows_at(cen, E, [1001])
    elif name == "straddle":
        cen[1040] = cen[1000]                    # rows: maximum before the edge, behind it, tied across it, in the last row of the cut
        cen[1059] = 3.0 * cen[1059]
        _rows_at(cen, E, [1010, 1030, 1000, 1059])
    elif name == "two_edges":
        cen[2050] = cen[500]
        cen[1500] = cen[40]
        _rows_at(cen, E, [10, 1100, 2100, 500, 40])
    E[M - 1] = np.nan
    n_slots = Tn + 2
    slot = g.permutation(n_slots)[:Tn].astype(np.int32)
    nact = g.integers(1, 4, M).astype(np.int32)
    nact[5] = 0                                  # an inactive row: -2 in every cut, its best score stays
    return E, cen, coff, slot, n_slots, nact


def cuts_expected(name, mistake=None):
    E, cen, coff, slot, n_slots, nact = cuts_case(name)
    m2, hard, best, err = R.assign_cuts(E, cen, coff, slot, n_slots, nact, mistake)
    M = E.shape[0]
    hard = np.concatenate([np.full(M, ICANARY, np.int32) if h is None else h for h in hard])      # a slot no cut writes keeps the canary
    return {"m2": whole(m2, (SLACK,), np.float64(FCANARY)), "hard": whole(hard, (SLACK,), np.int32(ICANARY)),
            "best": whole(best, (SLACK,), np.float64(FCANARY)), "err": whole(np.array([err], np.int32), (SLACK,), np.int32(ICANARY))}


# ---------------------------------------------------------------- recon_cuts
RECON = ("T1", "T3", "T65", "T3_planted")
RECON_CHUNKS = 12


@functools.lru_cache(None)
def recon_case(name):
    """-> seg [12][293][3], hard [Tg][36] (-2 among it), koff (K_t = 1 .. 7), count, ar0, cr0, rows, crow, act_in (planted: tables of ties for k_topk_cuts)"""
    Tg = int(name.split("_")[0][1:])
    g = rng(10, RECON.index(name))
    chunks = RECON_CHUNKS
    nact, _ = R.activation_frames(chunks)
    seg = g.random((chunks, F, S), dtype=np.float32)
    Ks = (np.arange(Tg) * 3) % 7 + 1
    koff = np.concatenate([[0], np.cumsum(Ks)]).astype(np.int32)
    hard = np.stack([g.integers(0, K, chunks * S) for K in Ks]).astype(np.int32)
    hard[g.random(hard.shape) < 0.1] = -2
    rows, crow, ar0, cr0 = nact - 40, nact - 47, 5, 3
    count = g.integers(0, 6, crow + cr0 + 2).astype(np.int32)
    act_in = None
    if name.endswith("planted"):
        act_in = np.round(g.uniform(0, 2, nact * int(koff[-1])) * 2) / 2
    return seg, hard, koff, count, ar0, cr0, rows, crow, act_in


def recon_expected(name, mistake=None):
    seg, hard, koff, count, ar0, cr0, rows, crow, act_in = recon_case(name)
    act, binary = R.recon_cuts(seg, hard, koff, count, ar0, cr0, rows, crow, act_in, mistake)
    return whole(act, (SLACK,), np.float64(FCANARY)), whole(binary, (SLACK,), np.uint8(BCANARY))


# ---------------------------------------------------------------- casts
CAST_N = (1, 255, 256, 257)


@functools.lru_cache(None)
def cast_case(n):
    """-> pcm int16 [n], a float32 [n], hard int32 [n], nact int32 [n]"""
    g = rng(11, n)
    pcm = g.integers(-32768, 32768, n).astype(np.int16)
    a = g.standard_normal(n).astype(np.float32)
    edge_p, edge_a = [-32768, -1, 0, 32767], [np.nan, np.inf, -0.0, 1e-45, 3.4028235e38, -np.inf]
    if n == 1:
        pcm[0], a[0] = -32768, np.float32(1e-45)
    else:
        pcm[:4], pcm[-1] = edge_p, 32767
        a[:6] = edge_a
    nact = g.integers(0, 3, n).astype(np.int32)
    nact[-1] = 0
    return pcm, a, g.integers(0, 9, n).astype(np.int32), nact


def cast_expected(n, mistake=None):
    pcm, a, hard, nact = cast_case(n)
    return (whole(R.pcm_to_f32(pcm), (SLACK,), np.float32(FCANARY)), whole(R.f32_to_f64(a), (SLACK,), np.float64(FCANARY)),
            whole(R.mark_inactive(hard, nact, mistake), (SLACK,), np.int32(ICANARY)))


# ---------------------------------------------------------------- sd_clustering at d = 1025 (k_cluster_means beyond one block of threads)
@functools.lru_cache(None)
def wide_clustering_case(d=1025):
    """-> emb [20][3][d] float64: three talkers of 18 rows each (above the minimum cluster size of 15), two stray rows, four NaN rows"""
    g = rng(12, d)
    centres = g.standard_normal((3, d))
    rows = np.concatenate([centres[k] + 0.05 * g.standard_normal((18, d)) for k in range(3)] + [g.standard_normal((2, d))])
    g.shuffle(rows)
    emb = np.full((60, d), np.nan)
    emb[np.sort(g.permutation(60)[:56])] = rows
    return emb.reshape(20, 3, d)


# which families can show a mistake: (names, expected) pairs that tests/test_backend_ref.py walks through
FAMILIES = {
    "binarize": (BINARIZE, binarize_expected), "count": (COUNT, count_expected), "gather": (GATHER, gather_expected), "means": (MEANS, means_expected),
    "assign": (ASSIGN, assign_expected), "activations": (ACTIVATIONS, activations_expected), "topk": (TOPK, topk_expected), "cuts": (CUTS, cuts_expected),
    "recon": (RECON, recon_expected), "casts": (CAST_N, cast_expected),
}
SHOWN_BY = {
    "pairwise_sum": ("means", "gather", "assign"), "f64_norm": ("gather",), "ge_argmax": ("assign", "cuts"), "last_max_across_tiles": ("assign",),
    "cln_ge_3": ("binarize",), "round_half_away": ("count",), "bracket_0": ("activations", "recon"), "unstable_topk": ("topk", "recon"),
    "count_unclamped": ("topk",), "carry_dropped": ("cuts",), "slot_ignored": ("cuts",), "inactive_skipped": ("cuts", "casts"),
}
