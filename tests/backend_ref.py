"""Plain numpy float64 references of the kernels behind the two networks (csrc/postseg.hip, cluster.hip, reconstruct.hip, cut.hip, the casts of
pipeline.cpp), one function per kernel, for tests/test_backend_kernels.py (GPU) and tests/test_backend_ref.py (CPU).  Each restates sd.cpp /
Clustering.py at the lines the kernel's header cites; where the oracle (oracle/orc.py) has a function at this level it is called, and the restatement
beside it is pinned to it on the CPU.

Every sum is SEQUENTIAL in the element index (seq_sum: a cumsum, never np.sum or @), products are rounded before they are added (numpy does not
contract), the norm of gather_normalize is rounded through np.float32: the results are the kernels' bytes, and the tests compare bytes.

`mistake` (default None) plants ONE of MISTAKES in a function: tests/test_backend_ref.py shows that each of them changes a byte of a case of
tests/backend_cases.py.
"""
import numpy as np

from oracle import orc

FRAMES, SPEAKERS = 293, 3
ONSET = 0.4442333667381752                       # sd.cpp:1339
NL = int(np.floor(FRAMES * 0.1))                 # frames trimmed on each side of a chunk for the count (sd.cpp:1755)
FT = FRAMES - 2 * NL
TILE = 1024                                      # ASSIGN_TILE / CUT_TILE: the LDS tile of k_assign / k_assign_cuts
DBL_MAX = np.finfo(np.float64).max

MISTAKES = ("pairwise_sum", "f64_norm", "ge_argmax", "last_max_across_tiles", "cln_ge_3", "round_half_away", "bracket_0", "unstable_topk",
            "count_unclamped", "carry_dropped", "slot_ignored", "inactive_skipped")


# ---------------------------------------------------------------- sums
def pairwise_sum(x, axis):
    x = np.moveaxis(np.asarray(x, np.float64), axis, 0)
    while x.shape[0] > 1:
        if x.shape[0] & 1:
            x = np.concatenate([x, np.zeros_like(x[:1])])
        x = x[0::2] + x[1::2]
    return x[0] if x.shape[0] else np.zeros(x.shape[1:])


def seq_sum(x, axis, mistake=None):
    """x[0] + x[1] + ... in index order, starting from 0.0 as the kernels do"""
    x = np.asarray(x, np.float64)
    if mistake == "pairwise_sum":
        return pairwise_sum(x, axis)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis))
    return np.take(np.cumsum(x, axis=axis), -1, axis=axis)


# ---------------------------------------------------------------- postseg.hip
def binarize_bits(seg):
    """k_binarize_masks' first loop = SegmentModel::binarize (sd.cpp:1506-1639): orc.binarize -> uint8 [chunks][293][3]"""
    return orc.binarize(np.ascontiguousarray(seg, np.float32)).astype(np.uint8)


def select_masks(b, mistake=None):
    """cleanSegmentations + the mask choice (sd.cpp:710-743, 3047-3078): the clean mask where its sum is > 3 frames -> float32 [chunks * 3][293]"""
    b = np.asarray(b, np.int64)
    keep = b.sum(-1, keepdims=True) < 2                                      # sd.cpp:730
    clean = b * keep
    cln = clean.sum(1, keepdims=True)
    use = cln >= 3 if mistake == "cln_ge_3" else cln > 3                      # sd.cpp:3017: min_num_frames = 3
    return np.ascontiguousarray(np.where(use, clean, b).transpose(0, 2, 1).reshape(-1, FRAMES), np.float32)


def binarize(seg, mistake=None):
    """-> bin uint8 [chunks][293][3], masks float32 [chunks * 3][293], nact int32 [chunks * 3]"""
    b = binarize_bits(seg)
    masks = orc.select_masks(b.astype(np.float64)) if mistake is None else select_masks(b, mistake)
    return b, masks, b.sum(1).reshape(-1).astype(np.int32)


def np_rint(v, mistake=None):
    if mistake == "round_half_away":
        return int(np.floor(abs(v) + 0.5) * np.sign(v))
    return orc.np_rint(v)


def count_frames(chunks):
    return orc.closest_frame(0.5 + 4.0 + (chunks - 1) * 0.5, start=0.5) + 1       # sd.cpp:1232, trim() 1776-1778


def count(b, mistake=None):
    """speaker_count (sd.cpp:1665-1782): every frame over ALL chunks, ascending -> count int32 [frames], avg float64 [frames] (the value in front of np_rint)"""
    b = np.asarray(b, np.int64)
    chunks = b.shape[0]
    nf = count_frames(chunks)
    tot, cnt = np.zeros(nf), np.zeros(nf)
    for c in range(chunks):
        s0 = orc.closest_frame(0.5 + 0.5 * c, start=0.5)                        # sd.cpp:1248-1253
        n = min(FT, nf - s0)
        tot[s0:s0 + n] += b[c, NL:NL + n].sum(-1).astype(np.float64)           # integers: exact in any order
        cnt[s0:s0 + n] += 1.0
    avg = np.where(cnt == 0, 0.0, tot / np.maximum(cnt, np.finfo(np.float64).eps))      # sd.cpp:1288, 1302-1305
    return np.array([np_rint(v, mistake) for v in avg], np.int32), avg


# ---------------------------------------------------------------- cluster.hip
def gather_normalize(X, tidx, mistake=None):
    """-> xout [N][d] = X[tidx], xn [N][d] = row / (double)(float)sqrt(sum x^2), the row itself where that norm is 0 (Helper::L2Norm returns float, sd.cpp:332-340)"""
    r = np.asarray(X, np.float64)[np.asarray(tidx)]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(seq_sum(r * r, 1, mistake))
        if mistake != "f64_norm":
            nrm = nrm.astype(np.float32).astype(np.float64)
        xn = np.where(nrm[:, None] != 0.0, r / nrm[:, None], r)
    return r.copy(), xn


def cluster_means(X, order, off, mistake=None):
    """cen[k] = (sum of X[order[off[k] : off[k + 1]]] in member order) / members (sd.cpp:442-473, 2149-2167)"""
    X = np.asarray(X, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([seq_sum(X[order[off[k]:off[k + 1]]], 0, mistake) / np.float64(off[k + 1] - off[k]) for k in range(len(off) - 1)])


def soft_scores(E, cen, mistake=None):
    """2 - cosine distance, the three sums sequential over d (sd.cpp:476-498; cosine_rule.h); NaN and err where a magnitude is 0 -> soft [M][K], err"""
    E, cen = np.asarray(E, np.float64), np.asarray(cen, np.float64)
    with np.errstate(all="ignore"):
        dot = seq_sum(E[:, None, :] * cen[None, :, :], 2, mistake)
        m1 = seq_sum(E * E, 1, mistake)[:, None] + np.zeros_like(dot)
        m2 = seq_sum(cen * cen, 1, mistake)[None, :] + np.zeros_like(dot)
        soft = 2.0 - (1.0 - dot / (np.sqrt(m1) * np.sqrt(m2)))
    zero = (m1 == 0.0) | (m2 == 0.0)
    soft[zero] = np.nan
    return soft, int(zero.any())


def first_max(row, mistake=None, edges=()):
    """Helper::argmax (sd.cpp:293-316): strict >, the first maximum wins; nothing compares greater (a NaN row): index 0 with the first score.
    `edges`: the indices at which a new LDS tile begins ("carry_dropped" starts afresh there) -> (index, score)"""
    best, mv, sb = 0, -DBL_MAX, row[0]
    for k, v in enumerate(row):
        if mistake == "carry_dropped" and k in edges:
            best, mv, sb = 0, -DBL_MAX, v
        if v > mv or (mistake == "ge_argmax" and v == mv):
            best, mv, sb = k, v, v
    return best, sb


def assign(E, cen, mistake=None):
    """k_assign -> hard int32 [M], err, soft [M][K], best [M]"""
    soft, err = soft_scores(E, cen, mistake)
    K = soft.shape[1]
    if mistake == "last_max_across_tiles":          # the running maximum of a tile replaces an equal one of the tiles before
        res = []
        for row in soft:
            best, mv, sb = 0, -DBL_MAX, row[0]
            for k0 in range(0, K, TILE):
                tb, tv = first_max(row[k0:k0 + TILE])
                if tv > mv or (tv == mv and k0 > 0):
                    best, mv, sb = k0 + tb, tv, tv
            res.append((best, sb))
    else:
        res = [first_max(row, mistake) for row in soft]
    return np.array([r[0] for r in res], np.int32), err, soft, np.array([r[1] for r in res], np.float64)


def nan_fill(soft):
    """Clustering.py:83: NaN scores become the smallest score of the whole table (0 when there is none)"""
    ok = soft[~np.isnan(soft)]
    return float(ok.min()) if ok.size else 0.0


def constrained_argmax(soft):
    """Clustering.py:81-94 through scipy's rectangular LSAP: orc.constrained_argmax, which tests/test_next_rows.py pins to scipy -> int32 [chunks][3]"""
    return orc.constrained_argmax(np.ascontiguousarray(soft, np.float64))


def mark_inactive(hard, nact, mistake=None):
    """sd.cpp:3172-3191: a local speaker without an active frame gets -2"""
    hard = np.array(hard, np.int32)
    if mistake != "inactive_skipped":
        hard[np.asarray(nact) == 0] = -2
    return hard


# ---------------------------------------------------------------- reconstruct.hip
def activation_frames(chunks):
    """-> frames, first frame of every chunk (sd.cpp:1233, 1248-1253 on the window (0.0, step, dur))"""
    return orc.closest_frame(5.0 + (chunks - 1) * 0.5) + 1, [orc.closest_frame(0.5 * c) for c in range(chunks)]


def activations(seg, hard, K, mistake=None):
    """act[f][k] = sum over ALL chunks c, ascending, that cover frame f of max_{s: hard[c][s] == k} seg[c][f - sfr[c]][s], std::max semantics (a NaN never
    replaces the running maximum, which starts at -inf: sd.cpp:2779); no such speaker: nothing is added (sd.cpp:2651) -> float64 [frames][K]"""
    seg, hard = np.asarray(seg, np.float32), np.asarray(hard)
    chunks = seg.shape[0]
    nact, sfr = activation_frames(chunks)
    act = np.zeros((nact, K), np.float64)
    per_chunk = 0.5 / 0.016875
    with np.errstate(all="ignore"):
        for c in range(chunks):
            n = min(FRAMES, nact - sfr[c])
            f = sfr[c] + np.arange(n)
            live = np.ones(n, bool)
            if mistake == "bracket_0":
                lo = np.maximum(((f - (FRAMES - 1)) / per_chunk).astype(np.int64), 0)
                hi = np.minimum((f / per_chunk).astype(np.int64), chunks - 1)
                live = (lo <= c) & (c <= hi)
            for k in range(K):
                who = [s for s in range(SPEAKERS) if hard[c, s] == k]
                if not who:
                    continue
                mx = np.full(n, -np.inf, np.float32)
                for s in who:
                    v = seg[c, :n, s]
                    mx = np.where(mx < v, v, mx)
                act[f[live], k] += mx[live].astype(np.float64)
    return act


def topk(act, count, ar0, cr0, rows, crow, mistake=None, slack=0):
    """binary[i] = 1 for the min(count[cr0 + i], K) largest of act[ar0 + i], stable order of the negated values on ties (sd.cpp:2681, 2720-2759); rows from
    crow on have no count: zeros -> uint8 [rows][K] (`slack` further rows of zeros, for a mistake that writes behind a row)"""
    act = np.asarray(act, np.float64)
    K = act.shape[1]
    out = np.zeros(((rows + slack) * K), np.uint8)
    for i in range(rows):
        n = int(count[cr0 + i]) if i < crow else 0
        a = -1.0 * act[ar0 + i]
        order = np.argsort(a, kind="stable") if mistake != "unstable_topk" else (K - 1 - np.argsort(a[::-1], kind="stable"))
        if mistake == "count_unclamped" and n > K:
            out[i * K + K:i * K + n] = 1                                      # entries K .. n - 1 of a "sorted" row that has only K
        out[i * K + order[:min(n, K)]] = 1
    return out.reshape(rows + slack, K)


# ---------------------------------------------------------------- cut.hip
def cen_norms(cen, mistake=None):
    """k_cut_cen_norms: m2 of every row of the table, the sequential sum of k_assign"""
    cen = np.asarray(cen, np.float64)
    return seq_sum(cen * cen, 1, mistake)


def assign_cuts(E, cen, coff, slot, n_slots, nact, mistake=None):
    """k_cut_cen_norms + k_assign_cuts: cut q is k_assign on rows [coff[q], coff[q + 1]) of the table, then the inactive rule; hard row slot[q], best row q
    -> m2 [total], hard int32 [n_slots][M] (None where no cut writes), best [Tn][M], err"""
    E = np.asarray(E, np.float64)
    M, Tn = E.shape[0], len(slot)
    hard, best, err = [None] * n_slots, np.zeros((Tn, M)), 0
    for q in range(Tn):
        a, b = int(coff[q]), int(coff[q + 1])
        if mistake == "carry_dropped":
            soft, e = soft_scores(E, cen[a:b])
            edges = [j - a for j in range(TILE, b, TILE) if j > a]          # the table's tile edges inside this cut
            res = [first_max(row, mistake, edges=edges) for row in soft]
            h, bs = np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res])
        else:
            h, e, _, bs = assign(E, cen[a:b], mistake if mistake in ("pairwise_sum", "ge_argmax") else None)
        err |= e
        hard[q if mistake == "slot_ignored" else int(slot[q])] = mark_inactive(h, nact, mistake)
        best[q] = bs
    return cen_norms(cen, mistake), hard, best, err


def recon_cuts(seg, hard, koff, count, ar0, cr0, rows, crow, act_in=None, mistake=None):
    """k_activations_cuts + k_topk_cuts: cut t is activations / topk with K_t = koff[t + 1] - koff[t] -> act [frames * koff[-1]], binary uint8 [rows * koff[-1]]"""
    chunks = np.asarray(seg).shape[0]
    nact, _ = activation_frames(chunks)
    acts, bins = [], []
    for t in range(len(koff) - 1):
        K = int(koff[t + 1] - koff[t])
        a = activations(seg, np.asarray(hard[t]).reshape(chunks, SPEAKERS), K, mistake)
        acts.append(a.reshape(-1))
        src = a if act_in is None else np.asarray(act_in, np.float64)[int(koff[t]) * nact:int(koff[t + 1]) * nact].reshape(nact, K)
        bins.append(topk(src, count, ar0, cr0, rows, crow, mistake).reshape(-1))
    return np.concatenate(acts), np.concatenate(bins)


# ---------------------------------------------------------------- pipeline.cpp
def pcm_to_f32(pcm):
    """sample * 1.0f / 32768.0 (sd.cpp:2948-2951), then the 512 zeros of SD_WAV_PAD"""
    return np.concatenate([np.asarray(pcm, np.int16).astype(np.float32) * np.float32(1.0 / 32768.0), np.zeros(512, np.float32)])


def f32_to_f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------- the crop of to_diarization (host code of reconstruct.hip), for the pin to the oracle
def crop_ranges(chunks):
    """sd.cpp:2691-2706 with crop_segment's float intermediates (2567-2618) -> ar0, cr0, rows, crow as run_reconstruct hands them to k_topk"""
    nact, n_count = activation_frames(chunks)[0], count_frames(chunks)
    step = dur = orc.FRAME_STEP
    a_end = 0.0 + (0 - .5) * step + .5 * dur + nact * step
    c_end = 0.5 + (0 - .5) * step + .5 * dur + n_count * step
    f0, f1 = max(0.0, 0.5), min(a_end, c_end)

    def crop(w_start, n_rows):
        rs = max(int(np.ceil(np.float32((f0 - dur - w_start) / step))), 0)
        re = int(np.floor(np.float32((f1 - w_start) / step))) + 1
        return (0, 0) if rs >= n_rows else (rs, max(min(re, n_rows), rs))

    (ar0, ar1), (cr0, cr1) = crop(0.0, nact), crop(0.5, n_count)
    return ar0, cr0, ar1 - ar0, min(cr1 - cr0, ar1 - ar0)
