"""Float64 references of the glue kernels of csrc/ecapa.hip (k_masked_mean, k_asp_stats, k_asp_pool, k_se_apply, k_build_rowtab, k_scatter_emb,
k_feats_to_half, k_rows_to_half), written from the definitions -- two passes, no running quantities -- and not from the kernels.
tests/test_ecapa_glue_ref.py pins them to the torch formulas of oracle/nn_oracle.py; tests/test_ecapa_glue.py compares the kernels with them.

Layout of the statistics operands, as run_ecapa_t hands them over: x [rows][ld], item i's frames at rows rowoff[i] - rowoff[0] + t, of which the first
nvalid[i] count; C <= ld channels.  `mutant` selects a deliberate mistake (test_ecapa_glue_ref.py shows that the tolerances tell each from the
reference).

The error bounds (*_bound) are derived in the docstring of tests/test_ecapa_glue.py; they are functions of the float64 quantities only."""
import numpy as np

EPS = 1e-12
U = 2.0 ** -24                              # unit roundoff of float32
STD_FLOOR_F32 = float(np.sqrt(np.float32(1e-12)))      # sqrtf(1e-12f): what a clamped variance gives


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u)"""
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


STATS_MUTANTS = ["div_nm1", "div_np1", "incl_nv", "skip_last", "no_clamp", "clamp_after", "eps6"]
MEAN_MUTANTS = ["div_nm1", "div_np1", "incl_nv", "skip_last"]
POOL_MUTANTS = ["incl_nv", "skip_last", "no_clamp", "clamp_after", "eps6", "no_rescale", "unweighted_mean"]
SE_MUTANTS = ["next_gate", "res_off1", "out_at_t2_row"]
ROWTAB_MUTANTS = ["n_in"]


def _frames(x, nvalid, rowoff, C, i, mutant=None):
    """the frames of item i that enter its statistics [n][C], and the divisor"""
    r0, nv = int(rowoff[i] - rowoff[0]), int(nvalid[i])
    n = nv + 1 if mutant == "incl_nv" else (nv - 1 if mutant == "skip_last" else nv)
    rows = np.full((n, C), np.nan)
    have = max(0, min(n, x.shape[0] - r0))                # (incl_nv behind the last item: the NaN guard behind the buffer)
    rows[:have] = x[r0:r0 + have, :C]
    div = {"div_nm1": nv - 1, "div_np1": nv + 1}.get(mutant, nv)
    return rows, float(div)


def _std(var, mutant):
    eps = 1e-6 if mutant == "eps6" else EPS
    if mutant == "no_clamp":
        return np.sqrt(var)
    if mutant == "clamp_after":
        return np.maximum(np.sqrt(var), eps)
    return np.sqrt(np.maximum(var, eps))


def masked_mean_ref(x, nvalid, rowoff, C, mutant=None):
    """SEBlock's masked mean: mean over the frames < nvalid  -> [items][C]"""
    out = np.zeros((len(nvalid), C))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(nvalid)):
            v, div = _frames(x, nvalid, rowoff, C, i, mutant)
            out[i] = v.sum(0) / div
    return out


def asp_stats_ref(x, nvalid, rowoff, C, mutant=None):
    """population mean and sqrt(max(var, 1e-12)) over the frames < nvalid  -> [items][2 C]"""
    out = np.zeros((len(nvalid), 2 * C))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(nvalid)):
            v, div = _frames(x, nvalid, rowoff, C, i, mutant)
            mean = v.sum(0) / div
            var = ((v - mean) ** 2).sum(0) / div
            out[i, :C], out[i, C:] = mean, _std(var, mutant)
    return out


def asp_pool_ref(x, logits, nvalid, rowoff, C, mutant=None):
    """softmax over the frames < nvalid of the logits, then the weighted mean and sqrt(max(sum w (x - mean)^2, 1e-12))  -> [items][2 C]"""
    out = np.zeros((len(nvalid), 2 * C))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(len(nvalid)):
            v, _ = _frames(x, nvalid, rowoff, C, i, mutant)
            l, _ = _frames(logits, nvalid, rowoff, C, i, mutant)
            if len(v) == 0:                                  # (skip_last on one frame: a softmax over nothing)
                out[i] = np.nan
                continue
            if mutant == "no_rescale":
                # a one-pass softmax that takes a new maximum without renormalising what it has summed: frame t's weight stays
                # exp(l_t - max(l_0 .. l_t)) while the later ones are taken against a larger maximum
                w = np.exp(l - np.maximum.accumulate(l, 0))
            else:
                w = np.exp(l - l.max(0))
            w = w / w.sum(0)
            mean = (w * v).sum(0)
            about = v.mean(0) if mutant == "unweighted_mean" else mean
            var = (w * (v - about) ** 2).sum(0)
            out[i, :C], out[i, C:] = mean, _std(var, mutant)
    return out


# ---------------------------------------------------------------- bounds of the statistics (derived in tests/test_ecapa_glue.py)
def masked_mean_bound(x, nvalid, rowoff, C):
    """gamma_(nv // 4 + 6) mean|x|: four partial sums of nv // 4 additions, the tail's three, two more to join them, one division"""
    out = np.zeros((len(nvalid), C))
    for i in range(len(nvalid)):
        v, _ = _frames(x, nvalid, rowoff, C, i)
        out[i] = gamma(len(v) // 4 + 6) * np.abs(v).mean(0)
    return out


def _sqrt_bound(var, dvar, std):
    """|sqrt(max(a, eps)) - sqrt(max(b, eps))| for |a - b| <= dvar, plus 2 u std for sqrtf and the store"""
    lo = np.sqrt(np.maximum(np.maximum(var, EPS) - dvar, EPS))
    return dvar / (std + lo) + 2 * U * std


def _welford_bound(v, p, eps_k, wt_err):
    """One-pass weighted mean / variance with update mean_k = mean_(k-1) + r_k d_k, d_k = v_k - mean_(k-1), r_k = w_k / W_k, and
    m2 += w_k d_k (v_k - mean_k), on weights p (normalised, [n][C]) whose ratio r_k the kernel has to a relative eps_k [n][C] and whose share of
    the final m2 / W to a relative wt_err [n][C]; float32 otherwise.  -> (mean, var, d_mean, d_var) of the final results"""
    n = v.shape[0]
    P = np.cumsum(p, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        run = np.where(P > 0, np.cumsum(p * v, 0) / P, 0.0)  # mean_k
    prev = np.concatenate([np.zeros_like(run[:1]), run[:-1]])
    d = v - prev
    # error of mean_k: sum over j <= k of (P_j / P_k) (r_j eps_j |d_j| + u |mean_j|): the ratio's error times the step, the rounding of the sum
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.where(P > 0, np.cumsum(p * eps_k * np.abs(d) + U * P * np.abs(run), 0) / P, 0.0)
    Eprev = np.concatenate([np.zeros_like(E[:1]), E[:-1]])
    mean, d_mean = run[-1], E[-1]
    t = d * (v - run)                                        # the terms of m2, all >= 0
    var = (p * t).sum(0)
    # each term: its two factors carry the running mean's error (the product of the two errors included: on a large mean it is no second-order
    # term), its weight wt_err; three roundings of its own, the sum's gamma_n
    d_var = (p * (np.abs(d) * E + np.abs(v - run) * Eprev + E * Eprev + t * wt_err)).sum(0) + (3 * U + gamma(n + 2)) * var
    s = 1.0 / (1.0 - 4 * n * U)                              # second-order terms
    return mean, var, d_mean * s, d_var * s


def asp_stats_bound(x, nvalid, rowoff, C):
    """-> bound [items][2 C] of (mean | std) of k_asp_stats.  Uniform weights: r_k = 1 / k is one correctly rounded division of d_k: eps_k = 3 u
    (the subtraction, the division, nothing else)"""
    out = np.zeros((len(nvalid), 2 * C))
    for i in range(len(nvalid)):
        v, _ = _frames(x, nvalid, rowoff, C, i)
        n = len(v)
        p = np.full_like(v, 1.0 / n)
        mean, var, dm, dv = _welford_bound(v, p, np.full_like(v, 3 * U), np.zeros_like(v))
        out[i, :C] = dm + U * np.abs(mean)
        out[i, C:] = _sqrt_bound(var, dv + U * var, np.sqrt(np.maximum(var, EPS)))
    return out


def exp_error(a):
    """relative error of __expf(a) = v_exp_f32(a * log2(e)) for an argument a that is itself a rounded difference: the subtraction, the product and
    the constant each move the exponent by |a| u; the instruction is ASSUMED good to 1 ulp = 2 u (the guides give no figure)"""
    return 3 * np.abs(a) * U + 2 * U


def asp_pool_bound(x, logits, nvalid, rowoff, C):
    """-> bound [items][2 C] of (mean | std) of k_asp_pool; see tests/test_ecapa_glue.py"""
    out = np.zeros((len(nvalid), 2 * C))
    for i in range(len(nvalid)):
        v, _ = _frames(x, nvalid, rowoff, C, i)
        l, _ = _frames(logits, nvalid, rowoff, C, i)
        n = len(v)
        mx = np.maximum.accumulate(l, 0)
        a = l - mx                                           # argument of frame k's weight (0 where it sets a new maximum)
        prev_mx = np.concatenate([l[:1], mx[:-1]])
        resc = l > prev_mx                                   # frames that rescale W and m2 ...
        resc[0] = False                                      # (the first multiplies zeros by exp(-inf) = 0)
        S = np.cumsum(np.where(resc, exp_error(prev_mx - l) + U, 0.0), 0)      # ... and what the factors so far have cost every earlier weight
        # a weight below 2^-126 is flushed to zero: an absolute error, relative to the weight as large as it takes
        own = exp_error(a) + np.minimum(1.0, 2.0 ** -126 / np.maximum(np.exp(a), 1e-300))
        k = np.arange(1, n + 1, dtype=np.float64)[:, None]
        w = np.exp(l - l.max(0))
        p = w / w.sum(0)
        P = np.cumsum(p, 0)
        # relative error of W_k: every component's own error + the rescales since, weighted by its share of W_k, + the sum's gamma_k
        with np.errstate(divide="ignore", invalid="ignore"):
            eW = np.where(P > 0, np.cumsum(p * (own - S), 0) / P, 0.0) + S + gamma(k)
        # r_k = w_k * rcp(W_k): own error, W's, v_rcp_f32 (ASSUMED 1 ulp = 2 u), the product; d_k's subtraction and the product with it
        eps_k = own + eW + 2 * U + U + 2 * U
        # the share of term k in m2 / W at the end: its weight, the rescales since, W_n, the products w d (v - mean) and the division
        wt_err = own + (S[-1] - S) + eW[-1] + 4 * U
        mean, var, dm, dv = _welford_bound(v, p, eps_k, wt_err)
        out[i, :C] = dm + U * np.abs(mean)
        out[i, C:] = _sqrt_bound(var, dv, np.sqrt(np.maximum(var, EPS)))
    return out


# ---------------------------------------------------------------- row tables, k_se_apply
def rowtab_ref(off_out, off_in, mutant=None):
    """k_build_rowtab: for every row of the output space (i0, t | (n_in - 1) << 10 | item << 20), i0 = the item's first row in the input space"""
    off_out, off_in = np.asarray(off_out, np.int64), np.asarray(off_in, np.int64)
    tab = np.zeros((off_out[-1] - off_out[0], 2), np.int64)
    for i in range(len(off_out) - 1):
        n_out, n_in = off_out[i + 1] - off_out[i], off_in[i + 1] - off_in[i]
        t = np.arange(n_out)
        r0 = off_out[i] - off_out[0]
        tab[r0:r0 + n_out, 0] = off_in[i] - off_in[0]
        tab[r0:r0 + n_out, 1] = t | ((n_in if mutant == "n_in" else n_in - 1) << 10) | (i << 20)
    return (tab & 0xffffffff).astype(np.uint32).view(np.int32)


def se_apply_ref(t2, gate, res, off, os, rs, ys, *, shared, y_ld, out_col0, res_col0=0, canary=-7776.0, mutant=None):
    """y = gate[item] * t2 + residual at every (item, frame) of space `os`, written into the [rows of space ys][y_ld] buffer of the hook
    (Diarizer.se_apply_case).  -> (buffer, written): the buffer as it must come back -- the canary, the residual slice (shared) and the results --
    and the mask of the elements the kernel writes.  |g t2| + |r| per written element comes back as a third array."""
    items, C = gate.shape
    Ry = int(off[ys][-1])
    buf = np.full((Ry, y_ld), canary, np.float64)
    mag = np.zeros((Ry, y_ld))
    written = np.zeros((Ry, y_ld), bool)
    if shared:
        buf[:, res_col0:res_col0 + C] = res
    src = np.asarray(res, np.float64)[:, :C]
    for i in range(items):
        n = int(off[os][i + 1] - off[os][i])
        g = gate[(i + 1) % items if mutant == "next_gate" else i].astype(np.float64)
        a = t2[off[os][i]:off[os][i] + n, :C].astype(np.float64)
        rr = off[rs][i] + np.arange(n) + (1 if mutant == "res_off1" else 0)
        r = np.full((n, C), np.nan)
        ok = rr < len(src)
        r[ok] = src[rr[ok]]
        orow = (off[os][i] if mutant == "out_at_t2_row" else off[ys][i]) + np.arange(n)
        buf[orow, out_col0:out_col0 + C] = g * a + r
        mag[orow, out_col0:out_col0 + C] = np.abs(g * a) + np.abs(r)
        written[orow, out_col0:out_col0 + C] = True
    return buf, written, mag


def se_apply_bound(buf, written, mag, f16):
    """2 u (|g a| + |r|): the product and the sum, or the one rounding of an FMA, each within u of a magnitude below |g a| + |r|; an fp16 store adds
    half an fp16 ulp of the stored value (2^-25 in the subnormal range).  0 where nothing may be written"""
    tol = np.where(written, 2 * U * mag, 0.0)
    if f16:
        tol = np.where(written, tol + np.maximum(2.0 ** -11 * (np.abs(buf) + tol), 2.0 ** -25), 0.0)
    return tol


def scatter_emb_ref(emb_c, cidx):
    """k_scatter_emb: row i = compact row cidx[i], or the NaN 0x7fc00000 where cidx[i] < 0 (as bit patterns)"""
    bits = np.ascontiguousarray(emb_c, np.float32).view(np.uint32).reshape(-1, 192)
    out = np.full((len(cidx), 192), 0x7fc00000, np.uint32)
    live = np.asarray(cidx) >= 0
    out[live] = bits[np.asarray(cidx)[live]]
    return out


def to_half_ref(f, feats):
    """numpy's float32 -> float16 rounding (nearest even, overflow to inf); feats: [rows][96] -> [rows][128] with zeros behind column 96"""
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(f, np.float32).astype(np.float16)
    if feats:
        h = np.concatenate([h, np.zeros((h.shape[0], 32), np.float16)], 1)
    return h
