"""Plain numpy references of the kernels of csrc/pyannet.hip that are not convolutions, for tests/test_seg_kernels.py:

    lstm_ref        k_lstm_rec / k_lstm_rec_x3    bidirectional LSTM recurrence over pre-computed input projections
    pool_norm_ref   k_pool_norm                   |.| (stage 0) -> MaxPool1d(3) -> InstanceNorm1d(C, affine) -> LeakyReLU(0.01)
    chunk_norm_ref  k_chunk_norm / k_chunk_stats  InstanceNorm1d(1, affine) of a chunk of L samples, zero beyond L; (a, c) of the affine form
    classifier_ref  k_classifier                  Linear(128 -> 3) + sigmoid, frames >= F zero

Each takes dtype (float64: the reference; float32: the same graph as a yardstick of what f32 arithmetic costs) and mutant (None, or the name
of ONE deliberate mistake: tests/test_seg_ref.py shows that the tolerances of the GPU tests tell every mutant from the reference).
tests/test_seg_ref.py pins all four to torch in float64 before anything is compared with them.  The *_bound functions are the rounding
bounds the GPU tests assert; their derivation is in the docstring of tests/test_seg_kernels.py."""
import numpy as np

EPS = 1e-5
U = 2.0 ** -24                      # unit roundoff of f32, round to nearest

LSTM_MUTANTS = ("swap_g_o", "swap_whh", "no_reverse", "carry_state", "drop_input")
POOL_MUTANTS = ("var_unbiased", "no_eps", "no_abs", "shift_window", "stats_short", "slope0")
CHUNK_MUTANTS = ("stats_80000", "var_unbiased", "no_eps")
CLS_MUTANTS = ("no_zero", "perm_w")


def gamma(n):
    return n * U / (1.0 - n * U)


def _sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---------------------------------------------------------------- LSTM
def lstm_ref(G, whh_f, whh_b, dtype=np.float64, mutant=None):
    """G [B][F][1024]: per direction 512 = gates i, f, g, o x 128 units (input projection + b_ih + b_hh); whh_f / whh_b [512][128]
    -> H [B][F][256] (forward units, then backward units), PyTorch's nn.LSTM equations with h_0 = c_0 = 0"""
    assert mutant is None or mutant in LSTM_MUTANTS, mutant
    G = np.asarray(G, dtype)
    B, F, _ = G.shape
    W = [np.asarray(whh_f, dtype), np.asarray(whh_b, dtype)]
    if mutant == "swap_whh":
        W = W[::-1]
    if mutant == "drop_input":
        W = [w.copy() for w in W]
        for w in W:
            w[:, 77] = 0
    H = np.zeros((B, F, 256), dtype)
    for d in range(2):
        g = G[:, :, 512 * d:512 * (d + 1)]
        Wt = np.ascontiguousarray(W[d].T)
        groups = [slice(b, b + 1) for b in range(B)] if mutant == "carry_state" else [slice(0, B)]
        h = c = None
        for rows in groups:
            n = rows.stop - rows.start
            if h is None or mutant != "carry_state":
                h, c = np.zeros((n, 128), dtype), np.zeros((n, 128), dtype)
            for step in range(F):
                t = F - 1 - step if (d == 1 and mutant != "no_reverse") else step
                pre = g[rows, t] + h @ Wt
                i, f, gg, o = pre[:, :128], pre[:, 128:256], pre[:, 256:384], pre[:, 384:]
                if mutant == "swap_g_o":
                    gg, o = o, gg
                c = _sigm(f) * c + _sigm(i) * np.tanh(gg)
                h = _sigm(o) * np.tanh(c)
                H[rows, t, 128 * d:128 * (d + 1)] = h
    return H


# ---------------------------------------------------------------- pool + instance norm + leaky relu
def pool_norm_ref(x, chunks, Lc, stage, gw, gb, cst=None, wsum=None, chunk_rows=0, dtype=np.float64, mutant=None, parts=False):
    """x [in_rows][C] (C = 80 at stage 0, 60 at stages 1, 2).  Chunk ck's rows start at ck * Lc, or -- shared form, cst [chunks][2] = (a, c),
    wsum [C] -- at ck * chunk_rows, and its values are a_ck * x + c_ck * wsum[channel].  Lp = Lc // 3 windows of 3 rows; the Lc % 3 last rows are dropped.
    -> out [chunks][Lp][C]; parts = True: also a dict of the float-`dtype` m [chunks][Lp][C], mu, var [chunks][C] and dm (the shared form's |v a| + |c wsum|
    of the pooled element)"""
    assert mutant is None or mutant in POOL_MUTANTS, mutant
    x = np.asarray(x, dtype)
    C = x.shape[1]
    assert C == (80 if stage == 0 else 60)
    gw, gb = np.asarray(gw, dtype), np.asarray(gb, dtype)
    Lp = Lc // 3
    shared = cst is not None
    start = (lambda ck: ck * chunk_rows) if shared else (lambda ck: ck * Lc)
    sh = 1 if mutant == "shift_window" else 0
    xx = np.concatenate([x, np.full((1, C), np.nan, dtype)])           # (the shifted mutant's last window may reach one row beyond the input)
    v = np.stack([xx[start(ck) + sh:start(ck) + sh + 3 * Lp] for ck in range(chunks)]).reshape(chunks, Lp, 3, C)
    mag = np.zeros_like(v)
    if shared:
        ca = np.asarray(cst, dtype)[:, 0].reshape(chunks, 1, 1, 1)
        cc = np.asarray(cst, dtype)[:, 1].reshape(chunks, 1, 1, 1) * np.asarray(wsum, dtype)
        mag = np.abs(v * ca) + np.abs(cc)
        v = v * ca + cc
    if stage == 0 and mutant != "no_abs":
        v = np.abs(v)
    m = v.max(2)                                                       # [chunks][Lp][C]
    dm = np.take_along_axis(mag, v.argmax(2)[:, :, None, :], 2)[:, :, 0, :]
    ms = m[:, :Lp - 1] if mutant == "stats_short" else m
    with np.errstate(all="ignore"):
        mu = ms.sum(1) / dtype(ms.shape[1])
        var = ((ms - mu[:, None, :]) ** 2).sum(1) / dtype(max(Lp - 1, 1) if mutant == "var_unbiased" else ms.shape[1])
        r = 1.0 / np.sqrt(var + (0.0 if mutant == "no_eps" else dtype(EPS)))
        y = (m - mu[:, None, :]) * r[:, None, :] * gw + gb
    y = np.where(y > 0, y, dtype(0.0 if mutant == "slope0" else 0.01) * y)
    if parts:
        return y, dict(m=m, mu=mu, var=var, dm=dm)
    return y


def pool_norm_bound(p, gw, gb, shared=False):
    """per-element bound [chunks][Lp][C] from the float64 parts of pool_norm_ref (derivation: tests/test_seg_kernels.py)"""
    m, mu, var, dm = p["m"], p["mu"][:, None, :], p["var"][:, None, :], p["dm"]
    Lp = m.shape[1]
    gw, gb = np.abs(np.asarray(gw, np.float64)), np.abs(np.asarray(gb, np.float64))
    a = gw / np.sqrt(var + EPS)
    d_m = 2 * U * dm if shared else np.zeros_like(m)
    d_mu = gamma(Lp) * np.abs(m).mean(1, keepdims=True) + U * np.abs(mu) + d_m.mean(1, keepdims=True)
    d_var = gamma(Lp + 3) * var + d_mu ** 2
    return a * np.abs(m - mu) * (d_var / (2 * (var + EPS)) + 4 * U) + a * d_mu + 3 * U * (a * np.abs(m) + a * np.abs(mu) + gb) + a * d_m


# ---------------------------------------------------------------- chunk normalisation
def chunk_norm_ref(wav, origin, first_chunk, hop, L, chunks, w, b, dtype=np.float64, mutant=None, parts=False):
    """chunk ck = wav[(first_chunk + ck) * hop - origin :][:L] -> (xn [chunks][80000], zero from L on; ac [chunks][2]: xn = a x + c)"""
    assert mutant is None or mutant in CHUNK_MUTANTS, mutant
    wav = np.concatenate([np.asarray(wav, dtype), np.full(80000, np.nan, dtype)])      # (the stats_80000 mutant reads beyond short inputs)
    w, b = dtype(w), dtype(b)
    n = 80000 if mutant == "stats_80000" else L
    base = [(first_chunk + ck) * hop - origin for ck in range(chunks)]
    assert min(base) >= 0
    xs = np.stack([wav[s:s + n] for s in base])
    x = xs[:, :L]
    mu = xs.mean(1)
    var = ((xs - mu[:, None]) ** 2).sum(1) / dtype(max(n - 1, 1) if mutant == "var_unbiased" else n)
    with np.errstate(all="ignore"):
        r = 1.0 / np.sqrt(var + (0.0 if mutant == "no_eps" else dtype(EPS)))
        a = r * w
        c = b - mu * a
        xn = np.zeros((chunks, 80000), dtype)
        xn[:, :L] = (x - mu[:, None]) * a[:, None] + b
    ac = np.stack([a, c], 1)
    if parts:
        return xn, ac, dict(x=x, mu=mu, var=var)
    return xn, ac


def chunk_norm_bound(p, w, b):
    """-> (bound of xn[:, :L] [chunks][L], bound of a [chunks], bound of c [chunks]): pool_norm_bound's form with Lp -> L, gw -> w, m -> x"""
    x, mu, var = p["x"], p["mu"], p["var"]
    L = x.shape[1]
    a = abs(float(w)) / np.sqrt(var + EPS)
    d_mu = gamma(L) * np.abs(x).mean(1) + U * np.abs(mu)
    d_var = gamma(L + 3) * var + d_mu ** 2
    rel = d_var / (2 * (var + EPS)) + 4 * U
    A, MU = a[:, None], mu[:, None]
    bx = A * np.abs(x - MU) * rel[:, None] + (a * d_mu)[:, None] + 3 * U * (A * np.abs(x) + A * np.abs(MU) + abs(float(b)))
    ba = a * rel
    bc = np.abs(mu) * ba + a * d_mu + 3 * U * (a * np.abs(mu) + abs(float(b)))
    return bx, ba, bc


# ---------------------------------------------------------------- classifier
def classifier_ref(y, W, b, chunks, F, dtype=np.float64, mutant=None, parts=False):
    """y [chunks * F][128], W [3][128], b [3] -> seg [chunks][293][3]: sigmoid(W y + b) for frames < F, zero from F on"""
    assert mutant is None or mutant in CLS_MUTANTS, mutant
    y, W, b = np.asarray(y, dtype), np.asarray(W, dtype), np.asarray(b, dtype)
    if mutant == "perm_w":
        W = np.roll(W, 1, 0)
    seg = np.zeros((chunks, 293, 3), dtype)
    if mutant == "no_zero":
        seg[:] = _sigm(b)                                 # (what an unguarded frame gives at best: no input at all)
    seg[:, :F] = _sigm(y @ W.T + b).reshape(chunks, F, 3)
    if parts:
        S = np.zeros((chunks, 293, 3))
        S[:, :F] = (np.abs(y.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))).reshape(chunks, F, 3)
        return seg, S
    return seg


def classifier_bound(seg, S):
    """gamma_131 S (128 products, 128 additions in any order, the bias) through the 1-Lipschitz sigmoid, + 4 ulp of the output for expf and the division"""
    return gamma(131) * S + 4 * 2.0 ** -23 * np.abs(seg)
