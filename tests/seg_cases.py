"""The cases of tests/test_seg_kernels.py and their operands, in one place: the GPU tests run them, tests/test_seg_ref.py shows on the CPU that
each case's tolerance tells the mutants of tests/seg_ref.py from the reference.  Operands and references are computed once per case and
shared read-only."""
import functools

import numpy as np

import seg_ref as R


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


# ---------------------------------------------------------------- LSTM
LSTM_SHAPES = [(1, 1), (1, 293), (31, 7), (32, 5), (33, 171), (64, 3), (65, 30)]       # (B, F): one lane; the real F; 32 - 1; 32; 32 + 1 at the short last
LSTM_DATA = ["mid", "wide", "small", "whh0"]                                            # chunk's F; 64; 64 + 1
LSTM_CASES = [(B, F, kind) for (B, F) in LSTM_SHAPES for kind in LSTM_DATA]


@functools.lru_cache(maxsize=None)
def lstm_operands(B, F, kind):
    """mid: G ~ 1.5 N(0, 1), W_hh ~ U(+-0.088) (PyTorch's initial range 1 / sqrt(128)); wide: G ~ 3 N, W_hh ~ U(+-0.5); small: G ~ 0.15 N: the
    pre-activations and cell states sit on both sides of tanh_fast's switch at 0.18; whh0: W_hh = 0: H depends on G element by element"""
    rng = np.random.default_rng(1000 * B + F + 7 * LSTM_DATA.index(kind))
    gs, ws = {"mid": (1.5, 0.088), "wide": (3.0, 0.5), "small": (0.15, 0.088), "whh0": (1.5, 0.0)}[kind]
    G = (gs * rng.standard_normal((B, F, 1024))).astype(np.float32)
    wf = (ws * rng.uniform(-1, 1, (512, 128))).astype(np.float32)
    wb = (ws * rng.uniform(-1, 1, (512, 128))).astype(np.float32)
    _ro(G, wf, wb)
    return G, wf, wb


@functools.lru_cache(maxsize=4)
def lstm_reference(B, F, kind):
    """-> (H float64 [B][F][256], e32 = max error of the float32 evaluation of the same graph)"""
    G, wf, wb = lstm_operands(B, F, kind)
    H = R.lstm_ref(G, wf, wb)
    e32 = float(np.abs(R.lstm_ref(G, wf, wb, dtype=np.float32).astype(np.float64) - H).max())
    _ro(H)
    return H, e32


# ---------------------------------------------------------------- pool_norm
POOL_FORMS = ["stage0", "stage1", "stage2", "shared0"]
POOL_LC = [3, 5, 17, 40, 49, 121]           # Lp = 1 (var = 0), 1, 5, 13, 16, 40: Lc % 3 = 0, 2, 2, 1, 1, 1; Q = 12 (C 80) / 16 (C 60) row groups lie between 5 and 40
POOL_REAL = {"stage0": 7975, "stage1": 2654, "stage2": 880, "shared0": 7975}           # the lengths of a full chunk (Lp = 2658 / 884 / 293): strided loops
POOL_KINDS = ["normal", "mean5", "outlier"]
POOL_CASES = [(form, Lc, chunks, kind) for form in POOL_FORMS for Lc in POOL_LC + [POOL_REAL[form]] for chunks in (1, 3) for kind in POOL_KINDS]


@functools.lru_cache(maxsize=None)
def pool_operands(form, Lc, chunks, kind):
    """-> dict(x, chunks, Lc, stage, gw, gb, cst, wsum, chunk_rows).  normal: N(0, 1); mean5: 0.01 N + 5; outlier: every channel a constant of its own
    with ONE outlier row per chunk.  shared0: the chunk's values are a_ck x + c_ck wsum: a in 0.5 .. 20, and for mean5 the large mean is 5 wsum in
    x and cancels against c_ck wsum, as a DC offset of the waveform does"""
    stage = {"stage0": 0, "stage1": 1, "stage2": 2, "shared0": 0}[form]
    C = 80 if stage == 0 else 60
    shared = form == "shared0"
    rng = np.random.default_rng(100000 * POOL_FORMS.index(form) + 10 * Lc + chunks + 3 * POOL_KINDS.index(kind))
    chunk_rows = (800 if Lc > 800 else (Lc + 1) // 2) if shared else 0
    rows = (chunks - 1) * chunk_rows + Lc if shared else chunks * Lc
    cst = wsum = None
    if shared:
        wsum = (0.3 * rng.standard_normal(80)).astype(np.float32)
        cst = np.stack([rng.uniform(0.5, 20.0, chunks), rng.standard_normal(chunks)], 1).astype(np.float32)
    if kind == "normal":
        x = rng.standard_normal((rows, C))
    elif kind == "mean5":
        x = 0.01 * rng.standard_normal((rows, C)) + (5.0 * wsum.astype(np.float64) if shared else 5.0)
        if shared:
            cst[:, 1] = (-5.0 * cst[:, 0].astype(np.float64) + 0.1 * rng.standard_normal(chunks)).astype(np.float32)
    else:
        x = np.tile(rng.uniform(-2, 2, (1, C)), (rows, 1))
        span = chunk_rows if shared and chunks > 1 else Lc
        for ck in range(chunks):
            x[ck * span + rng.integers(0, min(span, Lc), C), np.arange(C)] = rng.choice([-40.0, 40.0], C)
    x = x.astype(np.float32)
    gw = rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    gb = (0.5 * rng.standard_normal(C)).astype(np.float32)
    _ro(x, gw, gb, cst, wsum)
    return dict(x=x, chunks=chunks, Lc=Lc, stage=stage, gw=gw, gb=gb, cst=cst, wsum=wsum, chunk_rows=chunk_rows)


@functools.lru_cache(maxsize=8)
def pool_reference(form, Lc, chunks, kind):
    """-> (y float64 [chunks][Lp][C], bound)"""
    o = pool_operands(form, Lc, chunks, kind)
    y, p = R.pool_norm_ref(parts=True, **o)
    bound = R.pool_norm_bound(p, o["gw"], o["gb"], shared=form == "shared0")
    _ro(y, bound)
    return y, bound


# ---------------------------------------------------------------- chunk_norm / chunk_stats
CHUNK_L = [1, 255, 257, 1000, 80000]        # one sample (var = 0); one short of / one beyond the 256 threads; a few strides; the full chunk
CHUNK_KINDS = ["loud_dc", "near_silent"]
# (layout, L, kind): "slide" = 3 chunks, hop 8000 (both kernels); "rows" = 3 rows of L samples, hop = L (k_chunk_norm alone: k_chunk_stats's hop is 8000);
# "offset" = hop 8000 with first_chunk = 2 and origin = 12000: wav[0] is sample 12000 of the recording
CHUNK_CASES = [(lay, L, kind) for lay in ("slide", "rows") for L in CHUNK_L for kind in CHUNK_KINDS] + [("offset", 1000, k) for k in CHUNK_KINDS]


@functools.lru_cache(maxsize=None)
def chunk_operands(layout, L, kind):
    """loud_dc: 0.4 N + 0.3; near_silent: 2e-4 N + 0.05 (DC / sigma = 250, variance far below eps), as in
    test_segmentation_shared_conv0_with_a_dc_offset_on_near_silence; each chunk at a level of its own"""
    rng = np.random.default_rng(10 * L + CHUNK_KINDS.index(kind) + {"slide": 0, "rows": 3, "offset": 5}[layout])
    chunks = 3
    hop = L if layout == "rows" else 8000
    first_chunk, origin = (2, 12000) if layout == "offset" else (0, 0)
    n = (first_chunk + chunks - 1) * hop - origin + L
    n += 4000 if layout == "offset" else 0                 # samples behind the last chunk, as a recording has
    sig, dc = (0.4, 0.3) if kind == "loud_dc" else (2e-4, 0.05)
    wav = sig * rng.standard_normal(n) * (1.0 + 0.5 * np.sin(np.arange(n) / 700.0)) + dc
    wav = wav.astype(np.float32)
    w, b = (1.3, -0.2) if kind == "loud_dc" else (-0.6, 0.1)
    _ro(wav)
    return dict(wav=wav, origin=origin, first_chunk=first_chunk, hop=hop, L=L, chunks=chunks, w=w, b=b)


@functools.lru_cache(maxsize=4)
def chunk_reference(layout, L, kind):
    """-> (xn [chunks][80000], ac [chunks][2], bound of xn[:, :L], bound of a, bound of c)"""
    o = chunk_operands(layout, L, kind)
    xn, ac, p = R.chunk_norm_ref(parts=True, **o)
    bx, ba, bc = R.chunk_norm_bound(p, o["w"], o["b"])
    _ro(xn, ac, bx, ba, bc)
    return xn, ac, bx, ba, bc


# ---------------------------------------------------------------- classifier
CLS_CASES = [(1, 1), (1, 293), (3, 171), (7, 30)]          # (chunks, F): chunks * 293 = 293, 879 and 2051 are no multiples of the 256 threads


@functools.lru_cache(maxsize=None)
def cls_operands(chunks, F):
    rng = np.random.default_rng(100 * chunks + F)
    y = rng.standard_normal((chunks * F, 128)).astype(np.float32)
    y[y < 0] *= np.float32(0.01)                            # what the leaky ReLU of linear.1 leaves
    W = (0.3 * rng.standard_normal((3, 128))).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    _ro(y, W, b)
    return dict(y=y, W=W, b=b, chunks=chunks, F=F)


@functools.lru_cache(maxsize=None)
def cls_reference(chunks, F):
    seg, S = R.classifier_ref(parts=True, **cls_operands(chunks, F))
    bound = R.classifier_bound(seg, S)
    _ro(seg, bound)
    return seg, bound
