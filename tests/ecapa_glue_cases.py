"""The cases of tests/test_ecapa_glue.py and their operands, in one place: the GPU tests run them, tests/test_ecapa_glue_ref.py shows on the CPU that
each case's tolerance tells the mutants of tests/ecapa_glue_ref.py from the reference.  Operands and references are computed once per case and
shared read-only.  fp16 cases hold operands that are fp16 numbers already, so the reference sees what the kernel sees."""
import functools

import numpy as np

import ecapa_glue_ref as R

CANARY = -7776.0                           # (an fp16 number)
MARGIN = (65, 49, 28, 0)                   # the frames the four row spaces store beyond nvalid (csrc/ecapa.hip)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _h(a, f16):
    """float32 operands; for an fp16 case rounded to fp16 first"""
    a = a.astype(np.float32)
    return a.astype(np.float16).astype(np.float32) if f16 else a


# ---------------------------------------------------------------- per-item statistics: k_masked_mean, k_asp_stats, k_asp_pool
NV_ALL = [5, 64, 1, 501, 9, 3, 63, 436, 2, 8, 65, 4, 7, 6]        # every length of the 4-unrolled loop's tail, both sides of 64, the long ones
ITEM_SETS = {"one": [65], "three": [4, 501, 1], "all": NV_ALL}
STORE_MARGIN = (0, 28, 49)                 # item i stores min(501, nvalid + STORE_MARGIN[i % 3]) rows; those at and beyond nvalid hold NaN
# (C, ld - C, items, row_base): the product's 1024 and 3072, and 300 for the ch >= C guard of the second 256-thread block
STAT_SHAPES = [(1024, 0, "all", 0), (3072, 8, "all", 777), (300, 0, "three", 0), (300, 8, "one", 40), (1024, 8, "three", 1000), (3072, 0, "one", 0)]
STAT_DATA = ["unit", "cancel", "const", "outlier"]
LOGITS = ["n1", "n30", "asc", "desc", "const", "spike200", "jump100"]
# (C, pad, items, row_base, data, logits, f16)
STAT_CASES = [s + ("unit", None, f) for s in STAT_SHAPES for f in (0, 1)] + [(300, 8, "all", 40, d, None, f) for d in STAT_DATA[1:] for f in (0, 1)]
POOL_CASES = ([s + ("unit", "n1", f) for s in STAT_SHAPES for f in (0, 1)] + [(300, 8, "all", 40, "unit", l, 0) for l in LOGITS[1:]] +
              [(300, 8, "all", 40, "unit", "n30", 1)] + [(300, 8, "all", 40, d, "n1", 0) for d in STAT_DATA[1:]])


@functools.lru_cache(maxsize=None)
def stat_operands(C, pad, items, base, data, logits, f16):
    """-> dict(x, nvalid, rowoff, C_, logits).  unit: N(0, 1); cancel: 1e3 + 1e-2 N (fp16: the constant 1000); const: even channels one constant each (every
    fourth channel 0: there every step of a one-pass update is exact whatever the weights), odd channels N(0, 1); outlier: N(0, 1) with one frame of 1e4 per channel.
    logits, f32 in either mode: n1 N(0, 1); n30 30 N(0, 1) (DESIGN: real logits reach |30|); asc / desc strictly monotonic (a rescale at every frame /
    never one); const one value per channel; spike200 one frame 200 above N(0, 1); jump100 every other frame 105 .. 130 above its neighbours"""
    nv = np.array(ITEM_SETS[items], np.int32)
    n = len(nv)
    rng = np.random.default_rng([C, pad, n, base, STAT_DATA.index(data), LOGITS.index(logits) if logits else 99, f16])
    stored = np.minimum(501, nv + np.array(STORE_MARGIN)[np.arange(n) % 3])
    rowoff = (base + np.concatenate([[0], np.cumsum(stored)])).astype(np.int32)
    rows, ld = int(stored.sum()), C + pad
    x = np.full((rows, ld), np.nan, np.float32)
    lg = np.full((rows, ld), np.nan, np.float32) if logits else None
    for i in range(n):
        r0, k = rowoff[i] - base, int(nv[i])
        v = rng.standard_normal((k, C))
        if data == "cancel":
            v = 1e3 + 1e-2 * v
        elif data == "const":
            v[:, ::2] = rng.uniform(-2, 2, (1, (C + 1) // 2))
            v[:, ::4] = 0.0
        elif data == "outlier":
            v[rng.integers(0, k, C), np.arange(C)] = 1e4
        x[r0:r0 + k, :C] = _h(v, f16)
        if logits:
            g = rng.standard_normal((k, C))
            if logits == "n30":
                g *= 30.0
            elif logits in ("asc", "desc"):
                g = np.cumsum(rng.uniform(0.002, 0.06, (k, C)), 0) * (1 if logits == "asc" else -1) + 3.0 * rng.standard_normal((1, C))
            elif logits == "const":
                g = np.tile(3.0 * rng.standard_normal((1, C)), (k, 1))
            elif logits == "spike200":
                g[rng.integers(0, k, C), np.arange(C)] += 200.0
            elif logits == "jump100":
                g += ((np.arange(k)[:, None] + rng.integers(0, 2, (1, C))) % 2) * rng.uniform(105.0, 130.0, (k, C))
            lg[r0:r0 + k, :C] = g.astype(np.float32)
    if logits in ("asc", "desc"):                           # (strict in float32 too)
        for i in range(n):
            seg = lg[rowoff[i] - base:rowoff[i] - base + nv[i], :C]
            assert (np.diff(seg, axis=0) > 0).all() if logits == "asc" else (np.diff(seg, axis=0) < 0).all()
    _ro(x, lg, nv, rowoff)
    return dict(x=x, nvalid=nv, rowoff=rowoff, C_=C, logits=lg)


def _exact_std(o, C):
    """[items][C]: the column is one value over the item's valid frames (nvalid = 1 included): every d of the one-pass update is exactly 0, so the
    variance is exactly 0 and the std exactly sqrtf(1e-12f)"""
    base = o["rowoff"][0]
    return np.stack([(o["x"][r0:r0 + k, :C] == o["x"][r0, :C]).all(0) for r0, k in zip(o["rowoff"][:-1] - base, o["nvalid"])])


def stat_reference(kind, case, C=None):
    """-> (reference, tolerance) of kind "mean" [items][C], "stats" / "pool" [items][2 C], on the first C channels of the case (default: all; the CPU
    test takes a few: channels do not interact).  Tolerance 0 = the value must be exact"""
    o = stat_operands(*case)
    C = C or o["C_"]
    a = (o["x"], o["nvalid"], o["rowoff"], C)
    if kind == "mean":
        return R.masked_mean_ref(*a), R.masked_mean_bound(*a)
    if kind == "stats":
        ref, tol = R.asp_stats_ref(*a), R.asp_stats_bound(*a)
        ex = _exact_std(o, C)
        ref[:, C:][ex], tol[:, C:][ex] = R.STD_FLOOR_F32, 0.0
        return ref, tol
    return R.asp_pool_ref(o["x"], o["logits"], o["nvalid"], o["rowoff"], C), R.asp_pool_bound(o["x"], o["logits"], o["nvalid"], o["rowoff"], C)


@functools.lru_cache(maxsize=2)
def stat_reference_full(kind, case):
    ref, tol = stat_reference(kind, case)
    _ro(ref, tol)
    return ref, tol


# ---------------------------------------------------------------- k_se_apply
# pattern -> (os, rs, ys, shared, residual slice, output slice) in units of C: the first block reads its input from a buffer of its own in space 0 and
# writes slice 0 of `cat` (space 1, no output map); the later blocks read slice b - 1 and write slice b of `cat` through two maps
SE_PATTERNS = {"b0": (1, 0, 1, False, 0, 0), "b1": (2, 1, 1, True, 0, 1), "b2": (3, 1, 1, True, 1, 2)}
# (pattern, C, pad, items, f16); "limit": 4 095 items, the last with 501 rows in every space: item index 4 094, frame 500, last stored frame 500
SE_CASES = ([(p, C, pad, it, f) for p in SE_PATTERNS for (C, pad, it) in ((1024, 8, "three"), (64, 0, "all")) for f in (0, 1)] + [("b1", 8, 0, "limit", 0)])


def space_offsets(nv, limit=False):
    """prefix sums [4][items + 1] of the rows the four spaces store"""
    nv = np.asarray(nv, np.int64)
    rows = np.stack([np.full_like(nv, 2 if m > 28 else 1) if limit else np.minimum(501, nv + m) for m in MARGIN])
    if limit:                                              # (two rows per item in spaces 0 and 1, one in 2 and 3: the maps are no identities)
        rows[:, -1] = 501
    return np.concatenate([np.zeros((4, 1), np.int64), np.cumsum(rows, 1)], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def se_operands(pattern, C, pad, items, f16):
    """-> the keyword arguments of Diarizer.se_apply_case / ecapa_glue_ref.se_apply_ref.  Gates: item 0 all 0, item 1 all 1, item 2 U(0, 1), and so on
    in turn: every item differs from its neighbours.  The pad columns of t2 and of a residual buffer of its own hold NaN"""
    os_, rs, ys, shared, rsl, osl = SE_PATTERNS[pattern]
    limit = items == "limit"
    off = space_offsets(np.ones(4095) if limit else ITEM_SETS[items], limit)
    n = off.shape[1] - 1
    rng = np.random.default_rng([list(SE_PATTERNS).index(pattern), C, pad, n, f16])
    t2 = np.full((off[os_, -1], C + pad), np.nan, np.float32)
    t2[:, :C] = _h(rng.standard_normal((len(t2), C)), f16)
    res = np.full((off[rs, -1], C if shared else C + pad), np.nan, np.float32)
    res[:, :C] = _h(rng.standard_normal((len(res), C)), f16)
    gate = rng.uniform(0, 1, (n, C)).astype(np.float32)
    gate[0::3], gate[1::3] = 0.0, 1.0
    _ro(t2, res, gate, off)
    return dict(t2=t2, gate=gate, res=res, off=off, os=os_, rs=rs, ys=ys, shared=shared, y_ld=3 * C + pad, out_col0=osl * C, res_col0=rsl * C)


@functools.lru_cache(maxsize=2)
def se_reference(pattern, C, pad, items, f16):
    """-> (the [rows of space ys][y_ld] buffer as it must come back, tolerance: 0 where nothing may be written or the residual must stay, written mask)"""
    buf, written, mag = R.se_apply_ref(canary=CANARY, **se_operands(pattern, C, pad, items, f16))
    tol = R.se_apply_bound(buf, written, mag, f16)
    _ro(buf, tol, written)
    return buf, tol, written


# ---------------------------------------------------------------- k_build_rowtab
def _sums(rows, base):
    return (base + np.concatenate([[0], np.cumsum(rows)])).astype(np.int32)


def rowtab_cases():
    """name -> (off_out, off_in): same-space and cross-space tables, with and without items of a larger plan in front (bases > 0)"""
    nv = np.array(NV_ALL)
    sp = [np.minimum(501, nv + m) for m in MARGIN]
    return {"one item, same space": (_sums([37], 0), _sums([37], 0)),
            "one item, 501 of 501": (_sums([501], 0), _sums([501], 0)),
            "one item, cross space": (_sums([9], 0), _sums([74], 0)),
            "4095 items of one row": (_sums(np.ones(4095, int), 0), _sums(np.ones(4095, int), 0)),
            "1 row beside 501": (_sums([1, 501, 1], 0), _sums([1, 501, 66], 0)),
            "ragged, space 1 -> 0": (_sums(sp[1], 0), _sums(sp[0], 0)),
            "ragged, space 3 -> 1, bases > 0": (_sums(sp[3], 1234), _sums(sp[1], 5678)),
            "ragged, same space, base > 0": (_sums(sp[2], 99), _sums(sp[2], 99))}


# ---------------------------------------------------------------- k_scatter_emb, k_feats_to_half, k_rows_to_half
def scatter_cases():
    """name -> (emb_c [n_c][192], cidx [items]); 300 items = 57 600 elements: more than one block, not a multiple of 256"""
    rng = np.random.default_rng(192)
    out = {}
    for items in (5, 300):
        for name, live in (("none dropped", np.ones(items, bool)), ("all dropped", np.zeros(items, bool)), ("alternating", np.arange(items) % 2 == 0)):
            cidx = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
            out["%d items, %s" % (items, name)] = (rng.standard_normal((int(live.sum()), 192)).astype(np.float32), cidx)
    return out


def half_data(rows, width):
    """float32 values whose fp16 rounding is decided at the edges: ties (to even, both ways), fp16 subnormals and their ties, the largest finite fp16
    and the values beyond it, +-0, among values of every magnitude in between"""
    rng = np.random.default_rng(rows * 1000 + width)
    f = (rng.standard_normal((rows, width)) * np.exp(4.0 * rng.standard_normal((rows, width)))).astype(np.float32)
    edge = np.array([0.0, -0.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24,
                     -(2.0 ** -25), 2.0 ** -25 * (1 + 2.0 ** -20), 3e-6, 6.0e-5, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.996, 65520.0, -65520.0, 1e6, -3e38,
                     2049.0, 2051.0, 1e-30], np.float32)
    pos = rng.permutation(rows * width)[:len(edge) * 3]
    f.reshape(-1)[pos] = np.tile(edge, 3)[:len(pos)]
    f[0, :len(edge)] = edge
    return f
