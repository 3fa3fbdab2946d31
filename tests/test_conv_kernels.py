"""Every conv_gemm kernel on its own against the float64 convolution of tests/conv_ref.py.

Diarizer.conv_case (sd_test_conv, include/sdhip_test.h) runs ONE conv case through the product's dispatch and reports which kernel
ran; every case asserts the kernel it means to test.  Each case is compared twice.

(a) Exact data, zero tolerance.  Activations are integers in -2 .. 2, weights in -3 .. 3 (about half of each zero), bias and per-item
bias small integers, the BN scale a power of two, the shift an integer, act1 none or relu, no act2.  Every product and every partial
sum is then an integer far below 2^24 (asserted on the reference), so f32 accumulation is exact in any order; fp16 holds the operands
exactly, and an fp16 output is exact while it is a multiple of its ulp within +-2048 (asserted).  In the split mode (x3) the weight
scale is a power of two and every lo half is zero.  All three precisions must therefore equal the float64 reference BIT FOR BIT: a
wrong tap, row, column, item boundary, clamp, reflection or a missing K-step shows as a mismatch, reported with (item, frame, column).

(b) Random data, a derived bound.  Operands are standard normal (rounded to fp16 for prec 1: the reference takes the operands as the
kernel sees them; in fp16 mode the sum X + X2 is itself an fp16 tensor, so the reference takes fp16(X + X2) there).  With exact
operands an f32 dot product of n terms summed in ANY order satisfies |acc - acc64| <= gamma_n S, gamma_n = n u / (1 - n u),
S = sum |x| |w| + |bias| + |item_bias| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  u = 2^-23 -- one ulp
rather than half, because the matrix pipe's internal additions are not promised to round to nearest -- and n = K_total + 3
(K_total = kt * cin, doubled with X2; + 3 for the bias, the scale and the shift).  x3: n = 3 K_total + 3 (three partial products per
term) plus 2^-21 S for the dropped lo * lo products and the rounding of the two splits.  Through the epilogue: times |scale|; relu,
leaky relu, tanh and sigmoid are 1-Lipschitz; + 4 ulp(f32) of |y| for tanhf / expf; + the rounding of the stored value, 2^-11 |y|
for an fp16 Y and 2^-24 |y| for an f32 Y.  (The f32 term is needed: S does not contain |shift|, so where the shift dominates a short
contraction even the correctly rounded f32 result is further from the float64 one than gamma S |scale| -- seen at K = 36, ratio 1.13.)
At these shapes gamma <= 1e-4 while one dropped term is about S / K_total >= 1e-3 S, so the bound separates right from wrong.
Each case prints max(error / bound).

Both kinds also assert that every guard element of the output buffer is untouched (canary columns left and right of the slice, 256
canary rows behind the last row) and that no output is NaN (the 256 rows behind the stored input hold NaN).

What the kernels define and the hook cannot express: SincNet's first layer reads overlapping rows (x_ld = 10 < Cin); the hook's rows
do not overlap, so the narrow kernel sees that layer's (kt, cin) with ordinary rows.  k_skinny_gemm splits K into four shares of
Kq = ceil(Cin / 4 / 8) * 8; dispatch only admits Cin % 32 == 0, for which the shares are always equal, so "unequal shares" cannot
occur -- the Cin values here cover the 32-wide main loop alone, the 8-wide remainder loop alone, and both.

Measured on the MI355X, max(error / bound) over the cases of each kernel (fp16 outputs sit just below 1 by construction: the bound is
then dominated by the half ulp of the fp16 store, which a correctly rounded result reaches):
    w256_f32 0.071   g256_f32 0.071   w256_x3 0.025   w256_f16 0.963   g256_m32 0.963   g256_m16 0.846   pp_relu 0.863   pp 0.892
    gemm128_f32 0.081 (_x2 0.035)   gemm128_f16 0.882 (_x2 0.859)   gemm128_x3 0.040 (_x2 0.012)   skinny 0.407   narrow2 0.006   narrow3 0.007
The exact-data comparisons hold bit for bit in all three precisions.  The whole file: 197 tests in 10 s, none above 1 s.
"""
import functools

import numpy as np
import pytest

import sdhip
from conv_ref import conv_ref

pytestmark = pytest.mark.gpu

CANARY = -7776.0            # exact in fp16
SLACK = sdhip.CONV_SLACK_ROWS
DEFAULTS = {"conv_pp": 1, "conv_glds": 1, "conv_mfma16": 1, "conv_h256": 1, "conv_w256_f32": 1, "conv_glds_f32": 0, "conv_rot": 3,
            "conv_stagger": 0, "conv_pn128": 0}
U = 2.0 ** -23


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


class options:
    """set test / tuning keys, restore the defaults on exit"""

    def __init__(self, d, **kw):
        self.d, self.kw = d, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.d.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.d.set_option(k, DEFAULTS[k])


# ---------------------------------------------------------------- row layouts
@functools.lru_cache(maxsize=None)
def ragged_rows(total, tin, tile=256, seed=0):
    """n_out per item, sum = total: several items of 1 - 5 rows (many items in one tile, every tap clamps), an item boundary exactly on
    the first tile edge, at least one item with all tin rows (the right-edge reflection is live), the rest random"""
    rng = np.random.default_rng(seed + 7 * tin + total)
    n = [1, 2, 3, 4, 5, 1, 5, 3]
    while sum(n) + tin <= tile and len(n) < 12:
        n.append(tin)
    while sum(n) < tile and total > tile:
        n.append(min(tin, tile - sum(n)))
    if total > tile:
        assert tile in np.cumsum(n)
    if sum(n) + tin <= total:
        n.append(tin)
    while sum(n) < total:
        n.append(int(min(total - sum(n), rng.integers(1, tin + 1))))
    while sum(n) > total:
        n.pop()
    if sum(n) < total:
        n.append(total - sum(n))
    assert sum(n) == total and max(n) <= tin and min(n) >= 1
    return tuple(n)


# ---------------------------------------------------------------- one case
class Case:
    """geometry + placement + epilogue of one conv case; data(kind) draws the operands, run() goes through the GPU, ref() through float64"""

    def __init__(self, *, n_out=None, n_in=None, tin=None, dense=None, cin, cout, kt=1, dil=1, pad_mode=0, prec=0, x2=False, bias=True, bn=True,
                 item_bias=False, act1=1, act2=0, y_f32=False, try_narrow=False, shared=False, x_ld=None, x_col0=0, x2_col0=0, y_ld=None, y_col0=0,
                 cin_pad=0, seed=1):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        if dense is not None:
            items, tp_in, tin_, tp_out, t = dense
            self.items, self.tin = items, tin_
            self.n_in, self.n_out = (tp_in,) * items, (tp_out,) * items
            self.n_valid = (t,) * items
        else:
            self.items = len(n_out)
            self.n_in = tuple(n_in) if n_in is not None else tuple(n_out)
            self.n_out = self.n_valid = tuple(n_out)
        self.M, self.in_rows = sum(self.n_out), sum(self.n_in)
        cpad = cin_pad or (-(-cin // 64) * 64 if prec == 1 else -(-cin // 32) * 32)
        self.cpad = cpad
        self.y_ld_ = y_ld if y_ld is not None else y_col0 + cout
        self.x_ld_ = x_ld if x_ld is not None else (self.y_ld_ if shared else x_col0 + cpad)
        self.k_total = kt * cin * (2 if x2 else 1)

    def key(self, kind):
        d = {k: v for k, v in self.__dict__.items() if k in ("n_out", "n_in", "tin", "dense", "cin", "cout", "kt", "dil", "pad_mode", "x2", "bias", "bn",
                                                              "item_bias", "act1", "act2", "seed")}
        return (kind, self.prec == 1 and kind == "rand") + tuple(sorted(d.items()))


@functools.lru_cache(maxsize=6)
def _data_and_ref(key):
    """operands and float64 reference of a case; computed once and shared (read-only) by every kernel that runs the same case"""
    c = _CASES[key]
    kind, half = key[0], key[1]
    rng = np.random.default_rng(c.seed)
    shp_x, shp_w = (c.in_rows, c.cin), (c.kt, c.cout, c.cin)
    if kind == "exact":
        def ints(lo, hi, shape):
            return (rng.integers(lo, hi + 1, shape) * (rng.random(shape) < 0.6)).astype(np.float32)
        x, w = ints(-2, 2, shp_x), ints(-3, 3, shp_w)
        x2 = ints(-2, 2, shp_x) if c.x2 else None
        bias = rng.integers(-3, 4, c.cout).astype(np.float32) if c.bias else None
        ib = rng.integers(-3, 4, (c.items, c.cout)).astype(np.float32) if c.item_bias else None
        scale = (2.0 ** rng.integers(-1, 2, c.cout)).astype(np.float32) if c.bn else None
        shift = rng.integers(-3, 4, c.cout).astype(np.float32) if c.bn else None
        act1, act2 = (c.act1 if c.act1 in (0, 1) else 0), 0
    else:
        rnd = (lambda s: f16(rng.standard_normal(s))) if half else (lambda s: rng.standard_normal(s).astype(np.float32))
        x, w = rnd(shp_x), rnd(shp_w)
        x2 = rnd(shp_x) if c.x2 else None
        fl = lambda s: rng.standard_normal(s).astype(np.float32)
        bias = fl(c.cout) if c.bias else None
        ib = fl((c.items, c.cout)) if c.item_bias else None
        scale, shift = (fl(c.cout), fl(c.cout)) if c.bn else (None, None)
        act1, act2 = c.act1, c.act2
    if c.dense is not None:                         # frames of the input beyond tin are never read: NaN says so
        xv = x.reshape(c.items, c.n_in[0], c.cin)
        xv[:, c.tin:] = np.nan
        if x2 is not None:
            x2.reshape(c.items, c.n_in[0], c.cin)[:, c.tin:] = np.nan
    rx, rx2 = x, x2
    if half and x2 is not None:                     # fp16 mode: X + X2 is an fp16 tensor
        rx, rx2 = f16(x + x2), None
    y, S, acc = conv_ref(rx, w, c.n_in, c.n_valid, c.tin, dil=c.dil, pad_mode=c.pad_mode, x2=rx2, bias=bias, scale=scale, shift=shift, item_bias=ib,
                         act1=act1, act2=act2)
    if kind == "exact":
        assert np.abs(S).max() < 2.0 ** 24           # every partial sum is an exact f32 integer (x3: times the weights' power of two)
    if c.dense is not None and c.n_valid != c.n_out:        # rows T <= t < Tp of the output: the kernels store zeros there (conv_gemm.hip, tile_out: live ? v : 0)
        def widen(a):
            full = np.zeros((c.items, c.n_out[0], c.cout))
            full[:, :c.n_valid[0]] = a.reshape(c.items, c.n_valid[0], c.cout)
            return full.reshape(-1, c.cout)
        y, S = widen(y), widen(S)
    ops = dict(w=w, x=x, x2=x2, bias=bias, scale=scale, shift=shift, item_bias=ib, act1=act1, act2=act2)
    for a in (x, w, x2, bias, ib, scale, shift, y, S):
        if a is not None:
            a.setflags(write=False)
    return ops, y, S


_CASES = {}


def case_data(c, kind):
    key = c.key(kind)
    _CASES[key] = c
    return _data_and_ref(key)


def run_case(d, c, kind):
    """-> (Y slice [M][cout] f32, reference y, S, kernel name); asserts the guards"""
    ops, y_ref, S = case_data(c, kind)
    buf, name = d.conv_case(ops["w"], ops["x"], n_in=None if c.dense is not None else c.n_in, n_out=None if c.dense is not None else c.n_out, tin=c.tin,
                            dense=c.dense, dil=c.dil, pad_mode=c.pad_mode, x2=ops["x2"], bias=ops["bias"], scale=ops["scale"], shift=ops["shift"],
                            item_bias=ops["item_bias"], act1=ops["act1"], act2=ops["act2"], prec=c.prec, y_f32=c.y_f32, try_narrow=c.try_narrow,
                            shared=c.shared, x_ld=c.x_ld, x_col0=c.x_col0, x2_col0=c.x2_col0, y_ld=c.y_ld, y_col0=c.y_col0, cin_pad=c.cin_pad, canary=CANARY)
    M = c.M
    assert buf.shape == (M + SLACK, c.y_ld_)
    # expected image of everything that is NOT the Y slice
    exp = np.full(buf.shape, CANARY, np.float32)
    if c.shared:
        for col0, src in ((c.x_col0, ops["x"]), (c.x2_col0, ops["x2"])):
            if src is None:
                continue
            exp[:M, col0:col0 + c.cpad] = 0.0
            exp[:M, col0:col0 + c.cin] = f16(src) if c.prec == 1 else src
            exp[M:, col0:col0 + c.cpad] = np.nan
    guard = np.ones(buf.shape, bool)
    guard[:M, c.y_col0:c.y_col0 + c.cout] = False
    bad = guard & ~((buf == exp) | (np.isnan(buf) & np.isnan(exp)))
    if bad.any():
        r, col = np.argwhere(bad)[0]
        raise AssertionError("%s: guard element (row %d%s, column %d; the slice is columns [%d, %d)) was overwritten: %r, %d elements in all"
                             % (name, r, " >= M = %d" % M if r >= M else "", col, c.y_col0, c.y_col0 + c.cout, buf[r, col], bad.sum()))
    y = buf[:M, c.y_col0:c.y_col0 + c.cout]
    assert not np.isnan(y).any(), "%s: NaN in the output (a row beyond the stored input was multiplied): first at %s" % (name, where(c, np.isnan(y)))
    return y, y_ref, S, name


def where(c, mask):
    g, col = np.argwhere(mask)[0]
    o0 = np.concatenate([[0], np.cumsum(c.n_out)])
    item = int(np.searchsorted(o0, g, side="right") - 1)
    return "row %d = (item %d of %d rows, frame %d), column %d" % (g, item, c.n_out[item], g - o0[item], col)


def check_exact(d, c, want):
    y, y_ref, S, name = run_case(d, c, "exact")
    assert name == want, "dispatch chose %s, the case targets %s" % (name, want)
    if c.prec == 1 and not c.y_f32:
        assert np.abs(y_ref).max() <= 2048 and np.array_equal(y_ref.astype(np.float16).astype(np.float64), y_ref)
    bad = y.astype(np.float64) != y_ref
    assert not bad.any(), "%s: %d of %d outputs differ from the exact reference; first at %s: got %r, expected %r" % (
        name, bad.sum(), bad.size, where(c, bad), y[tuple(np.argwhere(bad)[0])], y_ref[tuple(np.argwhere(bad)[0])])
    return y


RATIOS = {}


def check_rand(d, c, want):
    y, y_ref, S, name = run_case(d, c, "rand")
    assert name == want, "dispatch chose %s, the case targets %s" % (name, want)
    ops = case_data(c, "rand")[0]
    K = c.k_total
    n = (3 * K + 3) if c.prec == 3 else (K + 3)
    bound = (n * U / (1 - n * U)) * S
    if c.prec == 3:
        bound = bound + 2.0 ** -21 * S
    if ops["scale"] is not None:
        bound = bound * np.abs(ops["scale"].astype(np.float64))
    if ops["act2"]:
        bound = bound + 4 * 2.0 ** -23 * np.abs(y_ref)
    bound = bound + (2.0 ** -11 if c.prec == 1 and not c.y_f32 else 2.0 ** -24) * np.abs(y_ref)       # the stored value: nearest fp16 / f32
    err = np.abs(y.astype(np.float64) - y_ref)
    live = bound > 0                                 # (rows the kernel zero-fills have S = 0: they must be exactly 0)
    assert np.array_equal(y[~live], y_ref[~live].astype(np.float32))
    ratio = float((err[live] / bound[live]).max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("%-15s M=%-5d K=%-5d Cout=%-5d max(error / bound) = %.3f" % (name, c.M, K, c.cout, ratio))
    over = live & (err > bound)
    assert not over.any(), "%s: %d outputs beyond the bound (max error / bound = %.3f); first at %s" % (name, over.sum(), ratio, where(c, over))
    return y


# ---------------------------------------------------------------- wide kernels (256 x 256 tile, row table, M >= 2048)
# kernel -> (prec, option keys that select it, the (kt, dil, cin) it accepts here)
G_BASE = [(1, 1, 128), (3, 2, 64), (3, 4, 128), (5, 1, 128)]
G_LONG = [(1, 1, 256), (1, 1, 512), (1, 1, 1024)]
WIDE = {
    "w256_f32": (0, {}, G_BASE + [(1, 1, 1024)]),                                                   # shortest contraction 128
    "g256_f32": (0, {"conv_glds_f32": 1}, G_BASE + [(1, 1, 1024)]),
    "w256_x3": (3, {}, G_BASE + [(1, 1, 1024)]),
    "w256_f16": (1, {"conv_pp": 0, "conv_glds": 0}, [(3, 4, 128), (5, 1, 128)] + G_LONG),           # shortest contraction 256
    "g256_m32": (1, {"conv_pp": 0}, [(3, 4, 128), (5, 1, 128), (1, 1, 256), (1, 1, 512)]),          # below 1024: the 32x32x16 form
    "g256_m16": (1, {"conv_pp": 0}, [(1, 1, 1024), (3, 4, 384)]),                                   # from 1024 on: the 16x16x32 form
    "pp_relu": (1, {}, [(5, 1, 128), (1, 1, 512), (1, 1, 1024)]),                                   # shortest contraction 512
    "pp": (1, {}, [(5, 1, 128), (1, 1, 512), (1, 1, 1024)]),
}
COUTS = [256, 768, 1280]                 # one column tile; three; five = more than the widest super-block (two column groups)
ROWS = [(1, 37), (255, 501), (255, 37), (1, 501)]      # (r, tin): 2048 + r rows = 9 row panels, the last of them 1 / 255 rows


def wide_cases():
    """every (kernel, geometry it accepts, Cout); (r, tin) rotate with the geometry and Cout.  Ordered by shape, so that the kernels that run
    the same shape follow each other and share its reference"""
    allg = G_BASE + G_LONG + [(3, 4, 384)]
    out = []
    for gi, (kt, dil, cin) in enumerate(allg):
        for ci, cout in enumerate(COUTS):
            r, tin = ROWS[(gi + ci) % 4]
            for name, (prec, opts, geoms) in WIDE.items():
                if (kt, dil, cin) in geoms:
                    out.append(pytest.param(name, kt, dil, cin, cout, r, tin, id="%s-k%dd%dc%d-n%d-r%d-t%d" % (name, kt, dil, cin, cout, r, tin)))
    return out


def wide_case(name, kt, dil, cin, cout, r, tin):
    return Case(n_out=ragged_rows(2048 + r, tin), tin=tin, cin=cin, cout=cout, kt=kt, dil=dil, prec=WIDE[name][0], act1=0 if name == "pp" else 1)


@pytest.mark.parametrize("name,kt,dil,cin,cout,r,tin", wide_cases())
def test_wide_kernel(diarizer, name, kt, dil, cin, cout, r, tin):
    c = wide_case(name, kt, dil, cin, cout, r, tin)
    with options(diarizer, **WIDE[name][1]):
        check_exact(diarizer, c, name)
        check_rand(diarizer, c, name)


@pytest.mark.parametrize("name,prec,opts,kt,dil,cin,falls_to", [
    ("w256_f32", 0, {}, 3, 1, 32, "gemm128_f32"),                     # K = 96 < 128
    ("g256_f32", 0, {"conv_glds_f32": 1}, 3, 1, 32, "gemm128_f32"),
    ("w256_f16", 1, {"conv_pp": 0, "conv_glds": 0}, 3, 2, 64, "gemm128_f16"),      # K = 192 < 256
    ("g256", 1, {"conv_pp": 0}, 3, 2, 64, "gemm128_f16"),
    ("pp", 1, {}, 3, 4, 128, "g256_m32"),                             # K = 384 < 512: the LDS-DMA kernel, 32x32x16 form
    ("g256_m16", 1, {"conv_pp": 0}, 5, 1, 128, "g256_m32"),           # K = 640 < 1024
    ("w256 M", 0, {}, 1, 1, 128, "gemm128_f32"),                      # (rows below: 2047 < 8 row panels)
])
def test_contraction_just_below_a_kernels_limit_falls_to_the_next_kernel(diarizer, name, prec, opts, kt, dil, cin, falls_to):
    rows = 2047 if name == "w256 M" else 2049
    c = Case(n_out=ragged_rows(rows, 37), tin=37, cin=cin, cout=256, kt=kt, dil=dil, prec=prec)
    with options(diarizer, **opts):
        check_exact(diarizer, c, falls_to)
        check_rand(diarizer, c, falls_to)


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_kernel_cross_space_and_output_slice(diarizer, name):
    """n_out[i] < n_in[i] (in_rows != M, as tdnn2 and MFA run: the output space drops the receptive-field margin) and Y as a slice of a
    wider row with live canaries on both sides (column offsets and leading dimensions multiples of 8: what k_conv_gemm_pp demands)"""
    prec, opts, geoms = WIDE[name]
    kt, dil, cin = (3, 4, 384) if name == "g256_m16" else (5, 1, 128) if prec == 1 else (3, 4, 128)
    tin = 61
    n_out = ragged_rows(2048 + 77, 40)
    n_in = tuple(min(tin, n + 21) for n in n_out)
    c = Case(n_out=n_out, n_in=n_in, tin=tin, cin=cin, cout=512, kt=kt, dil=dil, prec=prec, act1=0 if name == "pp" else 1,
             x_col0=16, x_ld=16 + cin + 24, y_col0=8, y_ld=8 + 512 + 40)
    with options(diarizer, **opts):
        check_exact(diarizer, c, name)
        check_rand(diarizer, c, name)


# ---------------------------------------------------------------- variant equalities at odd shapes (random data)
def _bits(d, c, opts, want):
    with options(d, **opts):
        y, _, _, name = run_case(d, c, "rand")
    assert name == want, (name, want)
    return y


@pytest.mark.parametrize("cout,r,tin", [(256, 1, 37), (1280, 255, 501)])
def test_variants_claimed_identical_give_the_same_bits(diarizer, cout, r, tin):
    d = diarizer
    c16 = wide_case("pp_relu", 5, 1, 128, cout, r, tin)
    pp = _bits(d, c16, {}, "pp_relu")
    assert np.array_equal(pp, _bits(d, c16, {"conv_pp": 0, "conv_mfma16": 2}, "g256_m16"))
    m32 = _bits(d, c16, {"conv_pp": 0}, "g256_m32")
    assert np.array_equal(m32, _bits(d, c16, {"conv_pp": 0, "conv_glds": 0}, "w256_f16"))
    assert np.array_equal(m32, _bits(d, c16, {"conv_h256": 0}, "gemm128_f16"))
    for rot in (0, 1):
        assert np.array_equal(m32, _bits(d, c16, {"conv_pp": 0, "conv_rot": rot}, "g256_m32"))
    c32 = wide_case("w256_f32", 3, 4, 128, cout, r, tin)
    w = _bits(d, c32, {}, "w256_f32")
    assert np.array_equal(w, _bits(d, c32, {"conv_glds_f32": 1}, "g256_f32"))
    assert np.array_equal(w, _bits(d, c32, {"conv_w256_f32": 0}, "gemm128_f32"))
    for rot in (0, 1):
        assert np.array_equal(w, _bits(d, c32, {"conv_glds_f32": 1, "conv_rot": rot}, "g256_f32"))


# ---------------------------------------------------------------- 128 x 128 kernel
PREC_NAME = {0: "f32", 1: "f16", 3: "x3"}


def g128_name(prec, x2):
    return "gemm128_" + PREC_NAME[prec] + ("_x2" if x2 else "")


@pytest.mark.parametrize("prec", [0, 1, 3])
@pytest.mark.parametrize("M,cout,x2", [(1, 128, False), (127, 192, True), (129, 320, False), (300, 128, True), (300, 192, False), (129, 128, True),
                                       (127, 320, False), (1, 320, True)])
def test_gemm128(diarizer, prec, M, cout, x2):
    cin = 64 if prec == 1 else 32
    c = Case(n_out=ragged_rows(M, 37, tile=128), tin=37, cin=cin, cout=cout, kt=3, dil=2, prec=prec, x2=x2)
    check_exact(diarizer, c, g128_name(prec, x2))
    check_rand(diarizer, c, g128_name(prec, x2))


@pytest.mark.parametrize("prec", [0, 1, 3])
@pytest.mark.parametrize("epi", ["item_bias_tanh", "sigmoid", "leaky", "no_bias", "no_bn", "bare"])
def test_gemm128_epilogues(diarizer, prec, epi):
    kw = {"item_bias_tanh": dict(item_bias=True, act1=1, act2=1), "sigmoid": dict(act1=0, act2=2), "leaky": dict(act1=2),
          "no_bias": dict(bias=False, item_bias=True), "no_bn": dict(bn=False, act2=1), "bare": dict(bias=False, bn=False, act1=0)}[epi]
    cin = 64 if prec == 1 else 32
    c = Case(n_out=ragged_rows(300, 37, tile=128), tin=37, cin=cin, cout=192, kt=3, dil=3, prec=prec, x2=epi in ("item_bias_tanh", "no_bias"), **kw)
    name = g128_name(prec, c.x2)
    check_exact(diarizer, c, name)           # (exact data: relu / none only, see the module docstring; the optional terms are as in the case)
    check_rand(diarizer, c, name)


@pytest.mark.parametrize("prec", [0, 1, 3])
def test_gemm128_res2net_slices_of_one_buffer(diarizer, prec):
    """X, X2 and Y are column slices of one row (ecapa.hip's ec_tr): Y's slice directly right of X2's; canaries on both sides and between"""
    c = Case(n_out=ragged_rows(300, 37, tile=128), tin=37, cin=128, cout=128, kt=3, dil=2, prec=prec, x2=True, shared=True,
             x_col0=8, x2_col0=8 + 128 + 16, y_col0=8 + 128 + 16 + 128, y_ld=8 + 128 + 16 + 128 + 128 + 24)
    check_exact(diarizer, c, g128_name(prec, True))
    check_rand(diarizer, c, g128_name(prec, True))


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("cout", [128, 192])
def test_gemm128_dense_mapping_with_padding_rows(diarizer, prec, cout):
    """no row table: 3 items of Tp = 50 rows, T = 37 valid.  The kernels store ZEROS in the rows T <= t < Tp of the output (tile_out:
    live ? v : 0) -- asserted exactly; the input's padding rows hold NaN and are never read (reflection about Tin - 1)"""
    cin = 64 if prec == 1 else 32
    c = Case(dense=(3, 50, 37, 50, 37), cin=cin, cout=cout, kt=3, dil=2, prec=prec, act2=1)
    check_exact(diarizer, c, g128_name(prec, False))
    check_rand(diarizer, c, g128_name(prec, False))


def test_gemm128_schedule_options_give_the_same_bits(diarizer):
    c = Case(n_out=ragged_rows(300, 37, tile=128), tin=37, cin=32, cout=320, kt=3, dil=2, prec=0)
    base = _bits(diarizer, c, {}, "gemm128_f32")
    for opts in ({"conv_stagger": 1}, {"conv_stagger": 2}, {"conv_pn128": 2}, {"conv_pn128": 1}):
        assert np.array_equal(base, _bits(diarizer, c, opts, "gemm128_f32")), opts


# ---------------------------------------------------------------- skinny kernel
@pytest.mark.parametrize("M,cout,cin,act", [(1, 128, 128, "relu"), (31, 192, 1024, "sigmoid"), (33, 1024, 6144, "relu"), (100, 128, 6144, "sigmoid"),
                                            (100, 192, 32, "relu"), (33, 128, 96, "sigmoid"), (31, 1024, 160, "relu"), (1, 192, 100, "sigmoid"),
                                            (100, 1024, 36, "relu"), (1, 1024, 1024, "sigmoid")])
def test_skinny(diarizer, M, cout, cin, act):
    """Cin (padded to 32): 32 and 96 -> Kq = 8 / 24: the 8-wide loop alone; 128, 1024, 6144 -> the 32-wide loop alone; 160 -> Kq = 40: both;
    100 and 36 are padded to 128 / 64 by the weight builder"""
    kw = dict(act1=1) if act == "relu" else dict(act1=0, act2=2)
    c = Case(dense=(1, M, M, M, M), cin=cin, cout=cout, **kw)
    check_exact(diarizer, c, "skinny")
    check_rand(diarizer, c, "skinny")


# ---------------------------------------------------------------- narrow kernel (SincNet: "valid" padding, dense rows)
SINC = [(1, 251), (5, 80), (5, 60)]          # (kt, cin) of pyannet.hip's sinc0 / sinc1 / sinc2


def narrow_case(kt, cin, cout, M, **kw):
    items, t = (3, 43) if M == 129 else (1, M)
    tin = t + (kt - 1)
    kw.setdefault("bn", False)
    kw.setdefault("act1", 0)
    return Case(dense=(items, tin, tin, t, t), cin=cin, cout=cout, kt=kt, pad_mode=1, try_narrow=True, **kw)


@pytest.mark.parametrize("kt,cin", SINC)
@pytest.mark.parametrize("cout,M", [(60, 1), (80, 127), (60, 129), (80, 129), (80, 1), (60, 127)])
def test_narrow(diarizer, kt, cin, cout, M):
    c = narrow_case(kt, cin, cout, M)
    want = "narrow3" if cout > 64 else "narrow2"
    check_exact(diarizer, c, want)
    check_rand(diarizer, c, want)


@pytest.mark.parametrize("why,cout,kw", [("act1", 80, dict(act1=1)), ("cout", 100, {})])
def test_narrow_refuses_and_conv_gemm_serves_the_case(diarizer, why, cout, kw):
    c = narrow_case(5, 80, cout, 129, **kw)
    check_exact(diarizer, c, "gemm128_f32")
    check_rand(diarizer, c, "gemm128_f32")


# ---------------------------------------------------------------- contract edges (launch_conv_gemm's guards)
@pytest.mark.parametrize("prec,cin_pad", [(0, 48), (3, 80), (1, 96)])
def test_padded_channel_count_off_the_k_step_is_refused_and_nothing_is_launched(diarizer, prec, cin_pad):
    """documented precondition: Cin (padded) is a multiple of 32 (f32, x3) / 64 (fp16)"""
    c = Case(n_out=ragged_rows(129, 37, tile=128), tin=37, cin=40, cout=128, prec=prec, cin_pad=cin_pad)
    with pytest.raises(sdhip.SdError) as e:
        run_case(diarizer, c, "exact")
    assert e.value.code == 1 and e.value.kernel == "" and "not a multiple" in str(e.value)       # SD_ERR_ARG


# ---------------------------------------------------------------- the assembled network, frame by frame
def test_ecapa_mfa_every_valid_frame_against_float64_oracle(diarizer, weights):
    """test_ecapa_parity sees the pooled vector only.  Here the MFA output (ec_mfa: compact space 3, item i holds its nvalid_i frames,
    ld = 3072 + ecapa_ld_pad) is compared frame by frame with the float64 oracle.  Tolerance: the float32 torch oracle's own error against
    the float64 oracle on the same inputs, per-channel normalised, times 8 -- both are f32 evaluations of one graph in different
    summation orders; the margin covers the MFMA's grouping of K.  Measured on the MI355X: torch f32 2.066e-03, GPU 2.630e-04 (0.13 x the
float32 oracle's own error, limit 8 x)."""
    import torch
    from oracle import nn_oracle as nn
    rng = np.random.default_rng(3)
    feats = (3.0 * rng.standard_normal((6, 501, 80))).astype(np.float32)
    lens = np.array([1.0, 0.7311, 0.25, 0.5, 0.9991, 0.008], np.float32)
    diarizer.ecapa(feats, lens)
    nvalid = np.clip(np.ceil(lens * np.float32(501)), 1, 501).astype(np.int64)          # sd_ecapa's rule
    assert np.array_equal(nvalid, (torch.arange(501)[None, :] < (torch.from_numpy(lens) * 501)[:, None]).sum(1).numpy())      # = the oracle's mask
    ld = 3072
    got = diarizer.read_ws("ec_mfa", np.float32, int(nvalid.sum()) * ld).reshape(-1, ld)
    r64 = nn.EcapaOracle(weights[3], torch.float64)(feats, lens, return_intermediate=True)[1]["mfa"].numpy()       # [6][3072][501]
    r32 = nn.EcapaOracle(weights[3], torch.float32)(feats, lens, return_intermediate=True)[1]["mfa"].numpy().astype(np.float64)
    ref = np.concatenate([r64[i, :, :nvalid[i]].T for i in range(6)])
    o32 = np.concatenate([r32[i, :, :nvalid[i]].T for i in range(6)])
    norm = np.abs(ref).max(0)                          # per channel
    e32 = (np.abs(o32 - ref) / norm).max()
    eg = np.abs(got.astype(np.float64) - ref) / norm
    print("per-channel-normalised max error against the float64 oracle: torch f32 %.3e, GPU %.3e (%.2f x)" % (e32, eg.max(), eg.max() / e32))
    g, col = np.unravel_index(np.argmax(eg), eg.shape)
    o0 = np.concatenate([[0], np.cumsum(nvalid)])
    item = int(np.searchsorted(o0, g, side="right") - 1)
    assert eg.max() <= 8 * e32, "worst frame: item %d, frame %d, channel %d: GPU %r, float64 %r" % (item, g - o0[item], col, got[g, col], ref[g, col])
