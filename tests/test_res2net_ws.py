"""The weight-stationary Res2Net kernel (conv_res2.hip, names res2ws_f32 / res2ws_f32_x2) against the 128 x 128 kernel it replaces and
against the float64 convolution.

Every case runs through sd_test_conv twice: with option conv_res2_ws = 1 (the kernel name must be res2ws_f32[_x2]) and = 0
(gemm128_f32[_x2]).  The two WHOLE output buffers -- guard columns, the 256 guard rows and, in the shared layout, the X and X2 slices
included -- must be equal bit for bit (random data).  The first run is also checked against the float64 reference with the bars of
tests/test_conv_kernels.py: exact data with zero tolerance, random data within the derived bound.

Row layout (layout()): the first 1024 rows are items of 8 / 9 rows placed so that the item boundaries of tiles 0 .. 7 fall in every
residue of a 128-row tile (asserted); row 1023 is an item of one row that ends on the last row of a tile, the next item starts on the
first row of a tile; then items of 1, 2, d and d + 1 rows (double reflection, "all taps read row 0"), three items with all Tin = 37
rows (the right-edge reflection is live), random items of 1 .. 37 rows, and a short item at the very end of the buffer.  Every item of
fewer than Tin rows stores fewer rows than Tin: a tap beyond its last stored frame reads that frame (dead-row skipping); the 256 rows
behind X / X2 hold NaN, so a read past an item -- at the end of the buffer above all -- shows as a NaN or a wrong value.

Measured on the MI355X: the buffers of the two kernels are equal in every case; res2ws_f32 max(error / bound) 0.006, res2ws_f32_x2 0.004
(K = 384 / 768: the bound grows with K, the error of a sum of random terms with its root).  16 tests in 3 s.
"""
import functools

import numpy as np
import pytest

from test_conv_kernels import CANARY, Case, check_exact, check_rand, run_case

pytestmark = pytest.mark.gpu

TIN = 37
OFF = {"conv_res2_ws": 1, "conv_res2_wgs": 0}


class res2_options:
    def __init__(self, d, **kw):
        self.d, self.kw = d, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.d.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.d.set_option(k, OFF[k])


class Recorder:
    """a Diarizer whose conv_case keeps the whole buffer of the last call"""

    def __init__(self, d):
        self.d, self.buf = d, None

    def conv_case(self, *a, **kw):
        self.buf, name = self.d.conv_case(*a, **kw)
        return self.buf, name


@functools.lru_cache(maxsize=None)
def layout(M, d):
    b = {0, M}
    for k in range(8):
        b.update(128 * k + k + 8 * j for j in range(16))
    assert {x % 128 for x in b if x < 1024} == set(range(128))        # every residue of a tile
    assert 1023 in b
    pos = 1024
    b.add(pos)
    rng = np.random.default_rng(M + d)
    for n in (1, 2, d, d + 1, TIN, TIN, TIN):
        pos += n
        b.add(pos)
    while pos < M - 5 - TIN:
        pos += int(rng.integers(1, TIN + 1))
        b.add(pos)
    while M - 5 - pos > TIN:
        pos += TIN
        b.add(pos)
    b.add(M - 5)                         # the last item: 5 of Tin rows stored, at the very end of the buffer
    e = np.array(sorted(b))
    n = tuple(int(v) for v in np.diff(e))
    assert sum(n) == M and min(n) >= 1 and max(n) <= TIN and n[-1] == 5
    return n


def res2_case(M, d, x2, **kw):
    return Case(n_out=layout(M, d), tin=TIN, cin=128, cout=128, kt=3, dil=d, prec=0, x2=x2, **kw)


def both(d, c, ws_name, **opts):
    """the case on the new kernel (checked against float64) and on the 128 x 128 kernel: same bits in the whole buffer"""
    g_name = "gemm128_f32_x2" if c.x2 else "gemm128_f32"
    rec = Recorder(d)
    with res2_options(d, conv_res2_ws=1, **opts):
        check_exact(rec, c, ws_name)
        check_rand(rec, c, ws_name)
    new = rec.buf
    with res2_options(d, conv_res2_ws=0):
        _, _, _, name = run_case(rec, c, "rand")
    assert name == g_name, (name, g_name)
    bad = ~((new == rec.buf) | (np.isnan(new) & np.isnan(rec.buf)))
    assert not bad.any(), "%s and %s differ in %d elements of the buffer; first at (row, column) %s: %r against %r" % (
        ws_name, g_name, bad.sum(), tuple(np.argwhere(bad)[0]), new[tuple(np.argwhere(bad)[0])], rec.buf[tuple(np.argwhere(bad)[0])])
    return new


def ws_name(x2):
    return "res2ws_f32_x2" if x2 else "res2ws_f32"


@pytest.mark.parametrize("x2", [False, True])
@pytest.mark.parametrize("dil", [2, 3, 4])
def test_dilations_with_and_without_the_second_input(diarizer, dil, x2):
    both(diarizer, res2_case(2049, dil, x2), ws_name(x2))


@pytest.mark.parametrize("M", [2048, 2048 + 127])
def test_last_tile_full_and_one_row_short(diarizer, M):
    """(the last tile with ONE row is M = 2049, the case of every other test here)"""
    both(diarizer, res2_case(M, 3, True), ws_name(True))


def test_slices_of_one_buffer(diarizer):
    """ecapa.hip's ec_tr: X, X2 and Y are column slices of one row, Y directly right of X2, canaries on both sides and between"""
    c = res2_case(2049, 2, True, shared=True, x_col0=8, x2_col0=8 + 128 + 16, y_col0=8 + 128 + 16 + 128, y_ld=8 + 128 + 16 + 128 + 128 + 24)
    both(diarizer, c, ws_name(True))


@pytest.mark.parametrize("epi", ["no_bn", "no_bias"])
def test_epilogues_the_rule_admits(diarizer, epi):
    """(ReLU with BN is the case of every other test here)"""
    kw = {"no_bn": dict(bn=False), "no_bias": dict(bias=False)}[epi]
    both(diarizer, res2_case(2049, 4, epi == "no_bn", **kw), ws_name(epi == "no_bn"))


@pytest.mark.parametrize("why", ["rows", "taps", "act2", "item_bias"])
def test_refused_cases_are_served_by_the_128_tile(diarizer, why):
    if why == "rows":
        c = res2_case(2047, 3, True)
    elif why == "taps":
        c = Case(n_out=layout(2049, 3), tin=TIN, cin=128, cout=128, kt=5, dil=3, prec=0, x2=True)
    else:
        c = res2_case(2049, 3, True, **({"act2": 1} if why == "act2" else {"item_bias": True}))
    with res2_options(diarizer, conv_res2_ws=1):
        if why != "act2":                # (exact data runs without a second activation: that case is not refused)
            check_exact(diarizer, c, "gemm128_f32_x2")
        check_rand(diarizer, c, "gemm128_f32_x2")


def test_bits_do_not_depend_on_the_grid(diarizer):
    """17 tiles on 256 workgroups (one each), on 16 (one workgroup takes two), on 3 (six tiles each, both panels in turn) and on 1"""
    c = res2_case(2049, 4, True)
    base = both(diarizer, c, ws_name(True))
    rec = Recorder(diarizer)
    for wgs in (16, 3, 1):
        with res2_options(diarizer, conv_res2_wgs=wgs):
            _, _, _, name = run_case(rec, c, "rand")
        assert name == ws_name(True)
        assert np.array_equal(base, rec.buf, equal_nan=True), wgs
