"""CPU side of tests/test_input_kernels.py: the fmaf that tests/input_ref.py writes in numpy equals the C library's, the references agree with what the
project already pins on the CPU (oracle/resample_oracle.py, the host packer sd_test_pack_split_weights), and each of the single mistakes of
input_ref.MISTAKES, planted in a reference, changes at least one byte of at least one case of tests/input_cases.py -- the cases the GPU file runs and
compares byte for byte over the whole returned buffers.  A planted result that is not finite, or that reaches into a canary, differs in its bytes too."""
import ctypes as C

import numpy as np
import pytest

import input_cases as K
import input_ref as R
import sdhip
from oracle import resample_oracle as ro


# ---------------------------------------------------------------- fmaf
def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_fma32_is_the_c_librarys_on_random_triples():
    """120 000 triples: exponents of a * b and c drawn apart by -30 .. 30 binades, so that sums cancel, absorb and straddle; all normal"""
    g = np.random.default_rng(3)
    n = 120000
    a = (g.standard_normal(n) * np.exp2(g.integers(-20, 20, n))).astype(np.float32)
    b = (g.standard_normal(n) * np.exp2(g.integers(-20, 20, n))).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * np.exp2(g.integers(-30, 30, n).astype(np.float64)) * (1 + g.standard_normal(n))).astype(np.float32)
    c[::5] = (-(a.astype(np.float64) * b))[::5].astype(np.float32)                # near-total cancellation
    c[1::7] = 0.0
    assert np.array_equal(_bits(R.fma32(a, b, c)), _bits(R.c_fmaf(a, b, c)))


def constructed_triples():
    """a * b = -+2^-24 (1 - 2^-46) beside c = 1 + 2^-23: the exact sum lies 2^-70 off the midpoint of two float32, the float64 sum ON it, and the
    float32 on the other side is the even one -- in every binade and with every sign."""
    one = np.float32(1) + np.float32(2.0 ** -23)
    out = []
    for e in (-40, -7, 0, 1, 30):
        for sa in (1.0, -1.0):
            for sc in (1.0, -1.0):
                out.append((np.float32(sa * float(one)), np.float32(2.0 ** (e - 24) * (1 - 2.0 ** -23)), np.float32(sc * float(one) * 2.0 ** e)))
    return [np.array(v, np.float32) for v in zip(*out)]


def test_fma32_is_the_c_librarys_where_rounding_twice_is_not():
    a, b, c = constructed_triples()
    ref = R.c_fmaf(a, b, c)
    naive = R.fma32(a, b, c, naive=True)
    wrong = _bits(naive) != _bits(ref)
    assert wrong.sum() >= 4, "no triple on which float64-then-round differs from fmaf: the correction would be untested"
    assert np.array_equal(_bits(R.fma32(a, b, c)), _bits(ref))
    # ... and the sum acc0 + acc1, which goes through the same routine, is the C float addition
    g = np.random.default_rng(4)
    p = (g.standard_normal(50000) * np.exp2(g.integers(-30, 30, 50000))).astype(np.float32)
    q = (g.standard_normal(50000) * np.exp2(g.integers(-30, 30, 50000))).astype(np.float32)
    assert np.array_equal(_bits(R.fma32(p, np.ones_like(p), q)), _bits(p + q))


# ---------------------------------------------------------------- the resampler's references against the oracle
@pytest.mark.parametrize("sr", [8000, 11025, 44100, 48000])
def test_restated_host_table_is_the_oracles_to_half_an_ulp(sr):
    """the loop of resample_taps restated (the double expressions in its order) against resample_oracle.h: the bound the GPU test holds the device's table to"""
    from math import sin, sqrt, pi
    L, M, fc, half, J = ro.plan(sr, 16000)
    i0b = float(np.i0(ro.BETA))
    h64, inside = R.tap_table_ref(sr)
    tab = np.zeros((2 * J + 1, L), np.float32)
    for jj in range(2 * J + 1):
        for ph in range(0, L, max(L // 16, 1)):
            u = float(ph) + float(jj - J) * float(L)
            if abs(u) <= half:
                a, r = 2.0 * fc * u, u / half
                sinc = 1.0 if a == 0.0 else sin(pi * a) / (pi * a)
                tab[jj, ph] = np.float32(L * 2.0 * fc * sinc * float(np.i0(ro.BETA * sqrt(max(1.0 - r * r, 0.0)))) / i0b)
    sub = (slice(None), slice(0, L, max(L // 16, 1)))
    assert (np.abs(tab[sub] - h64[sub]) <= 2.0 ** -24 * np.abs(h64[sub]) * (1 + 2.0 ** -20)).all()
    assert (tab[sub][~inside[sub]] == 0).all() and not inside[2 * J].any()       # row j = +J lies outside the window at every phase


@pytest.mark.parametrize("name", [n for n in K.ORACLE if not n.startswith(("67", "68", "168"))])
def test_exact_reference_is_inside_the_oracles_bound(name):
    y = K.resample_expected(name)[:-K.SLACK].astype(np.float64)
    y64, bound = K.oracle_expected(name)
    assert len(y) == len(y64) and (np.abs(y - y64) <= bound).all() and np.abs(y64).max() > 0.1


@pytest.mark.parametrize("name", list(K.IMPULSES))
def test_impulse_expectation_is_the_exact_reference(name):
    x, sr = K.impulse_signal(name)
    no = ro.out_len(len(x), sr, 16000)
    exp = R.impulse_expected(len(x), sr, K.IMPULSES[name][2], K.cpu_table(sr), no)
    assert np.array_equal(_bits(exp + np.float32(0)), _bits(R.resample_ref(x, sr, no, K.cpu_table(sr), K.FCANARY)[:no] + np.float32(0)))
    assert np.count_nonzero(exp) > 100


def test_resampler_cases_hold_what_they_claim():
    for name, (sr, n, n_out) in K.RESAMPLE.items():
        assert sdhip.lib().sd_resample_len(n, sr, 16000) == ro.out_len(n, sr, 16000)
    assert [K.resample_case("%d_out%d" % (sr, no))[3] for sr in K.SMALL_RATES for no in (1, 255, 256, 257, 773)] == [1, 255, 256, 257, 773] * 5
    span = lambda sr: (255 * R.plan(sr)[1]) // R.plan(sr)[0] + 2 * R.plan(sr)[2] + 3
    assert span(672000) * 4 == 65492 and span(672000) * 4 <= 65536 < (span(672000) + 256) * 4
    assert span(688000) * 4 > 65536
    assert span(1680000) * 4 == 163704 and (span(1680000) + 256) * 4 == 164728 > 160 * 1024 >= span(1680000) * 4
    rows = [r for name in K.JOBS for r in K.JOBS[name][0]]
    assert {r[6] for r in rows} >= {1, 255, 256, 257, 600} and {r[1] for r in rows} >= {0, 1, 512, 700} and {r[8] % 4 for r in rows} == {0, 1, 2, 3}
    assert any(r[2] > 0 for r in rows) and any(r[4] < r[2] + r[3] for r in rows) and any(r[5] % 256 for r in rows)
    assert {len(K.JOBS[n][0]) for n in K.JOBS} >= {1, 2, 9}


# ---------------------------------------------------------------- the weight forms against the host packer
@pytest.mark.parametrize("name", K.WEIGHTS)
def test_restated_split_form_is_the_host_packers_bytes(name):
    w, cin = K.weight_case(name)
    Kt, Cout, CinPad = w.shape
    out = np.zeros(2 * Kt * Cout * CinPad, np.uint16)
    inv = C.c_float(0.0)
    assert sdhip.lib().sd_test_pack_split_weights(w.ctypes.data_as(C.c_void_p), Kt, Cout, CinPad, cin, out.ctypes.data_as(C.c_void_p), C.byref(inv)) == 0
    h, my_inv = K.split_expected(name)
    assert h[:-K.SLACK].tobytes() == out.tobytes() and np.float32(inv.value) == my_inv


def test_truncation_differs_from_rounding_only_where_it_should():
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -12, -1.0 - 3 * 2.0 ** -12, 65520.0, 1e-30], np.float32)
    assert R.to_half(v).tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -10, -1.0 - 2.0 ** -10]      # a tie to even, then three quarters of a step
    assert R.to_half(v, "truncated").tolist()[:4] == [1.0, 1.0, 1.0, -1.0]
    assert np.isinf(R.to_half(v)[4]) and R.to_half(v, "truncated")[4] == 65504.0 and R.to_half(v)[5] == 0


# ---------------------------------------------------------------- every mistake shows
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_a_mistake_changes_a_byte_of_a_case(mistake):
    shown = []
    for fam in K.SHOWN_BY[mistake]:
        names, expected = K.FAMILIES[fam]
        shown += ["%s/%s" % (fam, n) for n in names if np.asarray(expected(n)).tobytes() != np.asarray(expected(n, mistake)).tobytes()]
    print("%-22s changes %d cases: %s" % (mistake, len(shown), " ".join(shown)))
    assert shown, "%s changes no byte of any case of %s" % (mistake, K.SHOWN_BY[mistake])


def test_every_mistake_is_listed():
    assert set(K.SHOWN_BY) == set(R.MISTAKES) and len(R.MISTAKES) == 18
