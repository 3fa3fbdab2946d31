"""Every kernel in front of the two networks on its own -- k_resample, k_resample_jobs (resample.hip), k_tail_move, k_group_append (f32 and 16-bit),
k_group_scatter, k_group_tail_move (stream.hip), k_many_pack, k_many_gap_masks (many.hip), k_w16_planes, k_w_absmax, k_w16x (weights_gpu.hip) -- against
the references of tests/input_ref.py on the cases of tests/input_cases.py.

Diarizer.resample_case .. weight_forms_case (sd_test_* of include/sdhip_test.h, csrc/input_test.hip) make ONE launch through the function the product
calls, on operands with NaN (0x7fff for 16-bit samples) in 256 guard elements behind -- for the resampler also in front of -- every input, and a canary in
and 256 slack elements behind every output; the whole buffer comes back.  Wherever the reference is exact the comparison is byte equality over that whole
buffer, slack included, and a NaN anywhere fails it:
  the resampler     against input_ref.resample_exact on the tap table the context built, read back from the device; that table against the float64
                    oracle to half an ulp (values, not bits: outside the window the product stores +0.0 where the oracle's expression gives -0.0); whole
                    recordings also against resample_oracle.resample under the DERIVED bound (J + 4) 2^-24 sum |h x|; impulses against the table alone.
  copies, packs, masks   slicing.
  weight forms      numpy's round-to-nearest-even and, for the split form, the bytes of the host packer sd_test_pack_split_weights.  FINITE weights only:
                    what the two packers do with a NaN or an infinite weight (k_w_absmax skips it in the maximum) is not pinned here.
tests/test_input_ref.py shows on the CPU which case each of eighteen single mistakes changes.

At 1 680 000 Hz the span of a tile is 163 704 bytes, the largest resample_check accepts: k_resample takes it (a test of its own, one launch), and
resample_jobs, whose kernel holds a static kilobyte besides, refuses it before anything is launched.

Measured on the MI355X: the whole file, 137 tests, in 8.6 s, 1.9 s of it the context; the slowest tests are the three rates with thousands of taps
(2.6 s at 1 680 000 Hz, 1.0 s at 672 000 and 688 000 Hz: the numpy fmaf over 14 149 and 5 700 taps, not the launch), every other test below 0.2 s.  The
resampler's largest error against the float64 oracle was 5.3e-7 (48 000 Hz), the largest share of the derived bound 0.078 (16 001 Hz).  The first run failed in one place: the split
weight form of the all-zero layer, whose weights of -0.0 came back with a hi half of +0.0 and a lo half of -0.0 where the host packer has -0.0 and
+0.0 -- k_w16x's `(_Float16)(W * sc)` had been contracted into one fused multiply-add with a +0.0 addend; the kernel now takes hi's sign from W * sc."""
import ctypes as C

import numpy as np
import pytest

import input_cases as K
import input_ref as R
import sdhip

pytestmark = pytest.mark.gpu

SD_ERR_ARG = 1
FC = K.FCANARY


def same(what, got, exp):
    """byte equality of a whole returned buffer; no NaN anywhere"""
    got, exp = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
    assert got.dtype == exp.dtype and got.shape == exp.shape, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, exp.dtype, exp.shape)
    if got.dtype.kind == "f":
        assert not np.isnan(got).any(), "%s: NaN at %d" % (what, int(np.flatnonzero(np.isnan(got))[0]))
    if got.tobytes() == exp.tobytes():
        return
    raw = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(raw) != exp.view(raw))
    raise AssertionError("%s: %d of %d elements differ, first at %d (the slack begins at %d): got %r (bits %x), expected %r (bits %x)" % (
        what, len(bad), len(got), bad[0], len(exp) - K.SLACK, got[bad[0]], got.view(raw)[bad[0]], exp[bad[0]], exp.view(raw)[bad[0]]))


def refused(call):
    with pytest.raises(sdhip.SdError) as e:
        call()
    assert e.value.code == SD_ERR_ARG


_tables = {}


def table(d, sr):
    """the tap table the context built for sr -> 16 000 Hz, read back once (a call with no output launches nothing)"""
    if sr not in _tables:
        y, taps = d.resample_case(np.ones(1, np.float32), sr, n_out=0, canary=FC)
        assert (y == FC).all()
        taps.setflags(write=False)
        _tables[sr] = taps
    return _tables[sr]


# ---------------------------------------------------------------- resample.hip
@pytest.mark.parametrize("sr", K.RATES)
def test_tap_table_is_the_oracles_to_half_an_ulp(diarizer, sr):
    taps = table(diarizer, sr)
    h64, inside = R.tap_table_ref(sr)
    L, M, J = R.plan(sr)
    assert taps.shape == h64.shape == (2 * J + 1, L) and np.isfinite(taps).all()
    assert (np.abs(taps - h64) <= 2.0 ** -24 * np.abs(h64) * (1 + 2.0 ** -20)).all()
    assert (taps[~inside] == 0).all() and not inside[2 * J].any()


def check_oracle(name, y):
    y64, bound = K.oracle_expected(name)
    err = np.abs(y.astype(np.float64) - y64)
    print("%s: max error %.3g, %.3f of the bound" % (name, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert len(y) == len(y64) and (err <= bound).all()


@pytest.mark.parametrize("name", K.RESAMPLE_REST)
def test_resample(diarizer, name):
    x, sr, n_out, no = K.resample_case(name)
    y, _ = diarizer.resample_case(x, sr, n_out=n_out, want_taps=False, canary=FC)
    same("k_resample %s" % name, y, K.resample_expected(name, table(diarizer, sr)))
    if name in K.ORACLE:
        check_oracle(name, y[:no])


def test_resample_at_the_largest_span(diarizer):
    """1 680 000 Hz: 163 704 bytes of dynamic LDS, the most resample_check lets through; one launch"""
    name, = K.RESAMPLE_1680000
    x, sr, n_out, no = K.resample_case(name)
    y, taps = diarizer.resample_case(x, sr, n_out=n_out, canary=FC)
    _tables.setdefault(sr, taps)
    same("k_resample %s" % name, y, K.resample_expected(name, taps))
    check_oracle(name, y[:no])


@pytest.mark.parametrize("name", list(K.IMPULSES))
def test_resample_of_impulses_is_the_table(diarizer, name):
    x, sr = K.impulse_signal(name)
    y, _ = diarizer.resample_case(x, sr, want_taps=False, canary=FC)
    no = len(y) - K.SLACK
    exp = R.impulse_expected(len(x), sr, K.IMPULSES[name][2], table(diarizer, sr), no)
    assert (y[no:] == FC).all() and np.count_nonzero(exp) > 100
    assert np.array_equal(y[:no], exp) and not np.isnan(y).any()                     # values: amp * (+0.0) and a sum of zeros may differ in the sign of zero


def test_resample_refusals(diarizer):
    x = K.signal(100, 1)
    refused(lambda: diarizer.resample_case(x, 8000, n_out=201))                        # more than sd_resample_len
    refused(lambda: diarizer.resample_case(x, 0))
    refused(lambda: diarizer.resample_case(x, 1680001))                                # the span does not fit


@pytest.mark.parametrize("name", list(K.JOBS))
def test_resample_jobs(diarizer, name):
    rows, x, arena = K.jobs_case(name)
    tables = {r[0]: table(diarizer, r[0]) for r in rows}
    same("k_resample_jobs %s" % name, diarizer.resample_jobs_case(rows, x, arena, canary=FC), K.jobs_expected(name, tables))


def test_resample_jobs_refuses_a_span_that_leaves_no_room_for_its_outputs(diarizer):
    rows, x, arena = K.jobs_refused_case()
    out = diarizer.resample_jobs_case(rows, x, arena, canary=FC, refused=True)
    assert (out == FC).all()
    assert "LDS" in sdhip.lib().sd_last_error(diarizer._h).decode()


def test_resample_jobs_hook_refusals(diarizer):
    rows, x, arena = K.jobs_case("R2_mixed")
    in_sr, pad, first, held, n_limit, m_first, count, x_off, dst = rows[0]
    refused(lambda: diarizer.resample_jobs_case([(in_sr, pad, first + 8, held - 8, n_limit, m_first, count, x_off + 8, dst)], x, arena))      # sums in front of `first`
    refused(lambda: diarizer.resample_jobs_case([rows[0], rows[0]], x, arena))                                                               # one destination twice
    refused(lambda: diarizer.resample_jobs_case([(in_sr, pad, first, held, first + held + 1, m_first, count, x_off, dst)], x, arena))          # n_limit behind the inputs
    refused(lambda: diarizer.resample_jobs_case([(in_sr, pad, first, held, n_limit, m_first, count, x_off, arena - count)], x, arena))         # the pad leaves the arena


# ---------------------------------------------------------------- stream.hip
@pytest.mark.parametrize("name", K.GROUP)
@pytest.mark.parametrize("kind", list(K.KINDS))
def test_group_copy(diarizer, kind, name):
    which, src, rows, dst_len = K.group_case(kind, name)
    same("%s %s" % (kind, name), diarizer.group_copy_case(which, src, rows, dst_len, canary=FC), K.group_expected(kind, name))


@pytest.mark.parametrize("ln", K.TAIL_MOVE)
def test_tail_move(diarizer, ln):
    which, src, rows, dst_len = K.tail_move_case(ln)
    same("k_tail_move %d" % ln, diarizer.group_copy_case(which, src, rows, dst_len, canary=FC), K.tail_move_expected(ln))


def test_group_copy_refusals(diarizer):
    src = np.zeros(64, np.float32)
    refused(lambda: diarizer.group_copy_case(1, src, [(0, 0, 8, 8), (8, 7, 8, 8)], 32))          # destinations overlap
    refused(lambda: diarizer.group_copy_case(1, src, [(60, 0, 8, 8)], 32))                       # the source ends first
    refused(lambda: diarizer.group_copy_case(1, src, [(0, 30, 2, 8)], 32))                       # room leaves the arena
    refused(lambda: diarizer.group_copy_case(3, src, [(2, 0, 8, 600)], 700))                     # k_tail_move: a source that is not 16-byte aligned
    refused(lambda: diarizer.group_copy_case(3, src, [(0, 4, 8, 600)], 700))                     # ... a destination that is not the buffer's start
    refused(lambda: diarizer.group_copy_case(3, src, [(0, 0, 8, 519)], 700))                     # ... less room than len + 512
    refused(lambda: diarizer.group_copy_case(3, src, [(0, 0, 8, 520), (16, 600, 8, 520)], 2000))   # ... more than one row


# ---------------------------------------------------------------- many.hip
@pytest.mark.parametrize("name", K.PACK)
def test_many_pack(diarizer, name):
    src, rows, dst_len = K.pack_case(name)
    same("k_many_pack %s" % name, diarizer.many_pack_case(src, rows, dst_len, canary=FC), K.pack_expected(name))


def test_many_pack_refusals(diarizer):
    src = np.zeros(64, np.float32)
    refused(lambda: diarizer.many_pack_case(src, [(-1, 4, 0, 8)], 32))                           # a null source with samples to read
    refused(lambda: diarizer.many_pack_case(src, [(60, 8, 0, 8)], 32))
    refused(lambda: diarizer.many_pack_case(src, [(0, 4, 0, 8), (8, 4, 7, 8)], 32))              # destinations overlap


@pytest.mark.parametrize("name", list(K.GAPS))
def test_many_gap_masks(diarizer, name):
    gaps, total = K.GAPS[name]
    same("k_many_gap_masks %s" % name, diarizer.many_gap_masks_case(gaps, total, canary=FC), K.gaps_expected(name))


# ---------------------------------------------------------------- weights_gpu.hip
@pytest.mark.parametrize("name", K.WEIGHTS)
def test_weight_planes(diarizer, name):
    """k_w16_planes.  Finite weights only: the forms of non-finite weights are not pinned here."""
    w, cin = K.weight_case(name)
    h, inv = diarizer.weight_forms_case(w, cin, 0, canary=K.HCANARY)
    same("k_w16_planes %s" % name, h, K.planes_expected(name))
    assert inv == 0


@pytest.mark.parametrize("name", K.WEIGHTS)
def test_weight_split_form(diarizer, name):
    """k_w_absmax + k_w16x: the bytes and the inverse scale of the host packer, whose bits weights_gpu.hip's header claims, and of the layout formula
    restated in input_ref.w16x_ref.  Finite weights only: the forms of non-finite weights are not pinned here."""
    w, cin = K.weight_case(name)
    Kt, Cout, CinPad = w.shape
    h, inv = diarizer.weight_forms_case(w, cin, 1, canary=K.HCANARY)
    host = np.zeros(2 * Kt * Cout * CinPad, np.uint16)
    host_inv = C.c_float(0.0)
    assert sdhip.lib().sd_test_pack_split_weights(w.ctypes.data_as(C.c_void_p), Kt, Cout, CinPad, cin, host.ctypes.data_as(C.c_void_p), C.byref(host_inv)) == 0
    same("k_w16x %s against the host packer" % name, h, np.concatenate([host, np.full(K.SLACK, K.HCANARY, np.uint16)]))
    exp, exp_inv = K.split_expected(name)
    same("k_w16x %s against the restated layout" % name, h, exp)
    assert inv == np.float32(host_inv.value) == exp_inv


def test_weight_forms_refusals(diarizer):
    w = np.zeros((1, 2, 48), np.float32)
    refused(lambda: diarizer.weight_forms_case(w, 40, 1))                                        # CinPad % 32
    refused(lambda: diarizer.weight_forms_case(np.zeros((1, 2, 64), np.float32), 65, 0))         # cin > CinPad
