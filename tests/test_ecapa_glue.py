"""Every kernel of csrc/ecapa.hip, each on its own, against the float64 references of tests/ecapa_glue_ref.py.

Diarizer.ecapa_stats_case / se_apply_case / rowtab_case / scatter_emb_case / to_half_case (sd_test_* of include/sdhip_test.h) launch ONE kernel through
the launcher run_ecapa_t uses, on operands the test chooses.  Every input is followed by NaN, every output buffer is filled with a canary and has 256
slack rows behind it; rows at and beyond nvalid and the pad columns of ld > C hold NaN.  Each test asserts that no guard element changed and that
every output is finite.  The cases and their operands live in tests/ecapa_glue_cases.py; tests/test_ecapa_glue_ref.py pins the references to the
torch formulas of oracle/nn_oracle.py and shows on the CPU that each tolerance below is at least ten times smaller than what a wrong divisor, frame,
clamp, eps, rescale, gate or row does.  fp16 cases hold fp16 numbers, so the reference sees what the kernel sees; the statistics kernels widen them
exactly and compute and store in f32, so their bounds are the f32 ones.

Every tolerance is a per-element bound computed from the float64 reference, with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1).  None is measured; no case needs the 8 e32 yardstick.

k_masked_mean.  Four partial sums of nv // 4 additions each, up to three more for the tail, two to join them, one division: every path from an
input to the result passes at most nv // 4 + 6 roundings:  gamma_(nv // 4 + 6) mean|x|.

k_asp_stats (one-pass update mean_k = mean_(k-1) + d_k / k, d_k = x_k - mean_(k-1); m2 += d_k (x_k - mean_k)).  An error e of mean_(k-1) reaches
mean_k as (1 - 1/k) e, so a local error made at step j arrives at step k multiplied by j / k.  The local errors are 3 u |d_j| / j (the subtraction
and the correctly rounded division, one u to spare) and u |mean_j| (the addition):
    E_k = (1 / k) sum_(j <= k) (3 u |d_j| + j u |mean_j|)            d_mean = E_nv + u |mean|
Every term of m2 is >= 0.  Its factors carry E_(k-1) and E_k, so it is off by |x_k - mean_k| E_(k-1) + |d_k| E_k + E_(k-1) E_k (on a mean of 1e3 the
product is no second-order term) + 3 u of itself; the sum adds gamma_(nv + 2), the division u:
    d_var = (1 / nv) sum_k (...) + (gamma_(nv + 2) + 4 u) var        d_std = d_var / (std + sqrt(max(max(var, eps) - d_var, eps))) + 2 u std
(|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b), both sides clamped at eps = 1e-12; sqrtf and nothing else: 2 u).  All running quantities are
the float64 ones.  A column that holds one value over the item's frames -- nvalid = 1 included -- has d_k = 0 exactly from the second frame on: its
std must be EXACTLY sqrtf(1e-12f) (tolerance 0).  On the "cancel" data (mean 1e3, deviation 1e-2) the bound is honest about what a one-pass update
in f32 can lose -- nv u |mean| / 2, the size of the deviation itself; the measured error of the std there is three orders below it (the roundings do not line up).

k_asp_pool (online softmax: running maximum mx, W = sum of exp(l - mx), rescaled by exp(mx_old - l) at a new maximum; weighted update
mean_k = mean_(k-1) + (w_k rcp(W_k)) d_k; m2 = s m2 + w_k d_k (x_k - mean_k); std = sqrt(max(m2 / W, eps))).  The same recurrence with r_k = w_k / W_k
in place of 1 / k: a local error of step j arrives at step k multiplied by W_j / W_k = P_j / P_k, P = the cumulative sums of the true softmax weights p.
  delta_w, the relative error of one weight: __expf(a) = v_exp_f32(a log2 e) with a = l - mx a rounded difference.  The subtraction, the product and
    the rounded constant each move the exponent by |a| u, so 3 |a| u; the instruction itself is ASSUMED good to 1 ulp = 2 u (the guides state no
    figure for v_exp_f32 or v_rcp_f32).  A weight below 2^-126 is flushed: 2^-126 / w more.
  S_k = the sum of (delta_w(mx_old - l) + u) over the rescales up to k: what the factors have cost every earlier weight.
  eW_k, the relative error of W_k: the share-weighted mean of (delta_w_j + S_k - S_j) over its components j <= k, + gamma_k for the additions.
  eps_k = delta_w_k + eW_k + 5 u: the ratio r_k (v_rcp_f32 ASSUMED 1 ulp = 2 u, the product u) times d_k (its subtraction u, the product u).
    E_k = (1 / P_k) sum_(j <= k) (p_j eps_j |d_j| + u P_j |mean_j|)  d_mean = E_nv + u |mean|
  i.e. the mean moves by sum p eps |d| -- twice delta_w times the weighted mean absolute deviation when delta_w dominates -- plus the accumulation
  term.  The variance as for k_asp_stats with weights p, each term's weight off by delta_w_k + (S_nv - S_k) + eW_nv + 4 u, the sum by gamma_(nv + 2).
  Constant logits give the k_asp_stats reference (asserted on the CPU); one frame 200 above the rest leaves the clamp's 1e-6 as the reference std,
  and the bound allows what mean = mean_old + 1.0 * (x - mean_old) loses there (sqrt(u |d| |x|)).  Exactness is demanded where it follows without
  assumptions about the two instructions: the all-zero columns of the "const" data (bound 2 u 1e-6 on the std, 0 on the mean).

k_se_apply.  2 u (|g a| + |r|): the product and the sum, or the single rounding of an FMA -- the bound covers the fused and the unfused form.  An fp16
store adds half an fp16 ulp of the stored value, max(2^-11 (|y| + the f32 bound), 2^-25).  Everything else is exact: every element of the shared
buffer outside the written slice, every row of the slice at a frame the output space does not hold, the slack rows, and the residual slice.

k_build_rowtab, k_scatter_emb, k_feats_to_half, k_rows_to_half: bit equality (numpy's float16 rounding for the last two).

Measured on the MI355X, max(error / tolerance) per kernel family (f32 / fp16 operands):
    k_masked_mean            0.365 / 0.409      (unit 0.37, cancel 0.27, const 0.32, outlier 0.41)
    k_asp_stats   mean       0.421 / 0.409      std  0.228 / 0.241      (std on the cancel data: 0.001; every exact std exact)
    k_asp_pool    mean       0.355 / 0.306      std  0.596 / 0.529      (worst: logits 30 N(0, 1); N(0, 1) 0.28 / 0.19, ascending 0.16 / 0.10,
                                                                         descending 0.18 / 0.10, constant 0.18 / 0.09, spike of 200 0.12 / 0.004,
                                                                         jumps of 105 .. 130 0.29 / 0.33, cancel 0.28 / 0.001, outlier 0.24 / 0.20)
    k_se_apply               0.500 / 0.999      (f32: the compiler fuses the product and the sum, one rounding of the two allowed; fp16: results within
                                                 a hair of a rounding tie of the fp16 store, which the half-ulp term allows in full)
    k_build_rowtab, k_scatter_emb, k_feats_to_half, k_rows_to_half: equal bit for bit in every case.
The whole file: 92 tests in 5.7 s (2.1 s of it the context every GPU test file opens), none above 0.5 s.
"""
import numpy as np
import pytest

import sdhip
import ecapa_glue_cases as K
import ecapa_glue_ref as R

pytestmark = pytest.mark.gpu

CANARY = np.float32(K.CANARY)
SLACK = sdhip.GLUE_SLACK_ROWS
SD_ERR_ARG = 1


def live_and_guard(buf, rows, what):
    """buf [rows + SLACK][w] -> buf[:rows]; the slack rows must hold the canary"""
    assert buf.shape[0] == rows + SLACK, (buf.shape, rows)
    bad = buf[rows:] != CANARY
    assert not bad.any(), "%s: %d guard elements behind the output were overwritten, first at row %d + %d" % (what, bad.sum(), rows, np.argwhere(bad)[0][0])
    return buf[:rows]


def report(what, err, tol):
    """print max(error / tolerance), assert it is <= 1; tol = 0 demands an exact value"""
    exact = tol == 0
    assert not err[exact].any(), "%s: %d values that must be exact are not, first at %s" % (what, np.count_nonzero(err[exact]), np.argwhere(exact & (err != 0))[0])
    q = err[~exact] / tol[~exact]
    ratio = float(q.max()) if q.size else 0.0
    print("RATIO %-70s max(error / tolerance) = %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: %d values beyond the tolerance, max(error / tolerance) = %.3f, first at %s" % (what, (q > 1).sum(), ratio, np.argwhere((err > tol) & ~exact)[0])
    return ratio


def _name(case):
    C, pad, items, base, data, logits, f16 = case
    return "C=%d ld=C+%d %s items row_base=%d %s%s %s" % (C, pad, items, base, data, " logits=" + logits if logits else "", "fp16" if f16 else "f32")


# ---------------------------------------------------------------- per-item statistics
def _stats(diarizer, kind, kernel, case):
    o = K.stat_operands(*case)
    ref, tol = K.stat_reference_full(kind, case)
    what = "%s %s" % (kernel, _name(case))
    y = live_and_guard(diarizer.ecapa_stats_case(kind, f16=bool(case[6]), canary=CANARY, **o), len(o["nvalid"]), what)
    assert np.isfinite(y).all(), "%s: %d outputs are not finite (a frame at or beyond nvalid, a pad column or a guard was read), first at %s" % (
        what, (~np.isfinite(y)).sum(), np.argwhere(~np.isfinite(y))[0])
    assert not (y == CANARY).any(), "%s: %d outputs were never written" % (what, (y == CANARY).sum())
    C = o["C_"]
    err = np.abs(y.astype(np.float64) - ref)
    if kind == "mean":
        return report(what, err, tol)
    report(what + " mean", err[:, :C], tol[:, :C])
    return report(what + " std", err[:, C:], tol[:, C:])


@pytest.mark.parametrize("case", K.STAT_CASES, ids=_name)
def test_masked_mean(diarizer, case):
    _stats(diarizer, "mean", "k_masked_mean", case)


@pytest.mark.parametrize("case", K.STAT_CASES, ids=_name)
def test_asp_stats(diarizer, case):
    _stats(diarizer, "stats", "k_asp_stats", case)
    if case[4] == "const" or 1 in K.ITEM_SETS[case[2]]:
        assert (K.stat_reference_full("stats", case)[1] == 0).any()         # (the case does demand exact values)


@pytest.mark.parametrize("case", K.POOL_CASES, ids=_name)
def test_asp_pool(diarizer, case):
    _stats(diarizer, "pool", "k_asp_pool", case)


def test_statistics_hook_refuses_reads_outside_the_operands(diarizer):
    o = K.stat_operands(300, 8, "one", 40, "unit", "n1", 0)
    for bad in (dict(nvalid=np.array([94], np.int32)), dict(nvalid=np.array([0], np.int32)), dict(C_=309)):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.ecapa_stats_case("pool", **{**o, **bad})
        assert e.value.code == SD_ERR_ARG
    with pytest.raises(sdhip.SdError) as e:                                 # k_asp_pool without logits
        diarizer.ecapa_stats_case("pool", **{**o, "logits": None})
    assert e.value.code == SD_ERR_ARG


# ---------------------------------------------------------------- k_se_apply
def _se_name(case):
    return "%s C=%d pad=%d %s %s" % (case[0], case[1], case[2], case[3], "fp16" if case[4] else "f32")


@pytest.mark.parametrize("case", K.SE_CASES, ids=_se_name)
def test_se_apply(diarizer, case):
    o = K.se_operands(*case)
    buf, tol, written = K.se_reference(*case)
    what = "k_se_apply " + _se_name(case)
    got = diarizer.se_apply_case(f16=bool(case[4]), canary=CANARY, **o)
    rows, C = buf.shape[0], o["gate"].shape[1]
    assert got.shape == (rows + SLACK, o["y_ld"])
    # behind the buffer: the canary, and -- shared -- the NaN behind the residual slice
    slack = got[rows:]
    res_cols = np.zeros(o["y_ld"], bool)
    if o["shared"]:
        res_cols[o["res_col0"]:o["res_col0"] + C] = True
    assert (slack[:, ~res_cols] == CANARY).all(), "%s: the slack rows behind the buffer were written" % what
    assert np.isnan(slack[:, res_cols]).all()
    y = got[:rows]
    assert np.isfinite(y).all(), "%s: %d values are not finite (a pad column or a guard was read), first at %s" % (what, (~np.isfinite(y)).sum(), np.argwhere(~np.isfinite(y))[0])
    # what must not be touched: the canary outside the slice and at the frames the output space does not hold, the residual slice
    keep = ~written
    moved = keep & (y != buf)
    assert not moved.any(), "%s: %d elements outside the defined output changed, first at (row, column) %s" % (what, moved.sum(), np.argwhere(moved)[0])
    assert not (y[written] == CANARY).any(), "%s: %d outputs were never written" % (what, (y[written] == CANARY).sum())
    report(what, np.abs(y.astype(np.float64) - buf), tol)


def test_se_apply_hook_refuses_rows_the_spaces_do_not_hold(diarizer):
    o = dict(K.se_operands("b1", 64, 0, "all", 0))
    off = o["off"].copy()
    off[1] = off[3]                                       # the residual's / output's space stores fewer frames than t2's
    with pytest.raises(sdhip.SdError) as e:
        diarizer.se_apply_case(**{**o, "off": off, "res": o["res"][:off[1, -1]]})
    assert e.value.code == SD_ERR_ARG
    with pytest.raises(sdhip.SdError) as e:               # overlapping slices
        diarizer.se_apply_case(**{**o, "out_col0": 32})
    assert e.value.code == SD_ERR_ARG


# ---------------------------------------------------------------- k_build_rowtab
@pytest.mark.parametrize("name", list(K.rowtab_cases()))
def test_build_rowtab(diarizer, name):
    off_out, off_in = K.rowtab_cases()[name]
    tab = diarizer.rowtab_case(off_out, off_in, canary=-7776)
    rows = int(off_out[-1] - off_out[0])
    assert tab.shape == (rows + sdhip.ROWTAB_SLACK, 2)
    assert (tab[rows:] == -7776).all(), "slack entries of the table were written"
    ref = R.rowtab_ref(off_out, off_in)
    assert np.array_equal(tab[:rows], ref), "first difference at row %s" % np.argwhere(tab[:rows] != ref)[0]
    print("RATIO k_build_rowtab %-50s %d rows, %d items: equal" % (name, rows, len(off_out) - 1))


# ---------------------------------------------------------------- k_scatter_emb, k_feats_to_half, k_rows_to_half
@pytest.mark.parametrize("name", list(K.scatter_cases()))
def test_scatter_emb(diarizer, name):
    emb_c, cidx = K.scatter_cases()[name]
    out = diarizer.scatter_emb_case(emb_c, cidx, canary=CANARY)
    y = live_and_guard(out, len(cidx), "k_scatter_emb " + name)
    assert np.array_equal(y.view(np.uint32), R.scatter_emb_ref(emb_c, cidx))
    print("RATIO k_scatter_emb %-50s bit-equal" % name)


@pytest.mark.parametrize("rows,width,feats", [(3, 96, True), (301, 96, True), (1, 24, False), (77, 1032, False), (300, 128, False)])
def test_to_half(diarizer, rows, width, feats):
    f = K.half_data(rows, width)
    h = diarizer.to_half_case(f, feats=feats, canary=CANARY)
    what = "%s rows=%d width=%d" % ("k_feats_to_half" if feats else "k_rows_to_half", rows, width)
    assert h.shape == (rows + SLACK, 128 if feats else width)
    assert (h[rows:] == np.float16(CANARY)).all(), "%s: guard rows written" % what
    ref = R.to_half_ref(f, feats)
    assert np.isinf(ref).any() and (ref == 0).any() and ((ref != 0) & (np.abs(ref) < 6.1e-5)).any()       # (the data reach the edges)
    diff = h[:rows].view(np.uint16) != ref.view(np.uint16)
    at = tuple(np.argwhere(diff)[0]) if diff.any() else None
    assert at is None, "%s: %d of %d values differ from numpy's float16 rounding, first at %s: GPU %r, numpy %r" % (what, diff.sum(), diff.size, at, h[:rows][at], ref[at])
    if feats:
        assert not h[:rows, 96:].view(np.uint16).any(), "columns 96 .. 127 are not +0.0"
    print("RATIO %-60s bit-equal" % what)
