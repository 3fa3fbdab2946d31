"""Every kernel of csrc/pyannet.hip that is not a convolution, on its own, against the float64 references of tests/seg_ref.py.

Diarizer.lstm_rec_case / pool_norm_case / chunk_norm_case / classifier_case (sd_test_* of include/sdhip_test.h) launch ONE kernel through the
launcher seg_batch uses, on operands the test chooses.  Every input is followed by NaN, every output buffer is filled with a canary and has 256
slack rows behind it; each test asserts that no guard element changed and that no output is NaN.  The cases and their operands live in
tests/seg_cases.py; tests/test_seg_ref.py pins the references to torch and shows on the CPU that each tolerance below is at least ten times
smaller than what a wrong gate, direction, divisor, eps, window ... does (and where it is not: the statistics at the real lengths).

LSTM (k_lstm_rec, k_lstm_rec_x3).  A bound cannot be derived through up to 293 non-linear steps, so the yardstick is measured: e32 = the max error
of seg_ref.lstm_ref evaluated in float32 against the same function in float64, on the same operands (1.4e-8 .. 1.9e-6 over the cases here).  The kernel must stay within
8 e32 -- the margin this project gives two f32 evaluations of one graph in different orders (test_ecapa_mfa_every_valid_frame_..., test_embed_parity).
(B, F) puts 1, 31, 32, 33, 64 and 65 chunks on the 32-chunk workgroups, at the real F = 293, the short last chunk's 171 and a few small ones; the
data put the pre-activations at moderate size, deep in saturation, on both sides of tanh_fast's switch at 0.18, and -- W_hh = 0 -- make H a
function of G element by element.  The x3 kernel must also differ from the f32 kernel in at least one bit wherever W_hh enters (F > 1, W_hh != 0).

pool_norm (k_pool_norm, three instantiations + the shared form).  Per element, from the float64 reference's pooled value m, the channel's mu and
var, r = (var + eps)^-1/2, a = r |gw|, with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1):
    mean of Lp values summed in any order, one division:             d_mu  = gamma_Lp mean|m| + u |mu|
    sum of Lp squares of (m - mu), the subtraction, the division:    d_var = gamma_(Lp + 3) var + d_mu^2        (d_mu^2: the mean is off by d_mu)
    r = rsqrt(var + eps): relative d_var / (2 (var + eps)) + 2 u;  a = r gw: + u;  the product (m - mu) a: + u
    y = m a + (gb - mu a):  a |m - mu| (d_var / (2 (var + eps)) + 4 u)  +  a d_mu  +  3 u (a |m| + a |mu| + |gb|)
The last term is what the kernel's form m * a + (gb - mu * a) costs where m a and mu a cancel (large mean).  leaky_relu is 1-Lipschitz.  The shared
form computes m = |v c_a + c_c wsum| first: d_m = 2 u (|v c_a| + |c_c wsum|) on every m, which adds a d_m to the bound and mean(d_m) to d_mu.
Padding channels must be exactly 0.0.  The bound discriminates at small Lp only (test_seg_ref.py); the real lengths 7975 / 2654 / 880 are there
for the strided loops and the indexing.

chunk_norm / chunk_stats.  The same bound with Lp -> L, gw -> w, m -> x.  xn[j >= L] is exactly 0.  (a, c) of k_chunk_stats: a = r w within
|a| (d_var / (2 (var + eps)) + 4 u);  c = b - mu a within |mu| d_a + |a| d_mu + 3 u (|a mu| + |b|).

classifier.  gamma_131 S, S = sum |x| |w| + |b| (128 products, their additions in any order, the bias) through the 1-Lipschitz sigmoid, plus 4 ulp of
the output for expf and the division.  Frames >= F are exactly 0.

Measured on the MI355X, max(error / tolerance) per kernel family:
    k_pool_norm stage 0  0.341   stage 1  0.324   stage 2  0.285   shared form  0.276      (worst: Lp = 13 / 16 on the outlier input; real lengths 0.06 and below)
    k_chunk_norm  0.153 (at L = 1; 0.01 and below from L = 255 on)   k_chunk_stats  0.289 (L = 1; 0.27 at L >= 255)   k_classifier  0.002
LSTM, max error in units of e32 over the 28 cases (limit 8):
    k_lstm_rec     0.80 .. 2.32   (mid 0.84 .. 1.23, wide 0.80 .. 1.38, small 1.28 .. 2.32, W_hh = 0: 0.86 .. 1.23)
    k_lstm_rec_x3  0.52 .. 2.29   (mid 0.89 .. 1.01, wide 0.52 .. 1.32, small 1.52 .. 2.29, W_hh = 0: 0.86 .. 1.23, the bits of k_lstm_rec)
The largest ratios belong to the small data, where e32 itself is smallest (1.4e-8 .. 5.5e-8: outputs of 0.02): tanh_fast's polynomial branch and
v_rcp_f32 cost about one more ulp there than numpy's float32 tanh and division.  The whole file: 83 tests in 4 s, none above 0.2 s.
"""
import numpy as np
import pytest

import sdhip
import seg_cases as K

pytestmark = pytest.mark.gpu

CANARY = np.float32(-7776.0)
SLACK = sdhip.SEG_SLACK_ROWS


def live_and_guard(buf, rows, what):
    """buf [rows + SLACK][w] -> buf[:rows]; the slack rows must hold the canary, the live rows no NaN and no canary"""
    assert buf.shape[0] == rows + SLACK, (buf.shape, rows)
    bad = buf[rows:] != CANARY
    assert not bad.any(), "%s: %d guard elements behind the output were overwritten, first at row %d + %d" % (what, bad.sum(), rows, np.argwhere(bad)[0][0])
    y = buf[:rows]
    assert not np.isnan(y).any(), "%s: NaN in the output (something behind an input was read): first at %s" % (what, np.argwhere(np.isnan(y))[0])
    return y


def report(what, err, tol):
    """print max(error / tolerance), assert it is <= 1; tol = 0 demands an exact value"""
    exact = tol == 0
    assert not err[exact].any(), "%s: %d values that must be exact are not" % (what, np.count_nonzero(err[exact]))
    q = err[~exact] / tol[~exact]
    ratio = float(q.max()) if q.size else 0.0
    print("RATIO %-60s max(error / tolerance) = %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: %d values beyond the tolerance, max(error / tolerance) = %.3f, first at %s" % (what, (q > 1).sum(), ratio, np.argwhere((err > tol) & ~exact)[0])
    return ratio


# ---------------------------------------------------------------- LSTM
@pytest.mark.parametrize("B,F,kind", K.LSTM_CASES)
def test_lstm_rec(diarizer, B, F, kind):
    G, wf, wb = K.lstm_operands(B, F, kind)
    H, e32 = K.lstm_reference(B, F, kind)
    got = {}
    for prec, name in ((0, "k_lstm_rec"), (3, "k_lstm_rec_x3")):
        what = "%s B=%d F=%d %s" % (name, B, F, kind)
        y = live_and_guard(diarizer.lstm_rec_case(G, wf, wb, prec=prec, canary=CANARY), B * F, what).reshape(B, F, 256)
        assert not (y == CANARY).any(), "%s: %d outputs were never written" % (what, (y == CANARY).sum())
        err = np.abs(y.astype(np.float64) - H)
        print("RATIO %-60s max error = %.3e = %.2f e32 (e32 = %.3e, limit 8)" % (what, err.max(), err.max() / e32, e32))
        got[prec] = y, err.max() / e32, np.unravel_index(np.argmax(err), err.shape)
    for prec, (y, q, at) in got.items():
        assert q <= 8.0, "prec %d: %.2f e32 at (chunk, frame, unit) = %s: GPU %r, float64 %r" % (prec, q, at, y[at], H[at])
    if F > 1 and kind != "whh0":
        assert not np.array_equal(got[0][0], got[3][0]), "prec 3 gave the bits of the f32 kernel: k_lstm_rec_x3 did not run"


# ---------------------------------------------------------------- pool_norm
@pytest.mark.parametrize("form,Lc", [(form, Lc) for form in K.POOL_FORMS for Lc in K.POOL_LC + [K.POOL_REAL[form]]])
def test_pool_norm(diarizer, form, Lc):
    for chunks in (1, 3):
        for kind in K.POOL_KINDS:
            o = K.pool_operands(form, Lc, chunks, kind)
            ref, bound = K.pool_reference(form, Lc, chunks, kind)
            what = "k_pool_norm %s Lc=%d chunks=%d %s" % (form, Lc, chunks, kind)
            Lp, C = Lc // 3, ref.shape[2]
            y = live_and_guard(diarizer.pool_norm_case(canary=CANARY, **o), chunks * Lp, what)
            assert not y[:, C:].any(), "%s: padding channels are not exactly 0.0" % what
            report(what, np.abs(y[:, :C].astype(np.float64) - ref.reshape(-1, C)), bound.reshape(-1, C))


# ---------------------------------------------------------------- chunk_norm / chunk_stats
@pytest.mark.parametrize("layout,L,kind", K.CHUNK_CASES)
def test_chunk_norm_and_chunk_stats(diarizer, layout, L, kind):
    o = K.chunk_operands(layout, L, kind)
    xn, ac, bx, ba, bc = K.chunk_reference(layout, L, kind)
    chunks = o["chunks"]
    what = "k_chunk_norm %s L=%d %s" % (layout, L, kind)
    buf = diarizer.chunk_norm_case(canary=CANARY, **o)
    y = live_and_guard(buf.reshape(-1, 4), chunks * 20000, what).reshape(chunks, 80000)
    tol = np.zeros_like(xn)
    tol[:, :L] = bx                                       # (zero beyond L: the tail must be exactly 0)
    report(what, np.abs(y.astype(np.float64) - xn), tol)
    if layout != "rows":
        what = "k_chunk_stats %s L=%d %s" % (layout, L, kind)
        st = live_and_guard(diarizer.chunk_norm_case(stats_only=True, canary=CANARY, **o), chunks, what)
        report(what, np.abs(st.astype(np.float64) - ac), np.stack([ba, bc], 1))


# ---------------------------------------------------------------- classifier
@pytest.mark.parametrize("chunks,F", K.CLS_CASES)
def test_classifier(diarizer, chunks, F):
    o = K.cls_operands(chunks, F)
    seg, bound = K.cls_reference(chunks, F)
    what = "k_classifier chunks=%d F=%d" % (chunks, F)
    y = live_and_guard(diarizer.classifier_case(canary=CANARY, **o), chunks * 293, what).reshape(chunks, 293, 3)
    assert (bound[:, F:] == 0).all() and (bound[:, :F] > 0).all()
    report(what, np.abs(y.astype(np.float64) - seg), bound)


# ---------------------------------------------------------------- the assembled network across the 32-chunk boundary
def test_segment_chunks_70_rows_against_float64_oracle(diarizer, weights):
    """70 rows of 9000 samples (30 frames each): three LSTM workgroups per direction, the last with 6 live lanes; with seg_batch_chunks = 33 the
    batches are 33, 33 and 4 rows.  Loud, near-silent and DC-offset rows alternate.  Every row against PyanNetOracle in float64; tolerance 8 x the
    error of PyanNetOracle in float32 against the float64 one on the same rows (two f32 evaluations of one graph).
    Measured on the MI355X: torch f32 3.129e-06; GPU 4.181e-06 (1.34 x) in f32 and 4.121e-06 (1.32 x) with seg_precision = 3, the same with batches of
    4096 and of 33; limit 8 x."""
    import torch
    from oracle import nn_oracle as nn
    rng = np.random.default_rng(70)
    rows, T = 70, 9000
    wav = rng.standard_normal((rows, T)) * (1 + 0.5 * np.sin(np.arange(T) / 400.0))
    level = np.array([0.3, 2e-4, 0.05, 1e-3])[np.arange(rows) % 4]
    dc = np.array([0.0, 0.05, 0.2, -0.2])[np.arange(rows) % 4]
    wav = (wav * level[:, None] + dc[:, None]).astype(np.float32)
    r64 = nn.PyanNetOracle(weights[2], torch.float64)(wav).numpy()
    r32 = nn.PyanNetOracle(weights[2], torch.float32)(wav).numpy().astype(np.float64)
    assert r64.shape == (rows, 30, 3)
    e32 = np.abs(r32 - r64).max()
    try:
        for batch in (4096, 33):
            for prec in (0, 3):
                diarizer.set_option("seg_batch_chunks", batch)
                diarizer.set_option("seg_precision", prec)
                out, fr = diarizer.segment_chunks(wav)
                assert fr == 30 and out.shape == (rows, 293, 3) and not out[:, 30:].any()
                err = np.abs(out[:, :30].astype(np.float64) - r64)
                row = int(np.argmax(err.max((1, 2))))
                print("RATIO segment_chunks batch=%d prec=%d: max error against the float64 oracle: torch f32 %.3e, GPU %.3e (%.2f x), worst row %d"
                      % (batch, prec, e32, err.max(), err.max() / e32, row))
                assert err.max() <= 8 * e32, "batch %d, prec %d: worst row %d (%.2f x the float32 oracle's error)" % (batch, prec, row, err.max() / e32)
    finally:
        diarizer.set_option("seg_batch_chunks", 4096)
        diarizer.set_option("seg_precision", -1)
