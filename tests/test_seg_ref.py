"""Pins tests/seg_ref.py -- the float64 references tests/test_seg_kernels.py compares the kernels of csrc/pyannet.hip with -- on the CPU, before
anything is compared with them: against torch in float64 (nn.LSTM, max_pool1d + instance_norm + leaky_relu, instance_norm, linear + sigmoid) and
against the stages PyanNetOracle exposes.  Then it shows, on the inputs of every GPU case (tests/seg_cases.py), that the case's tolerance tells
the deliberate mistakes ("mutants") of seg_ref.py from the reference: error of the mutant / tolerance >= 10.

Where each mutant shows -- asserted: it differs there, and by >= 10 tolerances:
  lstm        swap_g_o       every case
              swap_whh       every case with F > 1 and W_hh != 0  (h_0 = 0: the first step does not read W_hh)
              no_reverse     every case with F > 1
              carry_state    every case with B > 1
              drop_input     every case with F > 1 and W_hh != 0
  pool_norm   no_abs         stage0 / shared0 at Lp > 1, on inputs that have negative values (normal, outlier; mean5 in the shared form)
              shift_window   every case with Lp > 1 (the last window of a chunk reads the next chunk's first row, or the NaN behind the input)
              slope0         every case with Lp > 1, the real lengths on mean5 input excepted
              stats_short    every case below the real lengths (Lp = 1: no statistics at all, NaN)
              var_unbiased   Lp = 5 .. 40 on every input kind
              no_eps         mean5 input (variance 1e-4 to 0.1 after the affine map) at Lp = 5 .. 40, and Lp = 1 (var = 0: NaN)
  chunk_norm  stats_80000    every L < 80000
              var_unbiased   loud input at L = 255, 257 and 1000
              no_eps         near-silent input (variance 4e-8 against eps 1e-5) at every L, and L = 1 (NaN)
  classifier  no_zero        every F < 293
              perm_w         every case
Everywhere else a mutant either equals the reference (Lp = 1: m = mu, the output is leaky_relu(gb) whatever the windows hold) or is >= 10 tolerances
away as well -- asserted -- with these exceptions, which are printed with their figure instead:
  - var_unbiased, no_eps and stats_short change the result by a RELATIVE 1 / (2 Lp), eps / (2 var) and about 1 / Lp.  The bound's own relative term is
    gamma_(Lp + 3) / 2 + 4 u, so at Lp = 2658 / 884 / 293 and L = 80000, and for eps against a variance of order one or larger (normal and outlier
    inputs, loud chunks), they are not ten bounds away and partly inside the bound (pool_norm at Lp = 2658: unbiased variance 1.3 bounds).  On
    near-silent chunks the variance is far below eps and its divisor hardly enters.  The long cases are there for the strided loops and the
    indexing; the statistics are pinned by the short ones.
  - slope0 at Lp = 1 and at the real lengths on mean5 input: the variance is 0 resp. 1e-4, a = |gw| / sqrt(var + eps) is 100 to 316 and multiplies the
    rounding of every m - mu, so the bound is as wide as the 0.01 |y| the slope is worth.
A mutant output that is not finite counts as caught: the GPU tests assert that no output is NaN."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_cases as K
import seg_ref as R


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ---------------------------------------------------------------- torch pins
@pytest.mark.parametrize("B,T", [(1, 1), (3, 7), (2, 30)])
def test_lstm_ref_equals_torch_lstm(B, T):
    torch.manual_seed(B * 100 + T)
    lstm = torch.nn.LSTM(60, 128, num_layers=1, bidirectional=True, batch_first=True).double().eval()
    x = torch.randn(B, T, 60, dtype=torch.float64)
    with torch.no_grad():
        ref = lstm(x)[0].numpy()
    p = {k: v.detach().numpy() for k, v in lstm.state_dict().items()}
    G = np.concatenate([x.numpy() @ p["weight_ih_l0" + s].T + p["bias_ih_l0" + s] + p["bias_hh_l0" + s] for s in ("", "_reverse")], -1)
    H = R.lstm_ref(G, p["weight_hh_l0"], p["weight_hh_l0_reverse"])
    assert H.shape == (B, T, 256) and close(H, ref)
    for m in R.LSTM_MUTANTS:                                # (the mutants are mutants: none of them is the reference in disguise)
        if T > 1 and (B > 1 or m != "carry_state"):
            assert not close(R.lstm_ref(G, p["weight_hh_l0"], p["weight_hh_l0_reverse"], mutant=m), ref, 1e-6), m


@pytest.mark.parametrize("stage,Lc,chunks", [(0, 17, 2), (1, 40, 3), (2, 49, 1), (0, 6, 2)])
def test_pool_norm_ref_equals_torch(stage, Lc, chunks):
    rng = np.random.default_rng(Lc)
    C = 80 if stage == 0 else 60
    x = rng.standard_normal((chunks * Lc, C))
    gw, gb = rng.standard_normal(C), rng.standard_normal(C)
    y = R.pool_norm_ref(x, chunks, Lc, stage, gw, gb)
    t = torch.from_numpy(x).reshape(chunks, Lc, C).transpose(1, 2)
    if stage == 0:
        t = t.abs()
    t = F.max_pool1d(t, 3, 3)
    ref = F.leaky_relu(F.instance_norm(t, weight=torch.from_numpy(gw), bias=torch.from_numpy(gb), eps=1e-5)).transpose(1, 2).numpy()
    assert y.shape == (chunks, Lc // 3, C) and close(y, ref)
    # one window (torch refuses a single spatial element): m = mu, var = 0, so the output is leaky_relu(gb)
    one = R.pool_norm_ref(x[:chunks * 5], chunks, 5, stage, gw, gb)
    assert one.shape == (chunks, 1, C) and np.array_equal(one, np.broadcast_to(np.where(gb > 0, gb, 0.01 * gb), one.shape))
    # the shared form: chunk ck = a_ck x[ck * chunk_rows ...] + c_ck wsum is the plain form of those values
    if stage == 0:
        cst, wsum, rows = rng.standard_normal((chunks, 2)), rng.standard_normal(80), 5
        xs = rng.standard_normal(((chunks - 1) * rows + Lc, C))
        flat = np.concatenate([xs[ck * rows:ck * rows + Lc] * cst[ck, 0] + cst[ck, 1] * wsum for ck in range(chunks)])
        assert close(R.pool_norm_ref(xs, chunks, Lc, 0, gw, gb, cst=cst, wsum=wsum, chunk_rows=rows), R.pool_norm_ref(flat, chunks, Lc, 0, gw, gb))


@pytest.mark.parametrize("L,hop,first,origin", [(2, 8000, 0, 0), (257, 257, 0, 0), (1000, 8000, 2, 12000)])
def test_chunk_norm_ref_equals_torch_instance_norm(L, hop, first, origin):
    rng = np.random.default_rng(L)
    chunks = 3
    wav = 0.3 * rng.standard_normal((first + chunks - 1) * hop - origin + L + 100) + 0.1
    xn, ac = R.chunk_norm_ref(wav, origin, first, hop, L, chunks, 1.3, -0.2)
    rows = np.stack([wav[(first + ck) * hop - origin:][:L] for ck in range(chunks)])
    ref = F.instance_norm(torch.from_numpy(rows)[:, None, :], weight=torch.tensor([1.3], dtype=torch.float64), bias=torch.tensor([-0.2], dtype=torch.float64), eps=1e-5)[:, 0].numpy()
    assert close(xn[:, :L], ref) and not xn[:, L:].any()
    assert close(rows * ac[:, :1] + ac[:, 1:], ref)       # the affine form k_chunk_stats hands to the shared-conv0 path
    one, _ = R.chunk_norm_ref(wav, origin, first, hop, 1, chunks, 1.3, -0.2)      # one sample (torch refuses it): x = mu, so xn = b
    assert np.array_equal(one[:, 0], np.full(chunks, -0.2)) and not one[:, 1:].any()


@pytest.mark.parametrize("chunks,Fr", [(1, 1), (2, 171), (1, 293)])
def test_classifier_ref_equals_torch(chunks, Fr):
    rng = np.random.default_rng(Fr)
    y, W, b = rng.standard_normal((chunks * Fr, 128)), rng.standard_normal((3, 128)), rng.standard_normal(3)
    seg = R.classifier_ref(y, W, b, chunks, Fr)
    ref = torch.sigmoid(F.linear(torch.from_numpy(y), torch.from_numpy(W), torch.from_numpy(b))).numpy().reshape(chunks, Fr, 3)
    assert seg.shape == (chunks, 293, 3) and close(seg[:, :Fr], ref) and not seg[:, Fr:].any()


def test_references_chain_to_the_stages_the_oracle_exposes():
    """PyanNetOracle(float64, return_intermediate=True) exposes the SincNet features (behind the three pool / norm stages), the LSTM output and the scores.
    chunk_norm_ref -> conv0 -> pool_norm_ref(0) -> conv1 -> pool_norm_ref(1) -> conv2 -> pool_norm_ref(2) gives the features; four lstm_ref layers on
    them the LSTM output; classifier_ref behind the two linear layers the scores (convolutions and linear layers by torch, float64)."""
    from oracle import nn_oracle as nn
    w = nn.synth_segmentation_weights()
    t = lambda k: torch.as_tensor(np.asarray(w[k]), dtype=torch.float64)
    rng = np.random.default_rng(4)
    B, T = 2, 9000
    wav = 0.1 * rng.standard_normal((B, T)) + 0.02
    scores, feat, h = nn.PyanNetOracle(w, torch.float64)(wav, return_intermediate=True)
    xn, _ = R.chunk_norm_ref(wav.reshape(-1), 0, 0, T, T, B, float(t("sincnet.wav_norm.weight")), float(t("sincnet.wav_norm.bias")))
    x = torch.from_numpy(xn[:, None, :T])
    for i in range(3):
        x = F.conv1d(x, t("sincnet.conv%d.weight" % i), None if i == 0 else t("sincnet.conv%d.bias" % i), stride=10 if i == 0 else 1)
        Lc = x.shape[2]
        y = R.pool_norm_ref(x.transpose(1, 2).reshape(B * Lc, -1).numpy(), B, Lc, i, t("sincnet.norm%d.weight" % i).numpy(), t("sincnet.norm%d.bias" % i).numpy())
        x = torch.from_numpy(y).transpose(1, 2)
    f = x.transpose(1, 2).numpy()
    assert f.shape == tuple(feat.shape) and f.shape[1] == 30 and close(f, feat.numpy(), 1e-11)
    hh = f
    for l in range(4):
        G = np.concatenate([hh @ t("lstm.weight_ih_l%d%s" % (l, s)).numpy().T + t("lstm.bias_ih_l%d%s" % (l, s)).numpy() + t("lstm.bias_hh_l%d%s" % (l, s)).numpy()
                            for s in ("", "_reverse")], -1)
        hh = R.lstm_ref(G, t("lstm.weight_hh_l%d" % l).numpy(), t("lstm.weight_hh_l%d_reverse" % l).numpy())
    assert close(hh, h.numpy(), 1e-11)
    y = F.leaky_relu(F.linear(torch.from_numpy(hh), t("linear.0.weight"), t("linear.0.bias")))
    y = F.leaky_relu(F.linear(y, t("linear.1.weight"), t("linear.1.bias"))).numpy()
    Fr = y.shape[1]
    seg = R.classifier_ref(y.reshape(B * Fr, 128), t("classifier.weight").numpy(), t("classifier.bias").numpy(), B, Fr)
    assert close(seg[:, :Fr], scores.numpy(), 1e-11)


# ---------------------------------------------------------------- the tolerances separate right from wrong
def ratio(mut, ref, tol):
    """max(error of the mutant / tolerance); 0.0 = the mutant equals the reference here; inf = the mutant is not finite (the GPU tests assert finiteness)"""
    if not np.isfinite(mut).all():
        return np.inf
    err = np.abs(np.asarray(mut, np.float64) - ref)
    if not err.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0, err / tol, 0.0)             # (tol = 0 where the output must be exact: any error there is infinitely many bounds)
    return float(q.max())


def check(table, family, must_show, may_be_inside=lambda m, case: False):
    """table {(mutant, case): ratio}.  must_show(mutant, case) -> the mutant has to differ there.  Wherever a mutant differs it is >= 10 tolerances away,
    except the (statistics mutant, case) pairs may_be_inside names, which are printed"""
    for (m, case), q in sorted(table.items(), key=str):
        if must_show(m, case):
            assert q > 0, "%s: mutant %s does not differ from the reference in case %s" % (family, m, case)
        if q and may_be_inside(m, case) and q < 10:
            print("%s: mutant %-13s case %-40s %.2f tolerances (not asserted)" % (family, m, case, q))
        elif q:
            assert q >= 10, "%s: mutant %s is only %.2f tolerances from the reference in case %s" % (family, m, q, case)
    for m in {m for m, _ in table}:
        shows = [case for (mm, case), q in table.items() if mm == m and q >= 10]
        assert shows, "%s: no case shows mutant %s" % (family, m)
        print("%s: mutant %-13s shows in %d of %d cases, weakest %.1f tolerances" % (family, m, len(shows), len([1 for mm, _ in table if mm == m]),
                                                                                    min(table[m, c] for c in shows)))


def test_lstm_tolerance_separates_every_mutant():
    table = {}
    for B, Fr, kind in K.LSTM_CASES:
        G, wf, wb = K.lstm_operands(B, Fr, kind)
        H, e32 = K.lstm_reference(B, Fr, kind)
        assert 0 < e32 < 2e-6, (B, Fr, kind, e32)          # f32 evaluation of the same graph: a few ulp of values below 1
        for m in R.LSTM_MUTANTS:
            table[m, (B, Fr, kind)] = ratio(R.lstm_ref(G, wf, wb, mutant=m), H, 8 * e32)

    def must_show(m, case):
        B, Fr, kind = case
        return {"swap_g_o": True, "swap_whh": Fr > 1 and kind != "whh0", "no_reverse": Fr > 1, "carry_state": B > 1, "drop_input": Fr > 1 and kind != "whh0"}[m]
    check(table, "lstm", must_show)


def test_pool_norm_bound_separates_every_mutant():
    table = {}
    for case in K.POOL_CASES:
        form, Lc, chunks, kind = case
        o = K.pool_operands(*case)
        y, bound = K.pool_reference(*case)
        for m in R.POOL_MUTANTS:
            if m == "no_abs" and o["stage"] != 0:
                continue
            table[m, case] = ratio(R.pool_norm_ref(mutant=m, **o), y, bound)

    def must_show(m, case):
        form, Lc, chunks, kind = case
        Lp, real = Lc // 3, Lc > 800
        return {"no_abs": Lp > 1 and (kind != "mean5" or form == "shared0"), "shift_window": Lp > 1, "stats_short": not real,
                "slope0": Lp > 1 and not (real and kind == "mean5"), "var_unbiased": 5 <= Lp <= 40, "no_eps": (kind == "mean5" and not real) or Lp == 1}[m]

    def may_be_inside(m, case):
        form, Lc, chunks, kind = case
        Lp, real = Lc // 3, Lc > 800
        return {"no_abs": False, "shift_window": False, "stats_short": real, "var_unbiased": real, "no_eps": kind != "mean5" or real,
                "slope0": Lp == 1 or (real and kind == "mean5")}[m]
    check(table, "pool_norm", must_show, may_be_inside)


def test_chunk_norm_bound_separates_every_mutant():
    table = {}
    for case in K.CHUNK_CASES:
        lay, L, kind = case
        o = K.chunk_operands(*case)
        xn, ac, bx, ba, bc = K.chunk_reference(*case)
        tol = np.zeros_like(xn)
        tol[:, :L] = bx
        for m in R.CHUNK_MUTANTS:
            mx, mac = R.chunk_norm_ref(mutant=m, **o)
            table[m, case] = ratio(mx, xn, tol)
            if lay != "rows":                               # k_chunk_stats runs these too: (a, c) against its own bound
                table[m + " (a, c)", case] = ratio(mac, ac, np.stack([ba, bc], 1))

    def must_show(m, case):
        lay, L, kind = case
        return {"stats_80000": L < 80000, "var_unbiased": kind == "loud_dc" and 1 < L <= 1000, "no_eps": kind == "near_silent" or L == 1}[m.split()[0]]

    def may_be_inside(m, case):
        lay, L, kind = case
        return {"stats_80000": False, "var_unbiased": kind == "near_silent" or L == 80000, "no_eps": kind == "loud_dc" and L > 1}[m.split()[0]]
    check(table, "chunk_norm", must_show, may_be_inside)


def test_classifier_bound_separates_every_mutant():
    table = {}
    for case in K.CLS_CASES:
        o = K.cls_operands(*case)
        seg, bound = K.cls_reference(*case)
        for m in R.CLS_MUTANTS:
            table[m, case] = ratio(R.classifier_ref(mutant=m, **o), seg, bound)
    check(table, "classifier", lambda m, case: m == "perm_w" or case[1] < 293)
