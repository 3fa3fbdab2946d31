"""Pins tests/ecapa_glue_ref.py -- the float64 references tests/test_ecapa_glue.py compares the glue kernels of csrc/ecapa.hip with -- on the CPU, before
anything is compared with them: against the torch formulas of oracle/nn_oracle.py in float64 (_se_res2net's masked mean, `stats`, masked_fill +
softmax, s * x + res) on random tensors and lengths.  Then it shows, on the inputs of every GPU case (tests/ecapa_glue_cases.py; the first 48
channels of each: channels do not interact), that the case's tolerance tells the deliberate mistakes ("mutants") of ecapa_glue_ref.py from the
reference: error of the mutant / tolerance >= 10 in at least one case, and it is asserted where.

Where each mutant must show:
  mean, stats   div_nm1, div_np1, incl_nv, skip_last    every case (the frame behind the valid ones holds NaN, another item's first frame, or the guard)
  stats         no_clamp, clamp_after, eps6    every case with a column that is constant over an item's frames: sqrtf(1e-12f) is demanded exactly there
                (nvalid = 1 is in every item set but "one")
  pool          no_clamp, clamp_after, eps6    the "const" data, in its all-zero columns: every step is exact there whatever v_exp_f32 and v_rcp_f32 give
                incl_nv              every case
                skip_last            every case with an item of 2 .. 9 frames, but "cancel" data and spike200
                no_rescale           the ascending logits (a new maximum at every frame), n30, spike200, jump100
                unweighted_mean      every case with more than one item and logits that are neither constant nor spike200, but "cancel" data
  se_apply      next_gate, res_off1  every case;  out_at_t2_row: the patterns with an output map (b1, b2)
  rowtab        n_in                 every case
Exceptions, printed with their figure instead of asserted:
  - pool's clamp mutants outside the all-zero columns.  On any other constant column, nvalid = 1 included, a reciprocal that is 1 ulp off leaves
    mean = v (1 - 2^-23) and a variance of v^2 2^-23: the bound, which assumes no more than 1 ulp of the two instructions, is wider than the clamp.
  - pool on "cancel" data (mean 1e3, deviation 1e-2): the one-pass update rounds a mean of 1e3 at every frame, the derived bound says so and is as
    wide as the data's deviation.  The zero-mean cases pin what it cannot.
A mutant output that is not finite counts as caught: the GPU tests assert that every output is finite."""
import numpy as np
import pytest
import torch

import ecapa_glue_cases as K
import ecapa_glue_ref as R

CS = 48                                     # channels of a case the mutant tables look at


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ---------------------------------------------------------------- torch pins
def _torch_case(seed, B=5, C=24, L=40):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, L))
    lengths = np.concatenate([[1.0, 1.0 / L], rng.uniform(0.05, 1.0, B - 2)])
    mask = (torch.arange(L)[None, :] < (torch.from_numpy(lengths) * L)[:, None]).to(torch.float64)[:, None, :]      # EcapaOracle._mask
    nv = mask.sum((1, 2)).numpy().astype(np.int32)
    rowoff = (np.arange(B + 1) * L).astype(np.int32)
    rows = np.ascontiguousarray(x.transpose(0, 2, 1).reshape(B * L, C))                                             # channels-last rows
    return x, mask, nv, rowoff, rows, rng


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_statistics_refs_equal_the_torch_formulas_of_the_oracle(seed):
    x, mask, nv, rowoff, rows, rng = _torch_case(seed)
    B, C, L = x.shape
    assert nv.min() == 1 and nv.max() == L
    xt = torch.from_numpy(x)
    total = mask.sum(dim=2, keepdim=True)
    s = ((xt * mask).sum(dim=2, keepdim=True) / total)[:, :, 0].numpy()                     # _se_res2net
    assert close(R.masked_mean_ref(rows, nv, rowoff, C), s)

    def stats(x, m):                                                                        # EcapaOracle.__call__
        mean = (m * x).sum(2)
        std = torch.sqrt((m * (x - mean.unsqueeze(2)).pow(2)).sum(2).clamp(1e-12))
        return mean, std
    mean, std = stats(xt, mask / total)
    assert close(R.asp_stats_ref(rows, nv, rowoff, C), torch.cat([mean, std], 1).numpy())
    for scale in (1.0, 30.0):
        lg = scale * rng.standard_normal((B, C, L))
        attn = torch.from_numpy(lg).masked_fill(mask == 0, float("-inf"))
        mean, std = stats(xt, torch.softmax(attn, dim=2))
        lrows = np.ascontiguousarray(lg.transpose(0, 2, 1).reshape(B * L, C))
        assert close(R.asp_pool_ref(rows, lrows, nv, rowoff, C), torch.cat([mean, std], 1).numpy())
    # constant logits: the softmax is uniform, the pooling is the plain statistics
    assert close(R.asp_pool_ref(rows, np.full_like(rows, 2.5), nv, rowoff, C), R.asp_stats_ref(rows, nv, rowoff, C))
    # the mutants are mutants
    for m in R.STATS_MUTANTS:
        if m not in ("no_clamp", "clamp_after"):            # (these two show on a zero variance only: nvalid = 1, below)
            assert not close(R.asp_stats_ref(rows, nv, rowoff, C, mutant=m), R.asp_stats_ref(rows, nv, rowoff, C), 1e-6), m
    one = R.asp_stats_ref(rows, nv, rowoff, C)[1, C:]
    assert np.array_equal(one, np.full(C, 1e-6))
    assert not R.asp_stats_ref(rows, nv, rowoff, C, mutant="no_clamp")[1, C:].any() and close(R.asp_stats_ref(rows, nv, rowoff, C, mutant="clamp_after")[1, C:], 1e-12, 1e-3)


def test_se_apply_ref_equals_the_torch_formula_of_the_oracle():
    """s * x + res of _se_res2net on [B][C][L] tensors against se_apply_ref on the same numbers as rows of one space (no maps), then of three
    different spaces (the maps move rows, not values)"""
    rng = np.random.default_rng(9)
    B, C, L = 3, 8, 11
    x, res, s = rng.standard_normal((B, C, L)), rng.standard_normal((B, C, L)), rng.uniform(0, 1, (B, C))
    ref = (torch.from_numpy(s)[:, :, None] * torch.from_numpy(x) + torch.from_numpy(res)).numpy().transpose(0, 2, 1).reshape(B * L, C)
    rows = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1).reshape(B * L, C))
    off = np.tile(np.arange(B + 1) * L, (4, 1)).astype(np.int32)
    buf, written, _ = R.se_apply_ref(rows(x), s, rows(res), off, 1, 0, 1, shared=False, y_ld=C + 4, out_col0=4)
    assert written[:, 4:].all() and not written[:, :4].any() and close(buf[:, 4:], ref) and (buf[:, :4] == -7776.0).all()
    # ragged spaces: item i stores n[s][i] frames in space s; the output holds (item, t) at the row of space ys
    n = np.array([[11, 11, 11], [9, 11, 10], [5, 11, 7], [2, 11, 3]])
    off = np.concatenate([np.zeros((4, 1), int), np.cumsum(n, 1)], 1).astype(np.int32)
    pick = lambda a, sp: np.concatenate([a[i, :, :n[sp, i]].T for i in range(B)])
    buf, written, _ = R.se_apply_ref(pick(x, 2), s, pick(res, 1), off, 2, 1, 1, shared=True, y_ld=2 * C, out_col0=C, res_col0=0)
    for i in range(B):
        r1 = off[1, i]
        assert close(buf[r1:r1 + n[2, i], C:], ref[i * L:i * L + n[2, i]]) and written[r1:r1 + n[2, i], C:].all()
        assert (buf[r1 + n[2, i]:off[1, i + 1], C:] == -7776.0).all() and not written[r1 + n[2, i]:off[1, i + 1]].any()
    assert np.array_equal(buf[:, :C], pick(res, 1)) and not written[:, :C].any()


def test_small_refs_by_hand():
    tab = R.rowtab_ref([10, 12, 15], [100, 105, 106])
    assert tab.tolist() == [[0, 0 | 4 << 10 | 0 << 20], [0, 1 | 4 << 10], [5, 0 | 0 << 10 | 1 << 20], [5, 1 | 1 << 20], [5, 2 | 1 << 20]]
    assert R.rowtab_ref([0, 1], [0, 1], mutant="n_in").tolist() == [[0, 1 << 10]]
    big = R.rowtab_ref(np.arange(4096), np.arange(4096))
    assert big.dtype == np.int32 and big[4094, 1] == np.int64(4094 << 20) - (1 << 32) and (big[4094, 1].astype(np.uint32) >> 20) == 4094
    e = np.arange(2 * 192, dtype=np.float32).reshape(2, 192)
    s = R.scatter_emb_ref(e, [1, -1, 0])
    assert np.array_equal(s[0], e[1].view(np.uint32)) and (s[1] == 0x7fc00000).all() and np.array_equal(s[2], e[0].view(np.uint32))
    h = R.to_half_ref(np.array([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 65520.0, -0.0] + [0.0] * 91], np.float32), feats=True)
    assert h.shape == (1, 128) and h.view(np.uint16)[0, :5].tolist() == [0x3c00, 0x3c02, 0x0000, 0x7c00, 0x8000] and not h[0, 96:].any()


# ---------------------------------------------------------------- the tolerances separate right from wrong
def ratio(mut, ref, tol):
    """max(error of the mutant / tolerance); 0.0 = the mutant equals the reference here; inf = the mutant is not finite (the GPU tests assert finiteness)"""
    if not np.isfinite(mut).all():
        return np.inf
    err = np.abs(np.asarray(mut, np.float64) - ref)
    if not err.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0, err / tol, 0.0)               # (tol = 0 where the output must be exact: any error there is infinitely many bounds)
    return float(q.max())


def check(table, family, must_show):
    """table {(mutant, case): ratio}.  must_show(mutant, case) -> the mutant has to be >= 10 tolerances away there; elsewhere its figure is printed
    when it differs and is closer.  Every mutant shows somewhere"""
    for (m, case), q in sorted(table.items(), key=str):
        if must_show(m, case):
            assert q >= 10, "%s: mutant %s is only %.2f tolerances from the reference in case %s" % (family, m, q, case)
        elif 0 < q < 10:
            print("%s: mutant %-15s case %-50s %.2f tolerances (not asserted)" % (family, m, case, q))
    for m in sorted({m for m, _ in table}):
        shows = [case for (mm, case), q in table.items() if mm == m and q >= 10]
        assert shows, "%s: no case shows mutant %s" % (family, m)
        print("%s: mutant %-15s shows in %d of %d cases, weakest %.1f tolerances" % (family, m, len(shows), len([1 for mm, _ in table if mm == m]),
                                                                                      min(table[m, c] for c in shows)))


def _short_items(case):
    return any(2 <= nv <= 9 for nv in K.ITEM_SETS[case[2]])


@pytest.mark.parametrize("kind", ["mean", "stats"])
def test_statistics_bounds_separate_every_mutant(kind):
    fn = {"mean": R.masked_mean_ref, "stats": R.asp_stats_ref}[kind]
    table = {}
    for case in K.STAT_CASES:
        o = K.stat_operands(*case)
        C = min(CS, o["C_"])
        ref, tol = K.stat_reference(kind, case, C)
        assert np.isfinite(ref).all() and np.isfinite(tol).all() and (tol >= 0).all()
        for m in (R.MEAN_MUTANTS if kind == "mean" else R.STATS_MUTANTS):
            table[m, case] = ratio(fn(o["x"], o["nvalid"], o["rowoff"], C, mutant=m), ref, tol)

    def must_show(m, case):
        data, has_one = case[4], 1 in K.ITEM_SETS[case[2]]
        if m in ("no_clamp", "clamp_after", "eps6"):
            return has_one or data == "const" or (data == "cancel" and case[6])
        return True
    check(table, kind, must_show)


def test_pool_bound_separates_every_mutant():
    table = {}
    for case in K.POOL_CASES:
        o = K.stat_operands(*case)
        C = min(CS, o["C_"])
        ref, tol = K.stat_reference("pool", case, C)
        assert np.isfinite(ref).all() and np.isfinite(tol).all() and (tol >= 0).all()        # (0: an all-zero column's mean)
        if case[5] == "const":                              # constant logits: the result must agree with the k_asp_stats reference
            assert close(ref, R.asp_stats_ref(o["x"], o["nvalid"], o["rowoff"], C))
        if case[5] == "spike200":                           # the weights beside the spike underflow: the std hits the clamp
            assert (ref[:, C:] == 1e-6).all()
        for m in R.POOL_MUTANTS:
            table[m, case] = ratio(R.asp_pool_ref(o["x"], o["logits"], o["nvalid"], o["rowoff"], C, mutant=m), ref, tol)

    def must_show(m, case):
        data, lg, has_one = case[4], case[5], 1 in K.ITEM_SETS[case[2]]
        if m in ("no_clamp", "clamp_after", "eps6"):
            return data == "const"
        if m == "incl_nv":
            return True
        if m == "skip_last":
            return _short_items(case) and data != "cancel" and lg != "spike200"
        if m == "no_rescale":
            return lg in ("asc", "n30", "spike200", "jump100") and data != "cancel"
        return m == "unweighted_mean" and lg not in ("const", "spike200") and case[2] != "one" and data != "cancel"
    check(table, "pool", must_show)


def test_se_apply_bound_separates_every_mutant():
    table = {}
    for case in K.SE_CASES:
        o = K.se_operands(*case)
        buf, tol, written = K.se_reference(*case)
        assert written.any() and (tol[~written] == 0).all() and (tol[written] > 0).all()
        for m in R.SE_MUTANTS:
            table[m, case] = ratio(R.se_apply_ref(canary=K.CANARY, mutant=m, **o)[0], buf, tol)
    check(table, "se_apply", lambda m, case: m != "out_at_t2_row" or case[0] != "b0")


def test_rowtab_mutant_differs_in_every_case():
    for name, (oo, oi) in K.rowtab_cases().items():
        assert not np.array_equal(R.rowtab_ref(oo, oi), R.rowtab_ref(oo, oi, mutant="n_in")), name
