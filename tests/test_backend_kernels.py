"""Every kernel behind the two networks on its own -- k_binarize_masks, k_count (postseg.hip), k_gather_normalize, k_cluster_means, k_assign,
k_constrained_argmax (cluster.hip), k_activations, k_topk (reconstruct.hip), k_cut_cen_norms, k_assign_cuts, k_activations_cuts, k_topk_cuts (cut.hip),
k_pcm_to_f32, k_f32_to_f64, k_mark_inactive (pipeline.cpp) -- against the float64 references of tests/backend_ref.py.

Diarizer.binarize_case .. mark_inactive_case (sd_test_* of include/sdhip_test.h) make ONE launch through the function the product's stage calls, on
operands of tests/backend_cases.py: NaN (or, for integers and bytes, a value that would change a result) in 256 guard units behind every input, a canary
in and 256 slack units behind every output, the whole buffer back.  Everything here is fp64 without contraction, or integer, so EVERY comparison is byte
equality over the whole returned buffer, slack included: no tolerance, no element left out (the one thing not compared is WHICH NaN sits where the
reference has a NaN: see same()).  tests/test_backend_ref.py pins the references to the oracle and shows, on the CPU, the case that each of twelve
single mistakes changes.

The batched kernels of cut.hip are held to the single-kernel references cut by cut (backend_ref.assign_cuts / recon_cuts call assign, activations and
topk on each cut's own table).  test_clustering_of_wide_rows runs sd_clustering at d = 1 025, where k_cluster_means used to ask for a block of 1 088
threads; its launch now takes at most 1 024 and a thread walks q, q + blockDim.x, ...

Measured on the MI355X: the whole file, 115 tests, in 2.7 s, 1.9 s of it the context; the slowest test 0.09 s (k_activations_cuts + k_topk_cuts on 65
cuts), k_assign at K = 2 049, k_cluster_means at d = 1 025 and sd_clustering at d = 1 025 0.01 s each, every other test below 0.005 s.  An earlier
run with plain byte equality failed in one place only, k_assign with a zero row and a zero centroid: 11 NaN scores whose bits differ from numpy's
NaN, which is why same() compares the place of a NaN and not its bits.
"""
import numpy as np
import pytest

import sdhip
import backend_cases as K
import backend_ref as R
from oracle import orc

pytestmark = pytest.mark.gpu

SD_ERR_ARG = 1
FC, IC = K.FCANARY, K.ICANARY


def same(what, got, exp):
    """byte equality of a whole returned buffer.  A NaN must sit where the reference has one, but which NaN it is is not compared: IEEE 754 leaves sign and
    payload of a NaN that an operation makes (2.0 - NaN in k_assign, where the reference throws and has no value at all) to the machine, and the GPU does
    not choose as x86 does.  Every other element, and every integer and byte, is compared as bytes."""
    got, exp = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
    assert got.dtype == exp.dtype and got.shape == exp.shape, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, exp.dtype, exp.shape)
    raw = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    g, e = got.view(raw).copy(), exp.view(raw).copy()
    if got.dtype.kind == "f":
        g[np.isnan(got)] = e[np.isnan(exp)] = np.array(np.nan, got.dtype).view(raw)
    if g.tobytes() == e.tobytes():
        return
    bad = np.flatnonzero(g != e)
    raise AssertionError("%s: %d of %d elements differ, first at %d (the slack begins at %d): got %r (bits %x), expected %r (bits %x)" % (
        what, len(bad), len(got), bad[0], len(exp) - K.SLACK, got[bad[0]], got.view(raw)[bad[0]], exp[bad[0]], exp.view(raw)[bad[0]]))


def refused(call):
    with pytest.raises(sdhip.SdError) as e:
        call()
    assert e.value.code == SD_ERR_ARG


# ---------------------------------------------------------------- postseg.hip
@pytest.mark.parametrize("want", K.BINARIZE_WANTS, ids="+".join)
@pytest.mark.parametrize("name", K.BINARIZE)
def test_binarize(diarizer, name, want):
    got = diarizer.binarize_case(K.binarize_case(name), want=want, fcanary=FC, icanary=IC)
    exp = K.binarize_expected(name)
    assert sorted(got) == sorted(want)
    for k in want:
        same("k_binarize_masks %s %s" % (name, k), got[k], exp[k])


@pytest.mark.parametrize("name", K.COUNT)
def test_count(diarizer, name):
    exp_cnt, exp_avg = K.count_expected(name)
    cnt, avg = diarizer.count_case(K.count_case(name), want_avg=True, fcanary=FC, icanary=IC)
    same("k_count %s count" % name, cnt, exp_cnt)
    same("k_count %s avg" % name, avg, exp_avg)
    cnt, avg = diarizer.count_case(K.count_case(name), want_avg=False, fcanary=FC, icanary=IC)
    assert avg is None
    same("k_count %s count, no avg" % name, cnt, exp_cnt)


# ---------------------------------------------------------------- cluster.hip
@pytest.mark.parametrize("name", K.GATHER)
def test_gather_normalize(diarizer, name):
    X, tidx, want = K.gather_case(name)
    exp_xo, exp_xn = K.gather_expected(name)
    xo, xn = diarizer.gather_normalize_case(X, tidx, want_xout=want, fcanary=FC)
    same("k_gather_normalize %s Xn" % name, xn, exp_xn)
    if want:
        same("k_gather_normalize %s Xout" % name, xo, exp_xo)
    else:
        assert xo is None


def test_gather_normalize_both_forms(diarizer):
    X, tidx, _ = K.gather_case("N129_d3")
    exp_xo, exp_xn = K.gather_expected("N129_d3")
    same("Xn without Xout", diarizer.gather_normalize_case(X, tidx, want_xout=False, fcanary=FC)[1], exp_xn)
    refused(lambda: diarizer.gather_normalize_case(X, np.array([0, len(X)], np.int32)))
    refused(lambda: diarizer.gather_normalize_case(X, np.array([-1], np.int32)))


@pytest.mark.parametrize("name", K.MEANS)
def test_cluster_means(diarizer, name):
    X, order, off = K.means_case(name)
    same("k_cluster_means %s" % name, diarizer.cluster_means_case(X, order, off, fcanary=FC), K.means_expected(name))


def test_cluster_means_refusals(diarizer):
    X, order, off = K.means_case("d1")
    bad = order.copy()
    bad[7] = len(X)
    refused(lambda: diarizer.cluster_means_case(X, bad, off))
    refused(lambda: diarizer.cluster_means_case(X, order[:17], np.array([0, 9, 5, 17], np.int32)))
    refused(lambda: diarizer.cluster_means_case(X, order[:17], np.array([1, 17], np.int32)))


@pytest.mark.parametrize("name", K.ASSIGN)
def test_assign(diarizer, name):
    E, cen = K.assign_case(name)
    exp = K.assign_expected(name)
    hard, err, soft, best = diarizer.assign_case(E, cen, fcanary=FC, icanary=IC)
    for k, v in (("hard", hard), ("err", err), ("soft", soft), ("best", best)):
        same("k_assign %s %s" % (name, k), v, exp[k])
    assert err[0] == ("zero" in name)


@pytest.mark.parametrize("want_soft,want_best", [(False, False), (True, False), (False, True)])
def test_assign_optional_tables(diarizer, want_soft, want_best):
    name = "M7_d192_K5"
    E, cen = K.assign_case(name)
    exp = K.assign_expected(name)
    hard, err, soft, best = diarizer.assign_case(E, cen, want_soft=want_soft, want_best=want_best, fcanary=FC, icanary=IC)
    same("hard", hard, exp["hard"])
    same("err", err, exp["err"])
    assert (soft is None) == (not want_soft) and (best is None) == (not want_best)
    if want_soft:
        same("soft", soft, exp["soft"])
    if want_best:
        same("best", best, exp["best"])


@pytest.mark.parametrize("name", K.CONSTRAINED)
def test_constrained_argmax(diarizer, name):
    soft = K.constrained_case(name)
    same("k_constrained_argmax %s" % name, diarizer.constrained_argmax_case(soft, R.nan_fill(soft), icanary=IC), K.constrained_expected(name))


def test_constrained_argmax_refusals(diarizer):
    refused(lambda: diarizer.constrained_argmax_case(np.zeros((2, 3, 65)), 0.0))


# ---------------------------------------------------------------- reconstruct.hip
@pytest.mark.parametrize("name", K.ACTIVATIONS)
def test_activations(diarizer, name):
    seg, hard, Kc = K.activations_case(name)
    nact, _ = R.activation_frames(len(seg))
    same("k_activations %s" % name, diarizer.activations_case(seg, hard, Kc, nact, fcanary=FC), K.activations_expected(name))


@pytest.mark.parametrize("name", K.TOPK)
def test_topk(diarizer, name):
    act, count, ar0, cr0, rows, crow = K.topk_case(name)
    same("k_topk %s" % name, diarizer.topk_case(act, count, ar0, cr0, rows, crow), K.topk_expected(name))


def test_topk_refusals(diarizer):
    act, count, ar0, cr0, rows, crow = K.topk_case("K3")
    refused(lambda: diarizer.topk_case(act, count, ar0, cr0, len(act) - ar0 + 1, crow))
    refused(lambda: diarizer.topk_case(act, count, ar0, cr0, rows, rows + 1))
    refused(lambda: diarizer.topk_case(act, count, ar0, len(count) - crow + 1, rows, crow))
    refused(lambda: diarizer.topk_case(act, count, -1, cr0, rows, crow))


# ---------------------------------------------------------------- cut.hip
@pytest.mark.parametrize("name", K.CUTS)
def test_assign_cuts(diarizer, name):
    E, cen, coff, slot, n_slots, nact = K.cuts_case(name)
    exp = K.cuts_expected(name)
    m2, hard, best, err = diarizer.assign_cuts_case(E, cen, coff, slot, n_slots, nact, fcanary=FC, icanary=IC)
    for k, v in (("m2", m2), ("hard", hard), ("best", best), ("err", err)):
        same("k_assign_cuts %s %s" % (name, k), v, exp[k])
    # each cut is k_assign on its own table
    M = len(E)
    for q in (0, len(slot) // 2, len(slot) - 1):
        h1, e1, _, b1 = R.assign(E, cen[coff[q]:coff[q + 1]])
        same("cut %d of %s: hard" % (q, name), hard[slot[q] * M:(slot[q] + 1) * M], R.mark_inactive(h1, nact))
        same("cut %d of %s: best" % (q, name), best[q * M:(q + 1) * M], b1)


def test_assign_cuts_zero_centroid_and_refusals(diarizer):
    E, cen, coff, slot, n_slots, nact = K.cuts_case("T65")
    cen = cen.copy()
    cen[int(coff[40])] = 0.0
    m2, hard, best, err = diarizer.assign_cuts_case(E, cen, coff, slot, n_slots, nact, fcanary=FC, icanary=IC)
    em2, ehard, ebest, eerr = R.assign_cuts(E, cen, coff, slot, n_slots, nact)
    assert err[0] == 1 == eerr and (err[1:] == IC).all()
    same("best beside a zero centroid", best[:-K.SLACK], ebest)
    for s_, h in enumerate(ehard):
        if h is not None:
            same("hard beside a zero centroid", hard[s_ * len(E):(s_ + 1) * len(E)], h)
    dup = slot.copy()
    dup[1] = dup[0]
    refused(lambda: diarizer.assign_cuts_case(E, cen, coff, dup, n_slots, nact))
    flat = coff.copy()
    flat[3] = flat[2]
    refused(lambda: diarizer.assign_cuts_case(E, cen, flat, slot, n_slots, nact))


@pytest.mark.parametrize("name", K.RECON)
def test_recon_cuts(diarizer, name):
    seg, hard, koff, count, ar0, cr0, rows, crow, act_in = K.recon_case(name)
    nact, _ = R.activation_frames(len(seg))
    exp_act, exp_bin = K.recon_expected(name)
    act, binary = diarizer.recon_cuts_case(seg, hard, koff, nact, count, ar0, cr0, rows, crow, act_in=act_in, fcanary=FC)
    same("k_activations_cuts %s" % name, act, exp_act)
    same("k_topk_cuts %s" % name, binary, exp_bin)


# ---------------------------------------------------------------- pipeline.cpp
@pytest.mark.parametrize("n", K.CAST_N)
def test_casts(diarizer, n):
    pcm, a, hard, nact = K.cast_case(n)
    exp_wav, exp_f64, exp_hard = K.cast_expected(n)
    wav = diarizer.pcm_to_f32_case(pcm, fcanary=FC)
    same("k_pcm_to_f32 n=%d" % n, wav, exp_wav)
    assert not wav[n:n + 512].any() and (wav[n + 512:] == np.float32(FC)).all()      # the pad is zero, what lies behind it is canary
    same("k_f32_to_f64 n=%d" % n, diarizer.f32_to_f64_case(a, fcanary=FC), exp_f64)
    same("k_mark_inactive n=%d" % n, diarizer.mark_inactive_case(hard, nact, icanary=IC), exp_hard)


# ---------------------------------------------------------------- the stage at d = 1 025
def test_clustering_of_wide_rows(diarizer):
    emb = K.wide_clustering_case(1025)
    ref_hard, ref_K, _ = orc.clustering(emb)
    hard, Kc = diarizer.clustering(emb)
    assert ref_K == 3 and Kc == ref_K and np.array_equal(np.asarray(hard).reshape(ref_hard.shape), ref_hard)
