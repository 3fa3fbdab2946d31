"""CPU side of tests/test_backend_kernels.py: the references of tests/backend_ref.py equal the oracle's stage functions where both apply, and each of
the single mistakes of backend_ref.MISTAKES, planted in a reference, changes at least one byte of at least one case of tests/backend_cases.py -- the
cases the GPU file runs, compared there byte for byte over the whole returned buffers."""
import numpy as np
import pytest

import backend_cases as K
import backend_ref as R
from oracle import orc


def _arrays(x):
    if isinstance(x, dict):
        return [x[k] for k in sorted(x)]
    return [a for a in (x if isinstance(x, tuple) else (x,)) if a is not None]


def same_bytes(a, b):
    a, b = _arrays(a), _arrays(b)
    return len(a) == len(b) and all(p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes() for p, q in zip(a, b))


# ---------------------------------------------------------------- the references are the oracle's
@pytest.mark.parametrize("name", K.BINARIZE)
def test_binarize_is_the_oracle(name):
    seg = K.binarize_case(name)
    b = R.binarize_bits(seg)
    assert np.array_equal(R.select_masks(b).view(np.int32), orc.select_masks(b.astype(np.float64)).view(np.int32))
    hard = np.arange(b.shape[0] * 3, dtype=np.int32).reshape(-1, 3) % 5
    nact = R.binarize(seg)[2]
    assert np.array_equal(R.mark_inactive(hard.reshape(-1), nact).reshape(-1, 3), orc.mark_inactive(b.astype(np.float64), hard))


def test_binarize_cases_hold_what_they_claim():
    b, masks, nact = R.binarize(K.binarize_case("c2_edges"))
    keep = b[0].sum(-1) < 2
    assert (b[0, :, 0] * keep).sum() == 3 and (b[0, :, 1] * keep).sum() == 4 and nact[:3].tolist() == [23, 24, 0]
    assert masks[0].sum() == 23 and masks[1].sum() == 4                       # the raw mask at 3 clean frames, the clean one at 4
    o = np.float32(R.ONSET)
    assert float(o) != R.ONSET and float(np.nextafter(o, np.float32(1))) > R.ONSET > float(np.nextafter(o, np.float32(0)))
    b1 = R.binarize(K.binarize_case("c1_all_on"))
    assert b1[0].all() and b1[1].all() and (b1[2] == 293).all()
    b65 = R.binarize(K.binarize_case("c65"))[0]
    assert not b65[7, :, 1].any() and b65[9].all() and 0 < b65[64].sum() <= 27


@pytest.mark.parametrize("name", K.COUNT)
def test_count_is_the_oracle(name):
    b = K.count_case(name)
    cnt, avg = R.count(b)
    ref, _, ft = orc.speaker_count(b.astype(np.float64))
    assert ft == R.FT and len(ref) == R.count_frames(b.shape[0]) and np.array_equal(cnt, ref)


def test_count_cases_hold_exact_halves():
    for name, half in (("c2_half_05", 0.5), ("c2_half_15", 1.5), ("c2_half_25", 2.5), ("c40_half", 0.5), ("c40_half", 1.5)):
        cnt, avg = R.count(K.count_case(name))
        assert (avg == half).any() and (cnt[avg == half] == 2 * round(half / 2)).all(), name


def test_clustering_references_are_the_oracle():
    """gather_normalize's copy, cluster_means and assign (scores, arg-max) against orc.clustering_full on three talkers with NaN rows"""
    emb = K.wide_clustering_case(192)
    hard, nk, soft = orc.clustering_full(emb)
    _, _, tl = orc.clustering(emb)
    E = emb.reshape(-1, 192)
    tidx = np.flatnonzero(~np.isnan(E[:, 0]))
    X, _ = R.gather_normalize(E, tidx)
    assert nk == 3 and len(tl) == len(tidx) and set(tl) == {0, 1, 2}
    order = np.concatenate([np.flatnonzero(tl == k) for k in range(nk)])
    off = np.concatenate([[0], np.cumsum([(tl == k).sum() for k in range(nk)])])
    cen = R.cluster_means(X, order, off)
    my_hard, err, my_soft, best = R.assign(E, cen)
    assert err == 0 and my_soft.tobytes() == soft.reshape(-1, nk).tobytes() and np.array_equal(my_hard, hard.reshape(-1))
    live = ~np.isnan(E[:, 0])
    assert np.array_equal(best[live], my_soft[live].max(1)) and np.isnan(best[~live]).all() and (my_hard[~live] == 0).all()


def test_unit_rows_cluster_as_the_oracles():
    """the oracle normalises inside orc.cluster_embeddings (the same f32-rounded norm) and shows only labels: the cut of the dendrogram of the reference's
    unit rows gives its clusters.  The bits of the f32 rounding themselves are held by the special rows of backend_cases.gather_case."""
    E = K.wide_clustering_case(192).reshape(-1, 192)
    tidx = np.flatnonzero(~np.isnan(E[:, 0]))
    X, Xn = R.gather_normalize(E, tidx)
    assert np.array_equal(X, E[tidx]) and np.allclose(np.sqrt((Xn * Xn).sum(1)), 1.0, atol=1e-6)
    lab, nk = orc.cluster_embeddings(X)
    T, _ = orc.ahc(Xn, orc.THRESH_F32)
    big = [t for t in np.unique(T) if (T == t).sum() >= 5]
    assert nk == len(big) == 3
    for t in big:
        assert len(set(lab[T == t])) == 1


@pytest.mark.parametrize("chunks", [1, 12, 40])
def test_reconstruction_references_are_the_oracle(chunks):
    """activations over all chunks, the crop and topk against orc.reconstruct (finite scores: the oracle's tensor marks a missing speaker with NaN)"""
    seg, hard, K_ = K.activations_case("c%d_K3" % chunks)
    seg = np.nan_to_num(seg, nan=0.25, neginf=0.0)
    b = (K.rng(99, chunks).random((chunks, R.FRAMES, 3)) < 0.4).astype(np.float64)
    cnt, cwin, ft = orc.speaker_count(b)
    Kr = int(hard.max()) + 1
    ref, _ = orc.reconstruct(seg, hard, cnt, cwin, ft, (chunks - 1) * 8000 + 80000)
    ar0, cr0, rows, crow = R.crop_ranges(chunks)
    got = R.topk(R.activations(seg, hard, Kr), cnt, ar0, cr0, rows, crow)
    assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.uint8))


# ---------------------------------------------------------------- every mistake shows
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_a_mistake_changes_a_byte_of_a_case(mistake):
    shown = []
    for fam in K.SHOWN_BY[mistake]:
        names, expected = K.FAMILIES[fam]
        shown += ["%s/%s" % (fam, n) for n in names if not same_bytes(expected(n), expected(n, mistake))]
    print("%-24s changes %d cases: %s" % (mistake, len(shown), " ".join(shown)))
    assert shown, "%s changes no byte of any case of %s" % (mistake, K.SHOWN_BY[mistake])


def test_every_mistake_is_listed():
    assert set(K.SHOWN_BY) == set(R.MISTAKES) and len(R.MISTAKES) == 12
