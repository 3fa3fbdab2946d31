"""Reference of the "max_num_embeddings" rule (include/sdhip.h, options) in Python integers, and of a clustering call under it, built from
what is already pinned: the C oracle's clustering on the table with the unselected train rows masked out, the sequential means of
tests/speakers_ref.py and the sequential cosine assignment of tests/enrolled_ref.py (sd.cpp:476-498)."""
import numpy as np

from oracle import orc

import enrolled_ref as er
import speakers_ref as sr

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def fin(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def key(seed, i):
    """64-bit wrap-around arithmetic throughout; seed is taken modulo 2^64 (a negative seed is its two's complement)"""
    a = fin((seed + G) & MASK)
    return fin((a + i * G) & MASK)


def sample(rows, max_num, seed=0):
    """rows ascending -> the rows that stay, ascending: all of them under -1 or when there are no more than max_num, else those with the smallest keys"""
    rows = [int(r) for r in rows]
    if max_num == -1 or len(rows) <= max_num:
        return rows
    return sorted(sorted(rows, key=lambda i: key(seed, i))[:max_num])


def train_rows(emb):
    flat = np.asarray(emb, np.float64).reshape(-1, np.shape(emb)[-1])
    return np.flatnonzero(~np.isnan(flat[:, 0]))


def masked(emb, max_num, seed):
    """(the table with the unselected train rows set to NaN, the selected rows, all train rows)"""
    emb = np.array(emb, np.float64)
    flat = emb.reshape(-1, emb.shape[-1])
    train = train_rows(emb)
    sel = np.array(sample(train, max_num, seed), np.int64)
    drop = np.setdiff1d(train, sel)
    flat[drop] = np.nan
    return emb, sel, train


def sampled_clustering(emb, max_num, seed=0, constrained=False, gallery=None, t=None, **kw):
    """emb [c][3][d] float64 with NaN rows -> dict(hard [c][3], K, centroids [K][d], counts [K], selected, and under a gallery `enrolled`).
    1 select the sample; 2 the oracle on the table with the unselected train rows masked: K and the labels of the selected and of the NaN rows;
    3 centroids = sequential means over the selected rows; 4 every other train row: first arg-max of 2 - cosine distance.  constrained: the
    assignment of step 4 covers every row and goes through constrained_argmax, chunk by chunk (Clustering.py:81-94).  kw: orc.clustering's."""
    emb = np.ascontiguousarray(emb, np.float64)
    c, S, d = emb.shape
    flat = emb.reshape(-1, d)
    m_emb, sel, train = masked(emb, max_num, seed)
    out = {"selected": sel}
    if gallery is not None:
        res = er.clustering(m_emb, gallery, t, constrained=constrained, **kw)
        K, cen, cnt, hard_m = res["K"], res["centroids"], res["counts"], np.asarray(res["hard"]).reshape(-1)
        out["enrolled"] = res["enrolled"]
    else:
        hard_m, K, tl = orc.clustering(m_emb, **kw)
        if constrained:
            hard_m, K, _ = orc.clustering_full(m_emb, constrained=True, **kw)
        hard_m = hard_m.reshape(-1)
        K = max(int(K), 1)                                # the one-cluster exit (sd.cpp:2081-2088): the oracle returns 0, the library counts the cluster it describes
        cen, cnt = sr.centroids(m_emb, tl)
    hard, _ = er.assign(flat, cen, constrained)
    if not constrained:                                   # the sample's and the NaN rows' labels are the oracle's own
        keep = np.ones(len(flat), bool)
        keep[np.setdiff1d(train, sel)] = False
        hard[keep] = hard_m[keep]
    out.update(hard=hard.reshape(c, S), K=int(K), centroids=cen, counts=np.asarray(cnt, np.int64))
    return out
