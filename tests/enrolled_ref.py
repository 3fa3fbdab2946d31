"""float64 reference of the enrolled flow of the clustering stage (include/sdhip.h, "enrolled speakers", steps 1 - 9) in numpy: nearest voiceprint by
the sequential cosine distance of tests/speakers_ref.py, claim, the oracle's linkage on what is left, the reference's float minVal loop over the
candidates, sequential means, assignment over the table [used voiceprints, new means].  `mistake` swaps exactly one rule for a plausible wrong one, so that
tests/test_enrolled_ref.py can show that the committed cases tell the two apart."""
import numpy as np

from oracle import orc

import speakers_ref as sr

MISTAKES = ("last minimum", "strict claim", "mcs from unclaimed", "candidates reversed")


def sequential_sqnorm(X):
    s = np.zeros(len(X), np.float64)
    for i in range(X.shape[1]):
        s = s + X[:, i] * X[:, i]
    return s


def normalize_f32(X):
    """rows divided by their norm rounded to float32 (Helper::L2Norm returns float, sd.cpp:332-340); a zero row stays"""
    nrm = np.sqrt(sequential_sqnorm(X)).astype(np.float32).astype(np.float64)
    return np.where(nrm[:, None] != 0.0, X / np.where(nrm == 0.0, 1.0, nrm)[:, None], X)


def cos_dist(a, b):
    return float(sr.cosine_distances(a[None], b[None])[0, 0])


def nearest(X, V, mistake=None):
    """step 1: (g [N] int32, dist [N]): the first minimum over the gallery rows of the sequential cosine distance"""
    D = sr.cosine_distances(X, V)
    if mistake == "last minimum":
        g = D.shape[1] - 1 - np.argmin(D[:, ::-1], 1)
    else:
        g = np.argmin(D, 1)
    return g.astype(np.int32), D[np.arange(len(X)), g]


def assign(flat, table, constrained=False):
    """step 8: every row of flat [M][d] over the table [K][d]: soft = 2 - distance, first maximum wins, a row without an embedding -> 0"""
    M, K = len(flat), len(table)
    ok = ~np.isnan(flat[:, 0])
    soft = np.full((M, K), np.nan)
    soft[ok] = 2.0 - sr.cosine_distances(table, flat[ok]).T
    hard = np.zeros(M, np.int32)
    hard[ok] = np.argmax(soft[ok], 1)
    if constrained:
        hard = orc.constrained_argmax(soft.reshape(M // 3, 3, K)).reshape(-1)
    return hard, soft


def clustering(emb, gallery, t, threshold=orc.THRESH_F32, min_cluster_size=orc.MIN_CLUSTER_SIZE, constrained=False, mistake=None):
    """emb [c][3][d] float64 with NaN rows, gallery [M][d], t = speaker_match_threshold -> dict: hard [c][3], K, centroids [K][d], counts [K],
    enrolled [K] (gallery row or -1), and the intermediate facts g, dist, claimed [N], G, L, n_unclaimed, to_enrolled (small clusters that went to a
    voiceprint)"""
    emb = np.ascontiguousarray(emb, np.float64)
    c, S, d = emb.shape
    flat = emb.reshape(-1, d)
    V = np.ascontiguousarray(gallery, np.float64)
    train = np.flatnonzero(~np.isnan(flat[:, 0]))
    N = len(train)
    X = flat[train]
    out = {"N": N}
    if N == 0:
        g, dist, claimed = np.zeros(0, np.int32), np.zeros(0), np.zeros(0, bool)
    else:
        g, dist = nearest(X, V, mistake)                                                   # 1
        claimed = dist < t if mistake == "strict claim" else dist <= t                      # 2
    U = sorted(set(int(m) for m in g[claimed]))                                             # 3
    G = len(U)
    out.update(g=g, dist=dist, claimed=claimed, G=G)
    if G == 0:
        hard, K, tl = orc.clustering(emb, threshold=threshold, min_cluster_size=min_cluster_size)
        if constrained:
            hard, K, _ = orc.clustering_full(emb, constrained=True, threshold=threshold, min_cluster_size=min_cluster_size)
        cen, cnt = sr.centroids(emb, tl)
        out.update(hard=hard, K=K, centroids=cen, counts=cnt, enrolled=np.full(K, -1, np.int32), L=K, n_unclaimed=N, to_enrolled=0, train_labels=tl)
        return out
    R = np.flatnonzero(~claimed)                                                            # 4 (indices into the train rows)
    N1 = len(R)
    mcs = min(min_cluster_size, max(1, int(np.floor(0.1 * (N1 if mistake == "mcs from unclaimed" else N) + 0.5))))      # std::round
    XR = X[R]
    if N1 >= 2:                                                                             # 5
        lab = orc.ahc(normalize_f32(XR), float(threshold))[0].astype(np.int64) - 1
    else:
        lab = np.zeros(N1, np.int64)
    nl = int(lab.max()) + 1 if N1 else 0
    sizes = np.bincount(lab, minlength=nl)
    large = [k for k in range(nl) if sizes[k] >= mcs]
    small = [k for k in range(nl) if 0 < sizes[k] < mcs]
    to_enrolled = 0
    if small:                                                                               # 6
        means = {k: sr.sequential_mean(XR[lab == k]) for k in range(nl)}
        cands = [("e", a, V[U[a]]) for a in range(G)] + [("l", k, means[k]) for k in large]
        if mistake == "candidates reversed":
            cands = [x for x in cands if x[0] == "l"] + [x for x in cands if x[0] == "e"]
        remap = {k: k for k in range(nl)}
        for sk in small:
            min_val, best = np.float32(np.finfo(np.float32).max), None                      # float minVal, dd < minVal (sd.cpp:2396)
            for kind, k, vec in cands:
                dd = cos_dist(vec, means[sk])
                if dd < float(min_val):
                    min_val, best = np.float32(dd), (kind, k)
            if best[0] == "e":
                remap[sk] = -1
                to_enrolled += 1
            else:
                remap[sk] = best[1]
        lab = np.array([remap[int(v)] for v in lab], np.int64)
    ids = sorted(set(int(v) for v in lab if v >= 0))                                        # 7
    L = len(ids)
    renum = {k: i for i, k in enumerate(ids)}
    lab = np.array([renum[int(v)] if v >= 0 else -1 for v in lab], np.int64)
    new_means = [sr.sequential_mean(XR[lab == k]) for k in range(L)]
    table = np.stack([V[m] for m in U] + new_means)                                         # 8
    hard, _ = assign(flat, table, constrained)
    counts = [int((g[claimed] == m).sum()) for m in U] + [int((lab == k).sum()) for k in range(L)]      # 9
    out.update(hard=hard.reshape(c, S), K=G + L, centroids=table, counts=np.array(counts, np.int64),
               enrolled=np.array(U + [-1] * L, np.int32), L=L, n_unclaimed=N1, to_enrolled=to_enrolled)
    return out


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share (computed once, read-only)
def far_row(cen):
    """a direction far from every centroid: the negative of their sum"""
    return -np.asarray(cen).sum(0)[None]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_CACHE = {}


def case(name):
    """(emb [40][3][192], gallery, t) of a named case; every threshold comes from the reference's own distances, never from the code under test"""
    if name in _CACHE:
        return _CACHE[name]
    small = 5 if "small" in name else 0
    emb = sr.planted_embeddings(chunks=40, clusters=3, small=small)
    flat = emb.reshape(-1, sr.DIM)
    X = flat[~np.isnan(flat[:, 0])]
    _, K, tl = orc.clustering(emb)
    cen, _ = sr.centroids(emb, tl)
    assert K == 3
    base = name.replace(" small", "")
    if base == "far":                              # nobody is claimed: the plain job
        gal, t = far_row(cen), 0.0
    elif base == "closed":                         # the plain job's own centroids, shuffled; everything is claimed
        gal, t = cen[[2, 0, 1]].copy(), 2.0
    elif base == "hybrid":                         # two of the three centroids and a far row; t = the largest distance of the rows near a voiceprint
        gal = np.vstack([cen[[1, 2]], far_row(cen)])
        dist = nearest(X, gal)[1]
        t = float(np.sort(dist)[int((dist < 0.5).sum()) - 1])
    elif base == "partial":                        # the same gallery, t = the 30 % quantile of the nearest distances: the voiceprints claim the core of
        gal = np.vstack([cen[[1, 2]], far_row(cen)])          # their clusters, the fringe is left over as small clusters
        dist = nearest(X, gal)[1]
        t = float(np.sort(dist)[int(0.3 * len(dist))])
    elif base == "one row":                        # t = exactly the smallest nearest distance: that row alone is claimed
        gal = np.vstack([cen[[1, 2]], far_row(cen)])
        t = float(nearest(X, gal)[1].min())
    elif base == "duplicates":                     # the same voiceprint twice: the first index must win
        gal, t = cen[[2, 0, 2, 1, 0]].copy(), 2.0
    elif base == "one left":                       # N' = 1: t = the second largest nearest distance
        gal = cen[[1, 2]].copy()
        t = float(np.sort(nearest(X, gal)[1])[-2])
    elif base == "tie":
        # one voiceprint e = 2 * mean(C): the same cosine distances as that mean, bit for bit (every sum doubles or quadruples exactly).  e itself is
        # planted as one more embedding row, which e claims alone (t = its own distance, about 0); C is then a large leftover cluster whose mean ties
        # with e for the small cluster, and the order of the candidates decides
        assert small
        lab4, K4 = orc.cluster_embeddings(X, min_cluster_size=1)
        assert K4 == 4
        sizes = np.bincount(lab4)
        s_id = int(np.argmin(sizes))
        assert sizes[s_id] == 5
        s_mean = sr.sequential_mean(X[lab4 == s_id])
        c_id = min((k for k in range(4) if k != s_id), key=lambda k: cos_dist(sr.sequential_mean(X[lab4 == k]), s_mean))
        e = 2.0 * sr.sequential_mean(X[lab4 == c_id])
        emb = emb.copy()
        dead = np.flatnonzero(np.isnan(emb.reshape(-1, sr.DIM)[:, 0]))
        emb.reshape(-1, sr.DIM)[dead[len(dead) // 2]] = e
        gal, t = e[None].copy(), max(0.0, cos_dist(e, e))
        assert np.sort(sr.cosine_distances(X, gal)[:, 0])[0] > 1e-3
    else:
        raise KeyError(name)
    _CACHE[name] = _freeze(emb, np.ascontiguousarray(gal, np.float64)) + (t,)
    return _CACHE[name]


CASES = ("far", "far small", "closed", "closed small", "hybrid", "hybrid small", "partial", "partial small", "one row", "duplicates", "one left", "tie small")
