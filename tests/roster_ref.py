"""The roster rule of include/sdhip.h (sd_roster_update) in plain Python and numpy: the reference the CPU and the GPU tests compare the library with,
bit for bit.  Sums are sequential, one dimension at a time (sd.cpp:476-498); nothing here is vectorised over the dimensions."""
import math

import numpy as np

T_DEFAULT = float(np.float32(0.7153814381597874)) ** 2 / 2          # option "speaker_match_threshold": t * t / 2
SD_ERR_NUMERIC = 5


class ZeroNorm(Exception):
    """a zero-norm centroid that step B had to read (SD_ERR_NUMERIC); the roster is unchanged"""


def cosine_distance(a, b):
    """1 - dot / (sqrt(m1) * sqrt(m2)), three sequential float64 sums in ascending dimension (sd.cpp:476-498); None for a zero norm"""
    dot = m1 = m2 = 0.0
    for x, y in zip(a.tolist(), b.tolist()):
        dot += x * y
        m1 += x * x
        m2 += y * y
    if m1 == 0.0 or m2 == 0.0:
        return None
    with np.errstate(all="ignore"):                                            # IEEE arithmetic at the edges, where Python's own division raises
        return float(1.0 - (np.float64(dot) / (np.sqrt(np.float64(m1)) * np.sqrt(np.float64(m2)))))


class Roster:
    """P entries: centroid cen[p] (float64 [d]), row count n[p], seen[p] = the index of the last update that gave p out (-1: loaded, never given out);
    updates = the update counter U"""

    def __init__(self, d):
        self.d = int(d)
        self.cen = np.zeros((0, self.d), np.float64)
        self.n = np.zeros(0, np.int64)
        self.seen = np.zeros(0, np.int64)
        self.updates = 0

    @property
    def P(self):
        return len(self.n)

    def load(self, cen, counts):
        assert self.P == 0                                                       # into an empty roster only
        self.cen = np.array(cen, np.float64).reshape(-1, self.d)
        self.n = np.where(np.isnan(self.cen[:, 0]), 0, np.array(counts, np.int64))   # a row whose first element is NaN has count 0
        self.seen = np.full(len(self.n), -1, np.int64)

    def table(self):
        """(centroids, counts, seen) as sd_roster_speakers returns them, and the update counter"""
        return self.cen.copy(), self.n.copy(), self.seen.copy(), self.updates

    def update(self, C, m, rows=None, prev=None, shift=0, t=T_DEFAULT):
        """C [K][d], m [K]; rows [M] hard labels of this job (< 0: none) and prev [Mp] ids of the previous update's rows (< 0: none), row i of this job
        being row i + shift of the previous one; -> ids [K] int32.  Raises ZeroNorm before anything is changed."""
        C = np.asarray(C, np.float64).reshape(-1, self.d)
        K, P = len(C), self.P
        live_k = [not math.isnan(C[k, 0]) for k in range(K)]
        m = [int(m[k]) if live_k[k] else 0 for k in range(K)]                    # a row whose first element is NaN has count 0
        ids = [-1] * K
        given = set()
        # A, rows: a speaker keeps the id his rows had
        if rows is not None and prev is not None:
            cnt = {}
            for i in range(len(rows)):
                j = i + shift
                if j >= len(prev):
                    break
                k, p = int(rows[i]), int(prev[j])
                if k >= 0 and p >= 0:
                    assert k < K and p < P
                    cnt[(k, p)] = cnt.get((k, p), 0) + 1
            for c, k, p in sorted((-c, k, p) for (k, p), c in cnt.items()):
                if ids[k] < 0 and p not in given:
                    ids[k] = p
                    given.add(p)
        # B, centroids: sd_match_speakers' rule over what is still free on both sides
        free_k = [k for k in range(K) if ids[k] < 0 and live_k[k]]
        free_p = [p for p in range(P) if p not in given and not math.isnan(self.cen[p, 0])]
        if free_k and free_p:
            pairs = []
            for k in free_k:
                for p in free_p:
                    v = cosine_distance(C[k], self.cen[p])
                    if v is None:
                        raise ZeroNorm((k, p))
                    if v <= t:
                        pairs.append((v, k, p))
            for v, k, p in sorted(pairs):
                if ids[k] < 0 and p not in given:
                    ids[k] = p
                    given.add(p)
        # C: new ids in ascending k
        new = [k for k in range(K) if ids[k] < 0]
        for q, k in enumerate(new):
            ids[k] = P + q
        if new:
            self.cen = np.concatenate([self.cen, np.zeros((len(new), self.d))])
            self.n = np.concatenate([self.n, np.zeros(len(new), np.int64)])
            self.seen = np.concatenate([self.seen, np.zeros(len(new), np.int64)])
        # D, refresh: an entry keeps the estimate made from the most rows; a tie goes to the later one
        for k in range(K):
            p = ids[k]
            if p >= P or m[k] >= self.n[p]:
                self.cen[p] = C[k]
                self.n[p] = m[k]
            self.seen[p] = self.updates
        self.updates += 1
        return np.array(ids, np.int32)


def relabel(turns, ids):
    """sd_relabel_turns_map: the label k of every turn becomes ids[k]; times and order stay"""
    return [(s, e, int(ids[k])) for s, e, k in turns]


def kept_rows(hard, ids):
    """what a stream keeps for its next update: ids[hard[i]] per row, -1 where the row has no label"""
    hard = np.asarray(hard).reshape(-1)
    ids = np.asarray(ids, np.int32)
    return np.where(hard >= 0, ids[np.clip(hard, 0, max(len(ids) - 1, 0))] if len(ids) else -1, -1).astype(np.int32)
