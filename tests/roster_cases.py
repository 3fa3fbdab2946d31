"""Shared inputs of tests/test_roster_cpu.py and tests/test_roster.py: the planted 75 s recording of tests/stream_cases.py pushed in pieces of 10 s, the
job the oracle sees at every prefix -- without a window and with a window of one block of 32 chunks -- and the roster reference run over those jobs.
Everything is computed once per session and handed out read-only."""
import functools

import numpy as np

import roster_ref
import speakers_ref
import stream_cases as sc
import synth
from oracle import orc

PIECE = 160000                                               # 10 s
PREFIXES = tuple(range(PIECE, 1120001, PIECE))               # 160 000 .. 1 120 000: seven updates
BLOCK = 256000                                               # samples of a block of 32 chunks


def origin_at(n, window):
    """samples a stream with sd_stream_set_window(window) has forgotten once n samples were pushed in pieces (the pieces never seal two blocks at once)"""
    if window is None:
        return 0
    return BLOCK * max(0, sc.sealed(n) // 32 - window)


@functools.lru_cache(maxsize=None)
def talkers():
    """[141][3] planted talker of every (chunk, local speaker), -1 = nobody"""
    _, assign = synth.planted_scores(synth.with_duets(synth.schedule(sc.SECONDS, sc.SEED)), sc.N, 0, sc.CHUNKS)
    a = assign.astype(np.int64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planted_job(origin, n):
    """what the oracle makes of samples [origin, n) with the planted rows of their chunks: (centroids [K][192], counts [K], hard [chunks * 3])"""
    scores, emb = sc.planted75()
    c0, nc = origin // sc.HOP, sc.total(n - origin)
    s = scores[c0:c0 + nc]
    e = emb[3 * c0:3 * (c0 + nc)].astype(np.float64)
    e[sc.nan_rows(s)] = np.nan
    hard, K, train_labels = orc.clustering(e.reshape(nc, 3, 192))
    hard = orc.mark_inactive(orc.binarize(s), hard).reshape(-1)
    cen, cnt = speakers_ref.centroids(e, train_labels)
    assert len(cen) == K
    for a in (cen, cnt, hard):
        a.setflags(write=False)
    return cen, cnt, hard


@functools.lru_cache(maxsize=None)
def planted_run(window):
    """the roster reference over the seven updates: a tuple of (n, origin, ids [K], hard [M], roster table after the update)"""
    r = roster_ref.Roster(192)
    out, prev, prev_origin = [], None, 0
    for n in PREFIXES:
        origin = origin_at(n, window)
        cen, cnt, hard = planted_job(origin, n)
        ids = r.update(cen, cnt, hard, prev, 3 * (origin - prev_origin) // sc.HOP)
        prev, prev_origin = roster_ref.kept_rows(hard, ids), origin
        out.append((n, origin, ids, hard, r.table()))
    return tuple(out)


def id_talkers(run):
    """{roster id: {talker: rows}} over all updates of a run, from the planted assignment of every row that carries a label"""
    seen = {}
    for n, origin, ids, hard, _ in run:
        who = talkers()[origin // sc.HOP:origin // sc.HOP + len(hard) // 3].reshape(-1)
        for h, t in zip(hard, who):
            if h >= 0 and t >= 0:
                seen.setdefault(int(ids[h]), {}).setdefault(int(t), 0)
                seen[int(ids[h])][int(t)] += 1
    return seen


def majority_map(run):
    """{id: talker}, the talker of an id in an update being the one that more than half of the id's labelled rows belong to (the assignment step puts a
    few rows of a duet or of a short turn with the wrong cluster: that is the clustering's error, which a roster neither makes nor mends); asserts
    that every id has such a talker in every update and never changes it"""
    fixed = {}
    for step in run:
        for i, talk in id_talkers((step,)).items():
            best = max(talk, key=talk.get)
            assert talk[best] * 2 > sum(talk.values()), (step[0], i, talk)
            assert fixed.setdefault(i, best) == best, (step[0], i, talk, fixed)
    return fixed
