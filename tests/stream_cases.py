"""Shared inputs of tests/test_stream.py and tests/test_stream_cpu.py: the 75 s recording (141 chunks: the smallest size that seals four blocks of
32 chunks and still leaves pending ones), its planted score / embedding tables -- row k serves chunk k of every prefix -- and the oracle's answer
on a prefix.  Everything is computed once per session and handed out read-only."""
import functools

import numpy as np

import synth
from oracle import orc, pipeline_oracle

SECONDS, SEED = 75.0, 1234
N, CHUNKS = 1200000, 141
CHUNK, HOP = 80000, 8000
# cumulative ends of the pushes of the prefix-equality test: both sides of the first chunk, of the second, and of the first two seals
PUSH_ENDS = (1, 2, 79999, 80000, 80001, 88000, 88001, 327999, 328000, 328001, 336001, 583999, 584001, 600123, 840000, 1200000)
# prefixes at which the planted case is compared (and shown not to be degenerate)
PLANTED_PREFIXES = (328000, 328001, 336001, 400000, 584001, 600123, 840000, 1000000, 1200000)


def full(n):
    """chunks k with k * 8000 + 80000 < n"""
    return 0 if n <= CHUNK else (n - CHUNK + HOP - 1) // HOP


def sealed(n):
    return 32 * (full(n) // 32)


def total(n):
    return orc.num_chunks(n)[0]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pcm75():
    pcm = synth.make_pcm(SECONDS, SEED)
    assert len(pcm) == N and total(N) == CHUNKS
    return _frozen(pcm)


@functools.lru_cache(maxsize=None)
def planted75():
    """(scores [141][293][3] f32, embeddings [423][192] f32) of the whole recording"""
    scores, assign = synth.planted_scores(synth.with_duets(synth.schedule(SECONDS, SEED)), N, 0, CHUNKS)
    emb = synth.planted_embeddings(assign, outlier_every=0)
    return _frozen(scores), _frozen(emb)


def nan_rows(scores):
    """rows the reference overwrites with NaN (sd.cpp:2479-2549), from the oracle's masks of these scores, batch of 32 items by batch"""
    masks = orc.select_masks(orc.binarize(scores))
    per_frame = np.bincount((np.arange(80000, dtype=np.int64) * 293) // 80000, minlength=293)
    counts = ((masks > 0.5) * per_frame[None, :]).sum(1).astype(np.int64)
    bad = np.zeros(len(counts), bool)
    for b0 in range(0, len(counts), 32):
        _, ts, an = orc.wav_lens(counts[b0:b0 + 32])
        bad[b0:b0 + 32] = ts | an
    return bad


@functools.lru_cache(maxsize=None)
def planted_oracle(n):
    """(turns, K) of the oracle on the first n samples with the planted tables' first total(n) rows"""
    scores, emb = planted75()
    nc = total(n)
    sc = scores[:nc]
    e = emb[:3 * nc].astype(np.float64)
    e[nan_rows(sc)] = np.nan
    turns, info = pipeline_oracle.diarize_ref(pcm75()[:n], None, None, seg_override=sc, emb_override=e, return_all=True)
    return tuple(turns), int(info["K"])
