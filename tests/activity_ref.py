"""float64 NumPy restatement of the activity stage (csrc/activity.hip) for tests/test_activity_ref.py and tests/test_activity.py:
pyannote's pre_aggregation_hook (largest = speech, second largest = overlap of the three local speakers), the overlap-add of
PipelineHelper::aggregate (sd.cpp:1167-1311) with skip_average = false, missing = 0.0, optionally Hamming-weighted (the branch
sd.cpp:1211-1215 leaves unimplemented), and the crop to the frames that do not lie wholly in the last chunk's zero padding."""
import functools

import numpy as np

import sdhip
import synth
from oracle import orc

KINDS = (sdhip.ACTIVITY_SPEECH, sdhip.ACTIVITY_OVERLAP)
NAMES = sdhip.ACTIVITY_KINDS            # ("speech", "overlap")
CHUNK_COUNTS = (1, 2, 10, 11, 12, 33)   # one chunk; two; the most that cover one frame is 11: one below, at, one above; several blocks of frames


def reduce_chunks(seg, kind):
    """[c][293][3] f32 -> [c][293] float64: the reduction in f32, widened afterwards; NaN where any of the three scores is NaN"""
    seg = np.asarray(seg, np.float32)
    bad = np.isnan(seg).any(-1)
    s = np.sort(np.where(bad[..., None], np.float32(0), seg), axis=-1)
    r = (s[..., 2] if kind == sdhip.ACTIVITY_SPEECH else s[..., 1]).astype(np.float64)
    r[bad] = np.nan
    return r


def num_frames(chunks):
    return orc.closest_frame(0.0 + 5.0 + (chunks - 1) * 0.5) + 1                 # sd.cpp:1232-1234


def rows_for(chunks, n_samples):
    return min(num_frames(chunks), orc.closest_frame(n_samples / 16000.0) + 1)


def aggregate_ref(reduced, hamming=False):
    """contributions added in ascending chunk order, one IEEE double operation at a time (NumPy does not contract)"""
    c = len(reduced)
    nf = num_frames(c)
    w = np.hamming(orc.FRAMES) if hamming else np.ones(orc.FRAMES)
    tot, cnt, msk = np.zeros(nf), np.zeros(nf), np.zeros(nf, bool)
    start = 0.0
    for i in range(c):
        sf = orc.closest_frame(start)                                             # sd.cpp:1251
        start += 0.5                                                              # sd.cpp:1253
        k = min(orc.FRAMES, nf - sf)
        ok = ~np.isnan(reduced[i][:k])
        tot[sf:sf + k] += np.where(ok, reduced[i][:k], 0.0) * np.where(ok, w[:k], 0.0)
        cnt[sf:sf + k] += np.where(ok, w[:k], 0.0)
        msk[sf:sf + k] |= ok
    out = tot / np.maximum(cnt, np.finfo(np.float64).eps)                         # sd.cpp:1288
    out[~msk] = 0.0                                                               # missing, sd.cpp:1302
    return out


def oracle_scores(seg, kind):
    """the contract: orc.aggregate of the reduced scores"""
    return orc.aggregate(reduce_chunks(seg, kind)[..., None], 0.0, 0.5, 5.0, missing=0.0)[:, 0]


def oracle_regions(scores, onset=0.5, offset=0.5, min_on=0.0, min_off=0.0, label=0):
    t = orc.to_annotation(np.asarray(scores, np.float64).reshape(-1, 1), 0.0, onset=onset, offset=offset, min_on=min_on, min_off=min_off)
    return [(a, b, label) for a, b, _ in t]


def random_scores(c, seed, nan_fraction=0.02):
    rng = np.random.default_rng(seed)
    seg = rng.random((c, orc.FRAMES, 3), dtype=np.float32)
    seg[rng.random(seg.shape) < nan_fraction] = np.nan
    return seg


@functools.lru_cache(maxsize=None)
def planted_120s():
    """the planted 120 s recording: (pcm, planted scores [chunks][293][3]); computed once, treat as read-only"""
    sec = 120.0
    pcm = synth.make_pcm(sec, seed=5)
    n = len(pcm)
    sc, _ = synth.planted_scores(synth.with_duets(synth.schedule(sec, 5)), n, 0, synth.num_chunks(n))
    pcm.setflags(write=False)
    sc.setflags(write=False)
    return pcm, sc
