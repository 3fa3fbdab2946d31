"""CPU tests of the activity stage's contract (include/sdhip.h: sd_activity*): the float64 restatement the GPU tests lean on equals the oracle's
aggregate bit for bit, the Hamming form is far enough from it for the GPU tolerance to tell the two apart, the crop rule, the planted 120 s
anchor from the committed oracle, the exported symbols and the command line's usage errors.  Nothing here needs a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import sdhip
from oracle import orc

import activity_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")


@pytest.mark.parametrize("c", ar.CHUNK_COUNTS)
def test_restatement_equals_the_oracle_aggregate_bit_for_bit(c):
    seg = ar.random_scores(c, seed=100 + c)
    assert np.isnan(seg).any()
    for kind in ar.KINDS:
        red = ar.reduce_chunks(seg, kind)
        assert np.array_equal(np.isnan(red), np.isnan(seg).any(-1))
        got = ar.aggregate_ref(red)
        ref = ar.oracle_scores(seg, kind)
        assert got.shape == ref.shape == (ar.num_frames(c),)
        assert np.array_equal(got, ref) and not np.isnan(ref).any()
    # the two reductions on numbers: largest and second largest
    ok = ~np.isnan(seg).any(-1)
    assert np.array_equal(ar.reduce_chunks(seg, 0)[ok], seg[ok].max(-1).astype(np.float64))
    assert np.array_equal(ar.reduce_chunks(seg, 1)[ok], np.median(seg[ok], axis=-1).astype(np.float64))


@pytest.mark.parametrize("c", ar.CHUNK_COUNTS)
def test_hamming_form_differs_from_the_unweighted_one(c):
    """... by more than 1e-6 somewhere: six orders above the 1e-12 the GPU's Hamming form is held to (tests/test_activity.py)"""
    seg = ar.random_scores(c, seed=100 + c)
    for kind in ar.KINDS:
        red = ar.reduce_chunks(seg, kind)
        gap = np.abs(ar.aggregate_ref(red, hamming=True) - ar.aggregate_ref(red)).max()
        if c == 1:
            assert gap < 1e-15          # one chunk: every frame has one contribution, and w r / w = r
        else:
            assert gap > 1e-6, gap


def test_a_missing_frame_is_zero_and_an_all_nan_chunk_contributes_nothing():
    seg = ar.random_scores(12, seed=3, nan_fraction=0.0)
    seg[5] = np.nan                        # a chunk that is all NaN
    seg[0, 17, 1] = np.nan                 # output frame 17 is covered by chunk 0 alone (chunk 1 starts at frame 29): missing
    assert orc.closest_frame(0.5) == 29
    for kind in ar.KINDS:
        red = ar.reduce_chunks(seg, kind)
        ref = ar.oracle_scores(seg, kind)
        assert ref[17] == 0.0 and ref[16] == red[0, 16]
        assert np.array_equal(ar.aggregate_ref(red), ref)
        only5 = np.full_like(red, np.nan)
        only5[5] = red[5]
        assert np.array_equal(ar.aggregate_ref(only5), np.zeros(ar.num_frames(12)))


@pytest.mark.parametrize("n,chunks,rows", [(80000, 1, 297), (80001, 2, 297), (88000, 2, 326), (1920000, 231, 7112)])
def test_crop_rule(n, chunks, rows):
    assert orc.num_chunks(n)[0] == chunks == sdhip.num_chunks(n)[0]
    nf = ar.num_frames(chunks)
    assert ar.rows_for(chunks, n) == rows == min(nf, orc.closest_frame(n / 16000.0) + 1)
    assert rows <= nf
    # the last frame kept starts inside the audio, the first one dropped (if any) lies wholly behind it
    assert (rows - 1) * orc.FRAME_STEP < n / 16000.0
    if rows < nf:
        assert rows * orc.FRAME_STEP >= n / 16000.0 - 0.5 * orc.FRAME_STEP


def test_planted_anchor_from_the_oracle():
    """the planted 120 s recording with the default options: 7112 rows, 35 speech and 4 overlap regions, asserted from the committed oracle"""
    pcm, sc = ar.planted_120s()
    n = len(pcm)
    assert n == 1920000 and sc.shape == (231, 293, 3)
    rows = ar.rows_for(len(sc), n)
    assert rows == 7112
    speech = ar.oracle_regions(ar.oracle_scores(sc, sdhip.ACTIVITY_SPEECH)[:rows])
    overlap = ar.oracle_regions(ar.oracle_scores(sc, sdhip.ACTIVITY_OVERLAP)[:rows])
    assert len(speech) == 35 and len(overlap) == 4
    assert speech[0][:2] == (0.2109375, 2.9784375) and overlap[0][:2] == (0.2109375, 0.4978125)
    # overlap is a property of the scores, not of the turns: every overlap region lies inside a speech region
    for a, b, _ in overlap:
        assert any(s <= a and b <= e for s, e, _ in speech)


def test_to_annotation_quirks_the_library_reproduces():
    """the oracle's state machine on the cases the scan has to get right: strict comparisons, the toggle of offset > onset, NaN, the initial state,
    the open last region, removeShort sparing the first region (sd.cpp:943-953)"""
    ts = lambda i: (i * orc.FRAME_STEP + (i * orc.FRAME_STEP + orc.FRAME_STEP)) / 2
    assert ar.oracle_regions([0.5, 0.5, 0.5]) == []                                           # == onset is not > onset
    assert ar.oracle_regions([0.9, 0.5, 0.5]) == [(ts(0), ts(2), 0)]                          # == offset is not < offset
    assert ar.oracle_regions([0.5] * 4, onset=0.4, offset=0.6) == [(ts(0), ts(1), 0), (ts(2), ts(3), 0)]      # strictly between: toggles
    assert ar.oracle_regions([np.nan, 0.9, np.nan, 0.1]) == [(ts(1), ts(3), 0)]               # NaN: initial state inactive, then the identity
    assert ar.oracle_regions([0.1, 0.1, 0.9]) == [(ts(2), ts(2), 0)]                          # opened on the last frame: an empty region
    short_first = [0.9, 0.1] + [0.1] * 40 + [0.9, 0.1] + [0.1] * 40 + [0.9] * 30
    assert len(ar.oracle_regions(short_first)) == 3
    assert [round(b - a, 6) for a, b, _ in ar.oracle_regions(short_first, min_on=0.3)] == [round(ts(1) - ts(0), 6), round(ts(113) - ts(84), 6)]


def test_symbols_are_exported_declared_and_cited():
    L = sdhip.lib()
    names = ["sd_activity_scores", "sd_activity_regions", "sd_activity", "sd_activity_dev", "sd_activity_f32", "sd_activity_wav", "sd_last_activity_scores"]
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    test_hdr = open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    for name in names:
        assert hasattr(L, name) and name in sdhip.EXPORTS
        assert re.search(r"^int %s\(" % name, hdr, re.M) and name not in test_hdr
    assert "sd.cpp:1167-1311" in hdr and "sd.cpp:2852-2935" in hdr and "sd.cpp:1211-1215" in hdr
    assert re.search(r"SD_ACTIVITY_SPEECH = 0, SD_ACTIVITY_OVERLAP = 1", hdr)
    assert (sdhip.ACTIVITY_SPEECH, sdhip.ACTIVITY_OVERLAP) == (0, 1)
    for name in ("activity_scores", "activity_regions", "activity", "activity_dev", "activity_f32", "activity_wav", "last_activity_scores", "set_activity"):
        assert callable(getattr(sdhip.Diarizer, name))


@pytest.mark.parametrize("args,needle", [
    (["--activity", "music"], "--activity takes speech or overlap"),
    (["--activity"], "--activity needs a value"),
    (["--activity", "speech", "--activity-onset", "0.5x"], "--activity-onset takes a number in [0, 1]"),
    (["--activity", "speech", "--activity-onset", "1.5"], "--activity-onset takes a number in [0, 1]"),
    (["--activity", "overlap", "--activity-offset", "-0.1"], "--activity-offset takes a number in [0, 1]"),
    (["--activity", "overlap", "--activity-offset", "nan"], "--activity-offset takes a number in [0, 1]"),
    (["--activity", "speech", "--activity-min-on", "abc"], "--activity-min-on takes a number of seconds >= 0"),
    (["--activity", "speech", "--activity-min-off", "-1"], "--activity-min-off takes a number of seconds >= 0"),
    (["--activity", "speech", "--activity-min-off"], "--activity-min-off needs a value"),
    (["--activity", "speech", "--gpus", "2"], "--gpus 2 is refused"),
])
def test_cli_usage_errors_need_no_gpu(args, needle):
    """a bad --activity value or an unparsable number ends the program with exit code 2 before any context is created; so does --gpus N"""
    out = subprocess.run([EXE, "seg.sdw", "emb.sdw", "audio.wav"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and needle in out.stderr and out.stdout == "", (out.returncode, out.stderr)
