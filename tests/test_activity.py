"""GPU tests of the activity stage (csrc/activity.hip; include/sdhip.h: sd_activity*): the aggregated speech / overlap timeline against the
oracle's aggregate bit for bit, the hysteresis scan against the oracle's to_annotation region for region at every tile and wave edge, and
the whole path -- device / host PCM, float samples, wav file, command line -- against the oracle applied to the same scores."""
import os
import re
import subprocess

import numpy as np
import pytest

import sdhip
from oracle import orc

import activity_ref as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
T = 1024             # ACT_TILE of csrc/activity.hip: frames per tile of the hysteresis scan = threads per workgroup (16 waves of 64)
WAVE = 64
ACTIVITY_KEYS = ("activity_onset", "activity_offset", "activity_min_duration_on", "activity_min_duration_off")


def test_tile_length_is_the_kernels():
    src = open(os.path.join(PKG, "csrc", "activity.hip")).read()
    assert int(re.search(r"^#define ACT_TILE (\d+)", src, re.M).group(1)) == T


@pytest.fixture
def act(diarizer):
    """the shared context with the activity options at their defaults before and after"""
    diarizer.set_activity()
    yield diarizer
    diarizer.set_activity()


# ------------------------------------------------------------------ sd_activity_scores
@pytest.mark.parametrize("c", ar.CHUNK_COUNTS)
def test_scores_equal_the_oracle_aggregate(act, c):
    seg = ar.random_scores(c, seed=100 + c)
    if c >= 10:
        seg[c // 2] = np.nan                                   # a chunk that is all NaN
    seg[0, 17, 1] = np.nan                                     # c <= 1 or not: output frame 17 belongs to chunk 0 alone -> missing
    for kind in ar.KINDS:
        got = act.activity_scores(seg, kind)
        ref = ar.oracle_scores(seg, kind)
        assert got.shape == ref.shape == (ar.num_frames(c),)
        assert np.array_equal(got, ref)
        assert got[17] == 0.0
    assert np.array_equal(act.activity_scores(seg, "overlap"), ar.oracle_scores(seg, sdhip.ACTIVITY_OVERLAP))      # kinds by name


@pytest.mark.parametrize("c", ar.CHUNK_COUNTS)
def test_hamming_scores_within_1e_12_of_the_float64_restatement(act, c):
    """at most 11 weighted terms in [0, 1]; the weights within a few ulp of NumPy's; the quotient within ~1e-14: 1e-12 leaves two orders of
    margin and sits six orders below the weighted / unweighted gap (tests/test_activity_ref.py)"""
    seg = ar.random_scores(c, seed=100 + c)
    if c >= 10:
        seg[c // 2] = np.nan
    act.set_option("activity_hamming", 1)
    for kind in ar.KINDS:
        got = act.activity_scores(seg, kind)
        ref = ar.aggregate_ref(ar.reduce_chunks(seg, kind), hamming=True)
        err = np.abs(got - ref).max()
        print("hamming c=%d kind=%d max abs err %.3e" % (c, kind, err))
        assert err <= 1e-12
        if c > 1:
            assert np.abs(got - ar.oracle_scores(seg, kind)).max() > 1e-6          # ... and it is the weighted form that ran
    act.set_option("activity_hamming", 0)
    assert np.array_equal(act.activity_scores(seg, 0), ar.oracle_scores(seg, 0))


# ------------------------------------------------------------------ sd_activity_regions
LENGTHS = list(range(1, 131)) + [T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 3]


def edge_timeline(n, shift, first_high):
    """high / low stretches that change exactly on the first (shift 0) or the last (shift -1) frame of every wave and tile"""
    edges = sorted({p + shift for p in list(range(WAVE, n + WAVE, WAVE)) + list(range(T, n + T, T)) if 0 < p + shift < n})
    v = np.empty(n)
    hi, prev = first_high, 0
    for p in edges + [n]:
        v[prev:p] = 0.9 if hi else 0.1
        hi, prev = not hi, p
    return v


def timelines(n, onset, offset, rng):
    nan5 = rng.random(n)
    nan5[rng.random(n) < 0.05] = np.nan
    yield "uniform", rng.random(n)
    yield "all above onset", np.full(n, max(onset, offset) + 0.25)
    yield "all below offset", np.full(n, min(onset, offset) - 0.25)
    yield "alternating", np.where(np.arange(n) % 2 == 0, 0.9, 0.1)
    yield "alternating from low", np.where(np.arange(n) % 2 == 1, 0.9, 0.1)
    yield "onset and offset themselves", rng.choice([onset, offset, np.nextafter(onset, 1.0), np.nextafter(offset, 0.0), 0.5 * (onset + offset), 0.1, 0.9], n)
    yield "5 % NaN", nan5
    for shift in (0, -1):
        for first_high in (False, True):
            yield "edges %d %s" % (shift, first_high), edge_timeline(n, shift, first_high)
    pulses = np.full(n, 0.1)                                   # one-frame regions on the last and the first frame of waves and tiles
    pulses[[p for p in (WAVE - 1, WAVE, T - 1, T, 2 * T - 1, 2 * T, n - 1) if p < n]] = 0.9
    yield "pulses", pulses


@pytest.mark.parametrize("onset,offset", [(0.5, 0.5), (0.6, 0.4), (0.4, 0.6)])
@pytest.mark.parametrize("min_on,min_off", [(0.0, 0.0), (0.3, 0.2)])
def test_regions_equal_the_oracle_to_annotation(act, onset, offset, min_on, min_off):
    act.set_activity(onset, offset, min_on, min_off)
    rng = np.random.default_rng(7)
    most = 0
    for n in LENGTHS:
        for name, v in timelines(n, onset, offset, rng):
            got = act.activity_regions(v)
            ref = ar.oracle_regions(v, onset, offset, min_on, min_off)
            assert got == ref, (n, name, len(got), len(ref))
            most = max(most, len(got))
    if min_on == 0.0 and min_off == 0.0:
        assert most == (5 * T + 3 + 1) // 2                    # alternating every frame: one region per two frames


def test_bad_options_and_arguments_are_refused(act):
    for key in ACTIVITY_KEYS[:2]:
        for bad in (-0.01, 1.01, float("nan"), float("inf")):
            with pytest.raises(sdhip.SdError) as e:
                act.set_option_f64(key, bad)
            assert e.value.code == 1                            # SD_ERR_ARG
        act.set_option_f64(key, 0.0)
        act.set_option_f64(key, 1.0)
    for key in ACTIVITY_KEYS[2:]:
        for bad in (-1e-9, float("nan")):
            with pytest.raises(sdhip.SdError) as e:
                act.set_option_f64(key, bad)
            assert e.value.code == 1
        act.set_option_f64(key, 7.5)
    with pytest.raises(sdhip.SdError) as e:
        act.set_option("activity_hamming", 2)
    assert e.value.code == 1
    with pytest.raises(sdhip.SdError) as e:
        act.set_activity(onset=1.5)
    assert e.value.code == 1
    seg = ar.random_scores(2, seed=1)
    for kind in (2, -1, "music"):
        with pytest.raises(sdhip.SdError) as e:
            act.activity_scores(seg, kind)
        assert e.value.code == 1
        with pytest.raises(sdhip.SdError) as e:
            act.activity(np.zeros(100000, np.int16), kind)
        assert e.value.code == 1


# ------------------------------------------------------------------ whole path
def test_whole_path_on_the_planted_recording(act):
    """sd_activity_dev on the planted 120 s recording, both kinds: the timeline is the oracle's aggregation of the planted scores, cropped, and the
    regions are the oracle's; with hysteresis, collar and minimum duration too"""
    import torch
    pcm, sc = ar.planted_120s()
    n, nc = len(pcm), len(sc)
    rows = ar.rows_for(nc, n)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc = torch.from_numpy(np.array(pcm)).to(dev), torch.from_numpy(np.array(sc)).to(dev)
    torch.cuda.synchronize()
    act.set_planted(d_sc.data_ptr(), 0, 0, nc)
    try:
        for kind, count in zip(ar.KINDS, (35, 4)):
            ref_scores = ar.oracle_scores(sc, kind)[:rows]
            for opts in ((0.5, 0.5, 0.0, 0.0), (0.6, 0.4, 0.3, 0.2)):
                act.set_activity(*opts)
                turns = act.activity_dev(d_pcm.data_ptr(), n, kind)
                assert np.array_equal(act.last_activity_scores(), ref_scores) and len(ref_scores) == rows == 7112
                assert turns == ar.oracle_regions(ref_scores, *opts, label=kind)
                if opts[2] == 0.0:
                    assert len(turns) == count
            ms = act.stage_ms()
            assert ms[0] > 0 and ms[1] == 0 and ms[2] == 0 and ms[3] >= ms[0]
    finally:
        act.set_planted(0, 0, 0, 0)


def test_every_entry_on_the_reference_wav_and_the_command_line(act, weights, golden_dir):
    """sd_activity (host PCM), sd_activity_f32 and sd_activity_wav on the reference's 1-min recording agree with the oracle applied to
    Diarizer.segment's scores of the same audio; the command line prints sd_activity_wav's turns"""
    path = os.path.join(golden_dir, "multi-speaker_1min.wav")
    pcm, sr, ch = sdhip.read_wav(path)
    wav = pcm.astype(np.float32) / np.float32(32768.0)
    seg = act.segment(wav)
    rows = ar.rows_for(len(seg), len(pcm))
    exe = os.path.join(PKG, "speakerDiarizer")
    rule = "-" * 52
    for kind, word in zip(ar.KINDS, ("SPEECH", "OVERLAP")):
        scores = ar.oracle_scores(seg, kind)[:rows]
        ref = ar.oracle_regions(scores, label=kind)
        assert act.activity(pcm, kind) == ref
        assert np.array_equal(act.last_activity_scores(), scores)
        assert act.activity_f32(wav, kind) == ref
        assert act.activity_wav(path, kind) == ref
        out = subprocess.run([exe, weights[0], weights[1], path, "--activity", ar.NAMES[kind]], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i0 = lines.index(rule)
        assert lines[i0 + 1:lines.index(rule, i0 + 1)] == ["[%g -- %g] --> %s" % (a, b, word) for a, b, _ in ref]
    # the options from the command line
    opts = (0.6, 0.4, 0.3, 0.2)
    act.set_activity(*opts)
    ref = act.activity_wav(path, "speech")
    assert ref == ar.oracle_regions(ar.oracle_scores(seg, 0)[:rows], *opts, label=0)
    out = subprocess.run([exe, weights[0], weights[1], path, "--activity", "speech", "--activity-onset", "0.6", "--activity-offset", "0.4",
                          "--activity-min-on", "0.3", "--activity-min-off", "0.2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    i0 = lines.index(rule)
    assert lines[i0 + 1:lines.index(rule, i0 + 1)] == ["[%g -- %g] --> SPEECH" % (a, b) for a, b, _ in ref]


def test_short_audio_and_bad_wav_flags(act, golden_dir):
    """SD_ERR_SHORT exactly where sd_diarize* returns it"""
    import torch
    one = np.zeros(1, np.int16)
    d_one = torch.from_numpy(one).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    for call, twin in ((lambda: act.activity(one, 0), lambda: act.diarize(one)),
                       (lambda: act.activity_dev(d_one.data_ptr(), 1, 0), lambda: act.diarize_dev(d_one.data_ptr(), 1)),
                       (lambda: act.activity_dev(d_one.data_ptr(), 0, 1), lambda: act.diarize_dev(d_one.data_ptr(), 0)),
                       (lambda: act.activity_f32(one.astype(np.float32), 1), lambda: act.diarize_f32(one.astype(np.float32)))):
        with pytest.raises(sdhip.SdError) as e:
            call()
        with pytest.raises(sdhip.SdError) as e2:
            twin()
        assert e.value.code == e2.value.code == 4                # SD_ERR_SHORT
    with pytest.raises(sdhip.SdError) as e:
        act.activity(np.zeros(0, np.int16), 0)
    assert e.value.code == 1
    L = sdhip.lib()
    import ctypes as C
    p, n = C.POINTER(sdhip.Turn)(), C.c_int64(0)
    assert L.sd_activity_wav(act._h, os.path.join(golden_dir, "multi-speaker_1min.wav").encode(), 8, 0, C.byref(p), C.byref(n)) == 1
    assert L.sd_activity_wav(act._h, b"/nonexistent.wav", 0, 0, C.byref(p), C.byref(n)) == 1


def test_an_activity_job_runs_neither_embedding_nor_linkage_and_leaves_diarization_alone(act):
    import torch
    pcm, sc = ar.planted_120s()
    n = len(pcm)
    d_pcm = torch.from_numpy(np.array(pcm)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    other_stages = ("stft_mel", "se_mean", "se_apply", "asp_stats", "asp_pool", "items_live", "conv_w256_ecapa", "binarize_masks", "count",
                    "pdist", "row_nn", "linkage", "linkage_hx", "linkage_heap", "clusters_K", "activations", "topk")
    act.set_option("profile", 1)
    try:
        act.reset_stats()
        before = act.diarize_dev(d_pcm.data_ptr(), n)
        ran = {k: act.kernel_stats(k)["launches"] for k in other_stages}
        assert ran["stft_mel"] > 0 and ran["asp_pool"] > 0 and ran["binarize_masks"] > 0 and ran["clusters_K"] > 0 and ran["activations"] > 0      # the names are live
        assert act.kernel_stats("activity_scores")["launches"] == 0
        act.reset_stats()
        for kind in ar.KINDS:
            assert len(act.activity_dev(d_pcm.data_ptr(), n, kind)) >= 0
        assert {k: act.kernel_stats(k)["launches"] for k in other_stages} == {k: 0 for k in other_stages}
        assert act.kernel_stats("lstm_rec")["launches"] > 0
        for k in ("activity_scores", "activity_maps", "activity_scan", "activity_regions"):
            assert act.kernel_stats(k)["launches"] == 2
        assert act.diarize_dev(d_pcm.data_ptr(), n) == before
    finally:
        act.set_option("profile", 0)
        act.reset_stats()
