"""GPU tests of the known-speaker entries (csrc/speakers.hip, csrc/cluster.hip; include/sdhip.h: sd_last_speakers, sd_span_masks, sd_voiceprint*,
sd_speaker_distances, sd_match_speakers): every result bit for bit against the float64 / integer references of tests/speakers_ref.py, which
tests/test_speakers_ref.py pins to the oracle."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import sdhip
import synth
from oracle import orc

import activity_ref as ar
import speakers_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
# tile sizes of k_speaker_dist (csrc/speakers.hip): gallery rows per workgroup, centroids per pass, dimensions per staged slice
TM, TK, TI = 128, 8, 16
SD_ERR_ARG, SD_ERR_SHORT, SD_ERR_NUMERIC = 1, 4, 5
NEW_KERNELS = ("span_masks", "voiceprint_mean", "speaker_dist")


def test_tile_sizes_are_the_kernels():
    src = open(os.path.join(PKG, "csrc", "speakers.hip")).read()
    for name, v in (("SPK_TM", TM), ("SPK_TK", TK), ("SPK_TI", TI)):
        assert int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1)) == v


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _assert_speakers(d, emb, train):
    cen_ref, cnt_ref = sr.centroids(emb, train)
    cen, cnt = d.last_speakers()
    assert cen.shape == cen_ref.shape and np.array_equal(cnt, cnt_ref)
    assert np.array_equal(cen, cen_ref, equal_nan=True)
    if not np.isnan(cen_ref).any():
        assert _same_bits(cen, cen_ref)
    return cen


# ------------------------------------------------------------------ 1. centroids after Diarizer.clustering
@pytest.mark.parametrize("case", ["plain", "num_clusters=2", "small cluster"])
def test_centroids_of_the_clustering_stage(diarizer, case):
    emb = sr.planted_embeddings(small=5 if case == "small cluster" else 0)
    kw = {"num_clusters": 2} if case == "num_clusters=2" else {}
    hard, K = diarizer.clustering(emb, **kw)
    h_ref, K_ref, train = orc.clustering(emb, **kw)
    assert K == K_ref == (2 if kw else 3) and np.array_equal(hard, h_ref)
    cen = _assert_speakers(diarizer, emb, train)
    assert len(cen) == K


@pytest.mark.parametrize("method", [m for m in sdhip.LINKAGE_METHODS if m != "centroid"])
def test_centroids_under_every_other_linkage_method(diarizer, method):
    from test_clustering_hyperparams import _py_spec
    emb = sr.planted_embeddings()
    h_ref, train = _py_spec(emb.copy(), method)
    try:
        diarizer.set_clustering(method)
        hard, K = diarizer.clustering(emb)
    finally:
        diarizer.set_clustering()
    assert K == train.max() + 1 and np.array_equal(hard, h_ref)
    _assert_speakers(diarizer, emb, train)


def test_centroids_of_the_degenerate_branches(diarizer):
    emb = np.full((4, 3, sr.DIM), np.nan)
    hard, K = diarizer.clustering(emb)                                       # no train row at all: a NaN row with count 0
    assert K == 1 and not hard.any()
    cen, cnt = diarizer.last_speakers()
    assert cen.shape == (1, sr.DIM) and np.isnan(cen).all() and list(cnt) == [0]
    row = np.random.default_rng(2).standard_normal(sr.DIM)
    emb[2, 1] = row                                                          # exactly one: the row itself
    hard, K = diarizer.clustering(emb)
    assert K == 1 and not hard.any()
    cen, cnt = diarizer.last_speakers()
    assert _same_bits(cen, row[None]) and list(cnt) == [1]
    emb = sr.planted_embeddings()                                            # max_clusters < 2: the mean of the train rows
    hard, K = diarizer.clustering(emb, num_clusters=1)
    assert K == 1 and not hard.any()
    N = int((~np.isnan(emb.reshape(-1, sr.DIM)[:, 0])).sum())
    _assert_speakers(diarizer, emb, np.zeros(N, np.int32))
    emb5 = np.random.default_rng(5).standard_normal((30, 3, 5))               # rows of another length
    diarizer.clustering(emb5)
    _assert_speakers(diarizer, emb5, orc.clustering(emb5)[2])


def test_no_speakers_before_any_clustering_call(weights):
    d = sdhip.Diarizer(None, None)
    try:
        cen, cnt = d.last_speakers()
        assert cen.shape == (0, sr.DIM) and cnt.shape == (0,)
        with pytest.raises(sdhip.SdError) as e:
            d.speaker_distances(np.ones((2, sr.DIM)))
        assert e.value.code == SD_ERR_ARG
    finally:
        d.close()


# ------------------------------------------------------------------ 2. whole path
def test_whole_path_and_stream_keep_the_same_speakers(diarizer):
    import torch
    pcm, sc = ar.planted_120s()
    n, nc = len(pcm), len(sc)
    _, asg = synth.planted_scores(synth.with_duets(synth.schedule(120.0, 5)), n, 0, nc)
    pe = synth.planted_embeddings(asg, outlier_every=53)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(np.array(pcm)).to(dev), torch.from_numpy(np.array(sc)).to(dev), torch.from_numpy(pe).to(dev)
    torch.cuda.synchronize()
    diarizer.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    try:
        turns = diarizer.diarize_dev(d_pcm.data_ptr(), n)
        cen, cnt = diarizer.last_speakers()
        diarizer.clustering(sr.planted_embeddings())                         # something else in between
        with diarizer.stream() as s:
            pos = 0
            for end in (1, 79999, 123457, 600001, 1000000, 1531234, n):
                s.push(pcm[pos:end])
                pos = end
            assert s.turns() == turns
            cen2, cnt2 = diarizer.last_speakers()
            _, emb = s.read(0, nc, seg=False)
    finally:
        diarizer.set_planted(0, 0, 0, 0)
    assert _same_bits(cen, cen2) and np.array_equal(cnt, cnt2)
    emb3 = emb.astype(np.float64).reshape(nc, 3, sr.DIM)
    _, K, train = orc.clustering(emb3)
    cen_ref, cnt_ref = sr.centroids(emb3, train)
    assert K >= 3 and len(turns) >= 10
    assert _same_bits(cen, cen_ref) and np.array_equal(cnt, cnt_ref)
    assert {t[2] for t in turns} <= set(range(K))


# ------------------------------------------------------------------ 3. span masks
N_LONG, N_SHORT = 30 * 16000 + 1234, 50000     # 52 chunks = 156 items: several 32-item batch boundaries; one short chunk
SPANS = [(1.0001, 1.9, 0),                     # starts mid-frame
         (3.0, 14.5, 0),                       # crosses several chunks
         (16.0, 16.03, 1),                     # 480 samples: shorter than 640
         (29.5, 31.0, 0), (40.0, 41.0, 0),     # partly and wholly behind the end of the audio
         (20.0, 22.0, 1), (21.0, 23.5, 1)]     # two that overlap; two labels
SHORT_SPAN = [SPANS[2]]


@pytest.mark.parametrize("n", [N_LONG, N_SHORT])
def test_span_masks_equal_the_reference(diarizer, n):
    assert sr.num_chunks(n) == sdhip.num_chunks(n)[0] == (52 if n == N_LONG else 1)
    fs = sr.frame_start(np.arange(sr.FRAMES))
    assert int(round(SPANS[0][0] * 16000)) not in set(fs) | set(fs + sr.HOP)   # mid-frame for chunks 0 and 1
    for label in (0, 1, -1):
        got = diarizer.span_masks(n, SPANS, label)
        ref = sr.span_masks(n, SPANS, label)
        assert got.dtype == np.float32 and np.array_equal(got, ref)
        assert not got[1::3].any() and not got[2::3].any()
        assert set(np.unique(got)) <= {0.0, 1.0}
    assert (diarizer.span_masks(n, SPANS, 0) * diarizer.span_masks(n, SPANS, 1)).sum() == 0          # the other label's frames are exactly zero
    if n == N_LONG:
        assert diarizer.span_masks(n, SPANS, 0).any() and diarizer.span_masks(n, SPANS, 1).any()
    assert np.array_equal(diarizer.span_masks(n, None), sr.span_masks(n, None))                       # the whole recording
    assert np.array_equal(diarizer.span_masks(n, []), sr.span_masks(n, None))
    assert not diarizer.span_masks(n, [], 0).any() and not diarizer.span_masks(n, SPANS, 7).any()
    last = diarizer.span_masks(n, None)[3 * (sr.num_chunks(n) - 1)]          # the frames of the last chunk that start behind the end of the audio are off
    assert last[0] == 1.0 and last[-1] == 0.0


# ------------------------------------------------------------------ 4. voiceprints
@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    pcm = synth.make_pcm(31.0, seed=7, limit=N_LONG)
    assert len(pcm) == N_LONG
    path = str(tmp_path_factory.mktemp("vp") / "rec.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    return pcm, pcm.astype(np.float32) / np.float32(32768.0), path


@pytest.fixture(scope="module")
def voiceprint_refs(diarizer, recording):
    """label -> (mean of the live rows 3c of Diarizer.embed under the reference masks, their number); computed once"""
    _, wav, _ = recording
    out = {}
    for label in (0, 1, -1, None):
        emb = diarizer.embed(wav, sr.span_masks(N_LONG, None if label is None else SPANS, -1 if label is None else label))
        assert np.isnan(emb[1::3]).all() and np.isnan(emb[2::3]).all()
        out[label] = sr.voiceprint(emb)
    return out


def test_voiceprints_equal_the_mean_of_the_embedding_stage_rows(diarizer, recording, voiceprint_refs):
    import torch
    pcm, wav, path = recording
    d_pcm = torch.from_numpy(pcm).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    for label in (0, 1, -1):
        ref, nw = voiceprint_refs[label]
        assert nw >= 3 and nw == int(sr.live_windows(sr.span_masks(N_LONG, SPANS, label)).sum())
        for got in (diarizer.voiceprint(pcm, SPANS, label), diarizer.voiceprint_dev(d_pcm.data_ptr(), N_LONG, SPANS, label),
                    diarizer.voiceprint_f32(wav, SPANS, label), diarizer.voiceprint_wav(path, SPANS, label)):
            assert got[1] == nw and _same_bits(got[0], ref)
    ref, nw = voiceprint_refs[None]
    assert nw == 52
    for spans in (None, []):
        got = diarizer.voiceprint(pcm, spans)
        assert got[1] == nw and _same_bits(got[0], ref)
    # one label per pass: the same bits whether or not the other label's spans are in the list
    for label in (0, 1):
        alone = [s for s in SPANS if s[2] == label]
        got = diarizer.voiceprint(pcm, alone, label)
        assert got[1] == voiceprint_refs[label][1] and _same_bits(got[0], voiceprint_refs[label][0])
    assert not _same_bits(voiceprint_refs[0][0], voiceprint_refs[1][0])
    ms = diarizer.stage_ms()
    assert ms[0] == 0 and ms[1] > 0 and ms[2] == 0 and ms[3] >= ms[1]


def test_voiceprint_errors_leave_the_context_usable(diarizer, recording, voiceprint_refs):
    pcm, wav, path = recording
    with pytest.raises(sdhip.SdError) as e:
        diarizer.voiceprint(pcm, SHORT_SPAN, 1)                               # 480 selected samples in every window
    assert e.value.code == SD_ERR_SHORT
    with pytest.raises(sdhip.SdError) as e:
        diarizer.voiceprint(pcm, SPANS, 7)                                    # nobody has that label
    assert e.value.code == SD_ERR_SHORT
    for bad in ((2.0, 1.0, 0), (float("nan"), 1.0, 0), (0.0, float("nan"), 0), (-0.5, 1.0, 0), (-2.0, -1.0, 0)):
        for call in (lambda s: diarizer.voiceprint(pcm, s), lambda s: diarizer.voiceprint_f32(wav, s), lambda s: diarizer.voiceprint_wav(path, s),
                     lambda s: diarizer.span_masks(N_LONG, s)):
            with pytest.raises(sdhip.SdError) as e:
                call([SPANS[1], bad])
            assert e.value.code == SD_ERR_ARG
        with pytest.raises(sdhip.SdError) as e:
            diarizer.voiceprint(pcm, [SPANS[1], bad], 0)                      # ... whatever its label
        assert e.value.code == SD_ERR_ARG
        got = diarizer.voiceprint(pcm, SPANS, 0)                              # a following good call still works
        assert got[1] == voiceprint_refs[0][1] and _same_bits(got[0], voiceprint_refs[0][0])
    with pytest.raises(sdhip.SdError) as e:
        diarizer.voiceprint(np.zeros(1, np.int16))
    assert e.value.code == SD_ERR_SHORT
    import ctypes as C
    emb, nw = np.zeros(sr.DIM), C.c_int64(0)
    assert sdhip.lib().sd_voiceprint_wav(diarizer._h, path.encode(), 8, None, 0, -1, emb.ctypes.data_as(C.c_void_p), C.byref(nw)) == SD_ERR_ARG
    assert sdhip.lib().sd_voiceprint_wav(diarizer._h, b"/nonexistent.wav", 0, None, 0, -1, emb.ctypes.data_as(C.c_void_p), C.byref(nw)) == SD_ERR_ARG


# ------------------------------------------------------------------ 5. distances
# K straddles the centroid tile (TK = 8): 7, 8, 9, and 70 = eight full passes and a part; M straddles the gallery tile (TM = 128): 127, 128, 129, and
# 1000 = seven full workgroups and a part; 63, 64, 65 straddle the wave inside a workgroup; d = 192 is twelve whole slices (TI = 16), 5 a part of
# one, 16 and 17 straddle the slice
KS = (1, 3, 7, 8, 9, 70)
MS = (1, 63, 64, 65, 127, 128, 129, 1000)
DS = (192, 5, 16, 17)


@pytest.mark.parametrize("integers", [True, False])
@pytest.mark.parametrize("d", DS)
def test_distances_equal_the_sequential_reference(diarizer, d, integers):
    for K in KS:
        for M in MS:
            cen, gal = sr.distance_case(K, M, d, integers)
            got = diarizer.speaker_distances(gal, cen)
            assert _same_bits(got, sr.cosine_distances(cen, gal)), (K, M, d)


def test_distances_skip_nan_centroids_and_refuse_zero_rows(diarizer):
    cen, gal = (np.array(a) for a in sr.distance_case(9, 129, 17, False))
    cen[[0, 8]] = np.nan
    cen[4, 1:] = np.nan                                                       # a NaN that is not in front: an ordinary row, NaN distances by arithmetic
    got = diarizer.speaker_distances(gal, cen)
    ref = sr.cosine_distances(cen, gal)
    assert np.isnan(got[[0, 4, 8]]).all() and np.array_equal(got, ref, equal_nan=True) and _same_bits(got[[1, 2, 3, 5, 6, 7]], ref[[1, 2, 3, 5, 6, 7]])
    match, best = diarizer.match_speakers(gal, cen, threshold=2.0)
    assert list(match[[0, 4, 8]]) == [-1, -1, -1] and (match[[1, 2, 3, 5, 6, 7]] >= 0).all() and np.isnan(best[[0, 4, 8]]).all()
    zc, zg = cen.copy(), gal.copy()
    zc[2] = 0.0
    zg[128] = 0.0
    for c_, g_ in ((zc, gal), (cen, zg), (np.full((1, 17), np.nan), zg)):     # a zero gallery row counts even when every centroid is skipped
        with pytest.raises(sdhip.SdError) as e:
            diarizer.speaker_distances(g_, c_)
        assert e.value.code == SD_ERR_NUMERIC
        with pytest.raises(sdhip.SdError) as e:
            diarizer.match_speakers(g_, c_)
        assert e.value.code == SD_ERR_NUMERIC
    assert _same_bits(diarizer.speaker_distances(gal, cen[1:4]), ref[1:4])     # ... and the context is fine afterwards


def test_distances_and_matching_of_the_last_job(diarizer):
    emb = sr.planted_embeddings()
    _, K = diarizer.clustering(emb)
    cen, _ = diarizer.last_speakers()
    assert K == 3
    rng = np.random.default_rng(8)
    gal = rng.standard_normal((70, sr.DIM))
    assert _same_bits(diarizer.speaker_distances(gal), sr.cosine_distances(cen, gal))
    # the last job's centroids in reverse order plus one random row: the reversal is recovered, the random row stays unused
    gal = np.vstack([cen[::-1], rng.standard_normal((1, sr.DIM))])
    match, best = diarizer.match_speakers(gal)
    assert list(match) == [2, 1, 0] and (best <= 1e-15).all()
    import ctypes as C
    out = np.zeros((2, 4))
    assert sdhip.lib().sd_speaker_distances(diarizer._h, None, 2, gal.ctypes.data_as(C.c_void_p), 4, sr.DIM, out.ctypes.data_as(C.c_void_p)) == SD_ERR_ARG      # K is not the job's
    assert sdhip.lib().sd_speaker_distances(diarizer._h, None, 3, gal.ctypes.data_as(C.c_void_p), 4, 5, out.ctypes.data_as(C.c_void_p)) == SD_ERR_ARG            # nor d


# ------------------------------------------------------------------ 6. matching
@pytest.mark.parametrize("K,M,d", [(70, 1000, 5), (9, 129, 192), (70, 65, 5), (3, 1, 192)])
def test_matching_equals_the_greedy_reference(diarizer, K, M, d):
    cen, gal = sr.distance_case(K, M, d, False)
    dist = sr.cosine_distances(cen, gal)
    flat = np.sort(dist.reshape(-1))
    for thr in (float(flat[len(flat) // 3]), sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT, 1.0, float(np.nextafter(flat[len(flat) // 3], 0.0))):
        match, best = diarizer.match_speakers(gal, cen, threshold=thr)
        m_ref, b_ref = sr.greedy_match(dist, thr)
        assert np.array_equal(match, m_ref) and np.array_equal(best, b_ref, equal_nan=True), thr
        taken = match[match >= 0]
        assert len(set(taken)) == len(taken)                                  # one-to-one


def test_match_threshold_option(diarizer):
    cen, gal = sr.distance_case(70, 1000, 5, False)
    dist = sr.cosine_distances(cen, gal)
    default = sr.greedy_match(dist, sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT)[0]
    t = float(np.float32(0.7153814381597874))
    assert sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT == t * t / 2
    # the table is dense around the default (20 distances within 1e-3 of it): another default would match other pairs
    near = np.sort(np.abs(dist.reshape(-1) - sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT))
    assert near[0] > 0 and near[20] < 1e-3
    assert np.array_equal(diarizer.match_speakers(gal, cen)[0], default)
    try:
        for bad in (-0.01, 2.01, float("nan"), float("inf")):
            with pytest.raises(sdhip.SdError) as e:
                diarizer.set_option_f64("speaker_match_threshold", bad)
            assert e.value.code == SD_ERR_ARG
        assert np.array_equal(diarizer.match_speakers(gal, cen)[0], default)   # a refused value changes nothing
        for thr in (0.0, 0.01, 2.0):
            diarizer.set_option_f64("speaker_match_threshold", thr)
            assert np.array_equal(diarizer.match_speakers(gal, cen)[0], sr.greedy_match(dist, thr)[0])
            assert np.array_equal(diarizer.match_speakers(gal, cen, threshold=0.5)[0], sr.greedy_match(dist, 0.5)[0])      # the argument wins
    finally:
        diarizer.set_option_f64("speaker_match_threshold", sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT)
    for bad in (-0.01, 2.5, float("inf")):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.match_speakers(gal, cen, threshold=bad)
        assert e.value.code == SD_ERR_ARG


# ------------------------------------------------------------------ 7. command line
def test_command_line_enrols_and_names_the_speakers(diarizer, weights, golden_dir, tmp_path):
    path = os.path.join(golden_dir, "multi-speaker_1min.wav")
    exe = os.path.join(PKG, "speakerDiarizer")
    vp, rttm = str(tmp_path / "people.txt"), str(tmp_path / "out.rttm")
    run = lambda *extra: subprocess.run([exe, weights[0], weights[1], path] + list(extra), capture_output=True, text=True, timeout=600)
    a, na = diarizer.voiceprint_wav(path, [(0.0, 20.0, 0)])
    b, nb = diarizer.voiceprint_wav(path)
    out = run("--enroll", "A", "--enroll-span", "0", "20", "--speakers", vp)
    assert out.returncode == 0 and out.stdout.strip() == "enrolled A from %d windows" % na, out.stderr
    out = run("--enroll", "B", "--speakers", vp)
    assert out.returncode == 0 and out.stdout.strip() == "enrolled B from %d windows" % nb, out.stderr
    ref_file = str(tmp_path / "ref.txt")
    sdhip.write_voiceprints(ref_file, ["A", "B"], np.stack([a, b]))
    assert open(vp, "rb").read() == open(ref_file, "rb").read()
    out = run("--enroll", "A", "--speakers", vp)                              # enrolling a name again replaces it, in place
    assert out.returncode == 0, out.stderr
    sdhip.write_voiceprints(ref_file, ["A", "B"], np.stack([b, b]))
    assert open(vp, "rb").read() == open(ref_file, "rb").read()
    sdhip.write_voiceprints(vp, ["A", "B"], np.stack([a, b]))
    rule = "-" * 52
    for flags, thr in (((), None), (("--speakers-threshold", "2"), 2.0)):
        turns = diarizer.diarize_wav(path)
        match, _ = diarizer.match_speakers(np.stack([a, b]), threshold=thr)
        name = lambda k: None if match[k] < 0 else "AB"[match[k]]
        if thr == 2.0:
            assert (match >= 0).sum() == min(len(match), 2)
        out = run("--speakers", vp, "--rttm", rttm, *flags)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i0 = lines.index(rule)
        assert lines[i0 + 1:lines.index(rule, i0 + 1)] == ["[%g -- %g] --> %s" % (s, e, name(k)) if name(k) else sdhip.format_turn((s, e, k)) for s, e, k in turns]
        ref_rttm = str(tmp_path / "ref.rttm")
        sdhip.write_rttm_named(ref_rttm, path, turns, [name(k) for k in range(len(match))])
        assert open(rttm).read() == open(ref_rttm).read()
    out = run("--speakers", vp, "--speakers-threshold", "2", "--stream", "7.5")      # a streamed run names them too
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    i0 = lines.index(rule)
    assert lines[i0 + 1:lines.index(rule, i0 + 1)] == ["[%g -- %g] --> %s" % (s, e, name(k)) if name(k) else sdhip.format_turn((s, e, k)) for s, e, k in turns]


# ------------------------------------------------------------------ 8. no cost when unused
def test_a_plain_job_launches_none_of_the_new_kernels(diarizer):
    import torch
    pcm, _ = ar.planted_120s()
    d_pcm = torch.from_numpy(np.array(pcm)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    diarizer.reset_stats()
    try:
        assert len(diarizer.diarize_dev(d_pcm.data_ptr(), len(pcm))) >= 0
        assert diarizer.kernel_stats("clusters_K")["launches"] == 1
        assert {k: diarizer.kernel_stats(k)["launches"] for k in NEW_KERNELS} == dict.fromkeys(NEW_KERNELS, 0)
        diarizer.voiceprint_dev(d_pcm.data_ptr(), len(pcm), [(1.0, 30.0, 0)])       # ... and the names are live
        diarizer.speaker_distances(np.ones((3, sr.DIM)))
        assert {k: diarizer.kernel_stats(k)["launches"] for k in NEW_KERNELS} == dict.fromkeys(NEW_KERNELS, 1)
    finally:
        diarizer.reset_stats()
