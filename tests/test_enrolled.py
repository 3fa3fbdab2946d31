"""GPU tests of the enrolled speakers (csrc/speakers.hip: k_nearest_gallery; csrc/cluster.hip: the enrolled flow of run_clustering; include/sdhip.h:
sd_set_enrolled, sd_enrolled_info, sd_nearest_speakers, sd_last_enrolled): the kernel alone bit for bit against the sequential cosine distance and its
first minimum, the stage and the whole path against tests/enrolled_ref.py, which tests/test_enrolled_ref.py pins on the CPU."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import sdhip
import synth
from oracle import orc

import activity_ref as ar
import enrolled_ref as er
import speakers_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
SD_ERR_ARG, SD_ERR_NUMERIC = 1, 5
LINKAGE_KERNELS = ("pdist", "row_nn", "linkage", "linkage_hx", "linkage_heap")      # every stats name of csrc/linkage*.hip


def _define(name):
    src = open(os.path.join(PKG, "csrc", "speakers.hip")).read()
    return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))


# tile sizes of k_nearest_gallery, read from the source: train rows per workgroup, gallery rows per tile, waves that share the gallery, longest row held in LDS
R, TK, WAVES, DMAX = (_define(n) for n in ("NG_R", "NG_TK", "NG_WAVES", "NG_DMAX"))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture
def gallery(diarizer):
    """sets a gallery and a threshold for one test and leaves the context as it was"""
    def enrol(gal, t=None):
        diarizer.set_enrolled(gal)
        diarizer.set_option_f64("speaker_match_threshold", sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT if t is None else t)
    yield enrol
    diarizer.set_enrolled(None)
    diarizer.set_option_f64("speaker_match_threshold", sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT)
    diarizer.set_option("constrained_assignment", 0)


# ------------------------------------------------------------------ 1. the kernel alone
def test_tile_sizes_fit_the_machine():
    assert R == 64 and WAVES * R <= 1024 and TK >= 2 and DMAX == sr.DIM
    assert R * (DMAX | 1) * 8 + WAVES * R * 12 <= 160 * 1024                  # the staged rows and the combine buffers, in the LDS of one CU


NS = (1, R - 1, R, R + 1, 2 * R + 3)
MS = (1, TK - 1, TK, TK + 1, 3 * TK + 2, WAVES * TK + 1)                       # ... and one gallery tile more than the waves of a workgroup
DS = (1, 5, 192)


@functools.lru_cache(maxsize=None)
def _kernel_case(N, M, d, integers):
    """(X, gallery, best, dist): the reference is computed once.  Integer-valued data has exact ties: gallery rows are repeated in another gallery
    tile, in another wave's share and on both sides of a row-tile boundary of the train rows"""
    rng = np.random.default_rng(100000 * N + 100 * M + d + int(integers))
    if integers:
        X, V = rng.integers(-3, 4, (N, d)).astype(np.float64), rng.integers(-3, 4, (M, d)).astype(np.float64)
        X[np.abs(X).sum(1) == 0, 0] = 1.0
        V[np.abs(V).sum(1) == 0, 0] = 2.0
        for dup, src in ((TK, 0), (M - 1, 1), (WAVES * TK, 0), (2 * TK + 1, TK - 1)):      # the later copy must never win
            if src < dup < M:
                V[dup] = V[src]
        if N > R:
            X[R] = X[R - 1]                                                     # the same train row in two workgroups
    else:
        X, V = rng.standard_normal((N, d)), rng.standard_normal((M, d))
    D = sr.cosine_distances(X, V)
    best = np.argmin(D, 1).astype(np.int32)                                     # first minimum
    dist = D[np.arange(N), best]
    for a in (X, V, best, dist):
        a.setflags(write=False)
    return X, V, best, dist


@pytest.mark.parametrize("integers", [True, False])
@pytest.mark.parametrize("d", DS)
def test_nearest_equals_the_sequential_reference(diarizer, d, integers):
    ties = 0
    for N in NS:
        for M in MS:
            X, V, best, dist = _kernel_case(N, M, d, integers)
            got_best, got_dist = diarizer.nearest_speakers(X, V)
            assert np.array_equal(got_best, best) and _same_bits(got_dist, dist), (N, M, d)
            D = sr.cosine_distances(X, V)
            ties += int(((D == dist[:, None]).sum(1) > 1).sum())
    if integers:
        assert ties > 0                                                         # equal distances exist: the first index had to win


def test_nearest_leaves_what_lies_behind_its_outputs(diarizer):
    import ctypes as C
    X, V, best, dist = _kernel_case(R + 1, 3 * TK + 2, 5, False)
    N = len(X)
    b, dd = np.full(N + 8, -77, np.int32), np.full(N + 8, -7.5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Xc, Vc = np.ascontiguousarray(X), np.ascontiguousarray(V)
    assert sdhip.lib().sd_nearest_speakers(diarizer._h, p(Xc), N, p(Vc), len(V), 5, p(b), p(dd)) == 0
    assert np.array_equal(b[:N], best) and _same_bits(dd[:N], dist) and (b[N:] == -77).all() and (dd[N:] == -7.5).all()
    b[:] = -77
    assert sdhip.lib().sd_nearest_speakers(diarizer._h, p(Xc), N, p(Vc), len(V), 5, p(b), None) == 0      # either output may be left out
    assert np.array_equal(b[:N], best)
    assert sdhip.lib().sd_nearest_speakers(diarizer._h, p(Xc), N, p(Vc), len(V), 5, None, p(dd)) == 0
    assert _same_bits(dd[:N], dist)


def test_nearest_on_a_long_gallery_and_on_the_enrolled_one(diarizer, gallery):
    rng = np.random.default_rng(77)
    X, V = rng.standard_normal((300, sr.DIM)), rng.standard_normal((20000, sr.DIM))
    V[15000] = V[123]
    X[7] = 3.0 * V[123]                                                         # its nearest row exists twice: the first one
    D = sr.cosine_distances(X, V)
    best = np.argmin(D, 1)
    assert best[7] == 123
    got_best, got_dist = diarizer.nearest_speakers(X, V)
    assert np.array_equal(got_best, best) and _same_bits(got_dist, D[np.arange(300), best])
    assert _same_bits(diarizer.speaker_distances(V[best[:9]], X[:9])[np.arange(9), np.arange(9)], got_dist[:9])      # the bits of sd_speaker_distances
    gallery(V[:1000])
    assert diarizer.enrolled_info() == (1000, sr.DIM)
    b2, d2 = diarizer.nearest_speakers(X)
    assert np.array_equal(b2, np.argmin(D[:, :1000], 1)) and _same_bits(d2, D[:, :1000].min(1))
    diarizer.set_enrolled(None)
    assert diarizer.enrolled_info() == (0, 0)
    with pytest.raises(sdhip.SdError) as e:
        diarizer.nearest_speakers(X)
    assert e.value.code == SD_ERR_ARG


def test_rows_longer_than_the_staged_tile(diarizer):
    rng = np.random.default_rng(5)
    X, V = rng.standard_normal((R + 2, DMAX + 9)), rng.standard_normal((2 * TK + 1, DMAX + 9))
    D = sr.cosine_distances(X, V)
    best, dist = diarizer.nearest_speakers(X, V)
    assert np.array_equal(best, np.argmin(D, 1)) and _same_bits(dist, D.min(1))


def test_nearest_errors_leave_the_context_usable(diarizer, gallery):
    X, V, best, dist = (np.array(a) for a in _kernel_case(R + 1, TK + 1, 5, False))
    zx = X.copy()
    zx[R] = 0.0
    with pytest.raises(sdhip.SdError) as e:
        diarizer.nearest_speakers(zx, V)
    assert e.value.code == SD_ERR_NUMERIC
    gallery(V)
    for bad, code in ((0.0, SD_ERR_NUMERIC), (np.nan, SD_ERR_ARG), (np.inf, SD_ERR_ARG)):
        g = V.copy()
        g[TK] = bad
        with pytest.raises(sdhip.SdError) as e:
            diarizer.set_enrolled(g)
        assert e.value.code == code
        with pytest.raises(sdhip.SdError) as e:
            diarizer.nearest_speakers(X, g)
        assert e.value.code == code
        assert diarizer.enrolled_info() == (len(V), 5)                          # the previous gallery stays
    with pytest.raises(sdhip.SdError) as e:
        diarizer.nearest_speakers(np.ones((3, 7)))                              # d is not the enrolled gallery's
    assert e.value.code == SD_ERR_ARG
    got = diarizer.nearest_speakers(X)
    assert np.array_equal(got[0], best) and _same_bits(got[1], dist)


# ------------------------------------------------------------------ 2. the stage
def _launches(d, names=LINKAGE_KERNELS + ("nearest_gallery",)):
    return {k: d.kernel_stats(k)["launches"] for k in names}


def _assert_stage(diarizer, name, constrained=False):
    emb, gal, t = er.case(name)
    ref = er.clustering(emb, gal, t, constrained=constrained)
    hard, K = diarizer.clustering(emb)
    assert K == ref["K"] and np.array_equal(hard, ref["hard"]), name
    cen, cnt = diarizer.last_speakers()
    assert np.array_equal(cnt, ref["counts"]) and _same_bits(cen, ref["centroids"]), name
    assert np.array_equal(diarizer.last_enrolled(), ref["enrolled"]), name
    return ref


@pytest.mark.parametrize("name", ["far", "far small"])
def test_a_far_gallery_changes_nothing(diarizer, gallery, name):
    emb, gal, t = er.case(name)
    diarizer.reset_stats()
    plain = diarizer.clustering(emb)
    plain_cen, plain_cnt = diarizer.last_speakers()
    assert list(diarizer.last_enrolled()) == [-1] * plain[1]
    before = _launches(diarizer)
    assert before["nearest_gallery"] == 0 and before["pdist"] == 1 and before["linkage"] + before["linkage_hx"] + before["linkage_heap"] >= 1
    gallery(gal, t)
    diarizer.reset_stats()
    ref = _assert_stage(diarizer, name)
    after = _launches(diarizer)
    assert ref["G"] == 0 and after["nearest_gallery"] == 1 and {k: after[k] for k in LINKAGE_KERNELS} == {k: before[k] for k in LINKAGE_KERNELS}
    hard, K = diarizer.clustering(emb)
    cen, cnt = diarizer.last_speakers()
    assert K == plain[1] and np.array_equal(hard, plain[0]) and _same_bits(cen, plain_cen) and np.array_equal(cnt, plain_cnt)
    diarizer.reset_stats()


@pytest.mark.parametrize("name", ["closed", "closed small", "duplicates"])
def test_closed_set_runs_no_linkage_at_all(diarizer, gallery, name):
    emb, gal, t = er.case(name)
    gallery(gal, t)
    diarizer.reset_stats()
    ref = _assert_stage(diarizer, name)
    assert ref["K"] == ref["G"] == 3 and ref["L"] == 0
    assert _launches(diarizer) == dict(dict.fromkeys(LINKAGE_KERNELS, 0), nearest_gallery=1)
    diarizer.reset_stats()


@pytest.mark.parametrize("name", ["hybrid", "hybrid small", "partial", "partial small", "one row", "one left", "tie small"])
def test_enrolled_and_new_speakers_side_by_side(diarizer, gallery, name):
    emb, gal, t = er.case(name)
    ref = er.clustering(emb, gal, t)
    # what the case is there for, shown on the reference before the GPU is asked
    if name.startswith("hybrid"):
        assert 0 < ref["claimed"].sum() < ref["N"] and ref["G"] == 2 and ref["L"] >= 1
    if name in ("hybrid small", "partial"):
        assert ref["to_enrolled"] >= 1
    if name == "one row":
        assert ref["claimed"].sum() == 1 and t == ref["dist"].min()
    if name == "one left":
        assert ref["n_unclaimed"] == 1
    gallery(gal, t)
    _assert_stage(diarizer, name)


@pytest.mark.parametrize("name", ["hybrid", "closed small", "partial small"])
def test_constrained_assignment_over_the_enrolled_table(diarizer, gallery, name):
    emb, gal, t = er.case(name)
    gallery(gal, t)
    diarizer.set_option("constrained_assignment", 1)
    ref = _assert_stage(diarizer, name, constrained=True)
    assert not np.array_equal(ref["hard"], er.clustering(emb, gal, t)["hard"])   # the constraint moved somebody


def test_the_three_refusals(diarizer, gallery, tmp_path):
    emb, gal, t = er.case("hybrid")
    plain = diarizer.clustering(emb)
    gallery(gal, t)
    for kw in ({"num_clusters": 2}, {"min_clusters": 2}, {"max_clusters": 4}):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.clustering(emb, **kw)
        assert e.value.code == SD_ERR_ARG
    with pytest.raises(sdhip.SdError) as e:
        diarizer.clustering(np.random.default_rng(1).standard_normal((10, 3, 5)))      # d is not the gallery's
    assert e.value.code == SD_ERR_ARG
    diarizer.set_dump_dir(str(tmp_path))
    try:
        with pytest.raises(sdhip.SdError) as e:
            diarizer.clustering(emb)
        assert e.value.code == SD_ERR_ARG
    finally:
        diarizer.set_dump_dir(None)
    _assert_stage(diarizer, "hybrid")                                          # the context is fine, the gallery still there
    diarizer.set_enrolled(None)
    assert diarizer.clustering(emb, num_clusters=2)[1] == 2
    hard, K = diarizer.clustering(emb)
    assert K == plain[1] and np.array_equal(hard, plain[0])


# ------------------------------------------------------------------ 3. whole path
REGION = (24.0, 28.0)                        # inside samples [336685, 481950) of the planted schedule: talker 0 alone


@pytest.fixture(scope="module")
def planted(diarizer):
    """the planted 120 s recording through both networks once: device scores and embeddings, their host copies, and the plain job"""
    import torch
    pcm, sc = ar.planted_120s()
    n, nc = len(pcm), len(sc)
    sched = synth.with_duets(synth.schedule(120.0, 5))
    assert any(a <= REGION[0] * 16000 and REGION[1] * 16000 <= b and who == 0 and other < 0 for a, b, who, other in sched)
    _, asg = synth.planted_scores(sched, n, 0, nc)
    pe = synth.planted_embeddings(asg, outlier_every=53)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(np.array(pcm)).to(dev), torch.from_numpy(np.array(sc)).to(dev), torch.from_numpy(pe).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, sr.DIM), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    diarizer.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    try:
        diarizer.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    finally:
        diarizer.set_planted(0, 0, 0, 0)
    turns = diarizer.finalize_dev(d_seg.data_ptr(), d_emb.data_ptr(), nc, n)
    conf = diarizer.last_confidence()
    cen, cnt = diarizer.last_speakers()
    seg, emb = d_seg.cpu().numpy(), d_emb.cpu().numpy().astype(np.float64).reshape(nc, 3, sr.DIM)
    assert len(cen) >= 3 and len(turns) >= 10
    return dict(pcm=pcm, n=n, nc=nc, d_pcm=d_pcm, d_sc=d_sc, d_pe=d_pe, d_seg=d_seg, d_emb=d_emb, seg=seg, emb=emb, turns=turns, conf=conf, cen=cen, cnt=cnt)


def _oracle_turns(seg, hard, n):
    b = orc.binarize(seg)
    cnt, win, ft = orc.speaker_count(b)
    binr, st = orc.reconstruct(seg, orc.mark_inactive(b, hard), cnt, win, ft, n)
    return orc.to_annotation(binr, st)


def test_whole_path_with_a_far_gallery_is_the_plain_job(diarizer, gallery, planted):
    p = planted
    gallery(er.far_row(p["cen"]), 0.0)
    turns = diarizer.finalize_dev(p["d_seg"].data_ptr(), p["d_emb"].data_ptr(), p["nc"], p["n"])
    assert turns == p["turns"] and _same_bits(diarizer.last_confidence(), p["conf"])
    cen, cnt = diarizer.last_speakers()
    assert _same_bits(cen, p["cen"]) and np.array_equal(cnt, p["cnt"]) and list(diarizer.last_enrolled()) == [-1] * len(cen)


def test_whole_path_under_its_own_centroids_reversed(diarizer, gallery, planted):
    p = planted
    gal = p["cen"][::-1].copy()
    t = sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT
    ref = er.clustering(p["emb"], gal, t)
    assert ref["G"] == len(gal)
    gallery(gal)
    turns = diarizer.finalize_dev(p["d_seg"].data_ptr(), p["d_emb"].data_ptr(), p["nc"], p["n"])
    assert turns == _oracle_turns(p["seg"], ref["hard"], p["n"])               # order included
    assert len(diarizer.last_confidence()) == len(turns) and np.isfinite(diarizer.last_confidence()).all()
    cen, cnt = diarizer.last_speakers()
    assert _same_bits(cen, ref["centroids"]) and np.array_equal(cnt, ref["counts"]) and np.array_equal(diarizer.last_enrolled(), ref["enrolled"])
    # the same people as in the plain job, under the gallery's numbering (reconstruction breaks ties between equally active speakers by label, so the turns
    # themselves need not be a relabelling of the plain job's)
    if ref["L"] == 0:
        assert {k for _, _, k in turns} == {len(gal) - 1 - k for _, _, k in p["turns"]}


def test_stream_labels_are_people(diarizer, gallery, planted):
    p = planted
    pcm, n, nc = p["pcm"], p["n"], p["nc"]
    gal = p["cen"][::-1].copy()
    gallery(gal)
    diarizer.set_planted(p["d_sc"].data_ptr(), p["d_pe"].data_ptr(), 0, nc)
    try:
        whole = diarizer.diarize_dev(p["d_pcm"].data_ptr(), n)
        whole_enrolled = diarizer.last_enrolled()
        seen = []
        with diarizer.stream() as s:
            for pos in range(0, n, 160000):
                s.push(pcm[pos:pos + 160000])
                turns = s.turns()
                rows = diarizer.last_enrolled()
                seen.append({int(rows[k]) for a, b, k in turns if a < REGION[1] and b > REGION[0]})
            last, last_enrolled = turns, rows
    finally:
        diarizer.set_planted(0, 0, 0, 0)
    assert last == whole and np.array_equal(last_enrolled, whole_enrolled)
    have = [r for r in seen if r]
    assert len(seen) == 12 and len(have) >= 9 and not any(seen[:2])            # the region starts at 24 s: the third update is the first that has it
    assert all(r == have[0] for r in have) and len(have[0]) == 1 and min(have[0]) >= 0


def test_no_cost_when_unused(diarizer, planted):
    p = planted
    diarizer.reset_stats()
    try:
        assert diarizer.finalize_dev(p["d_seg"].data_ptr(), p["d_emb"].data_ptr(), p["nc"], p["n"]) == p["turns"]
        assert diarizer.kernel_stats("clusters_K")["launches"] == 1
        assert _launches(diarizer, ("nearest_gallery", "gallery_norms")) == {"nearest_gallery": 0, "gallery_norms": 0}
        diarizer.set_enrolled(p["cen"])
        diarizer.finalize_dev(p["d_seg"].data_ptr(), p["d_emb"].data_ptr(), p["nc"], p["n"])
        assert _launches(diarizer, ("nearest_gallery", "gallery_norms")) == {"nearest_gallery": 1, "gallery_norms": 1}      # the names are live
        diarizer.set_enrolled(None)
        assert diarizer.finalize_dev(p["d_seg"].data_ptr(), p["d_emb"].data_ptr(), p["nc"], p["n"]) == p["turns"]
        assert _launches(diarizer, ("nearest_gallery", "gallery_norms")) == {"nearest_gallery": 1, "gallery_norms": 1}      # back to none
    finally:
        diarizer.set_enrolled(None)
        diarizer.reset_stats()


# ------------------------------------------------------------------ 4. command line
def test_command_line_enrols_before_the_job(diarizer, gallery, weights, golden_dir, tmp_path):
    path = os.path.join(golden_dir, "multi-speaker_1min.wav")
    exe = os.path.join(PKG, "speakerDiarizer")
    vp, rttm = str(tmp_path / "people.txt"), str(tmp_path / "out.rttm")
    run = lambda *extra: subprocess.run([exe, weights[0], weights[1], path] + list(extra), capture_output=True, text=True, timeout=600)
    a, _ = diarizer.voiceprint_wav(path, [(0.0, 20.0, 0)])
    b, _ = diarizer.voiceprint_wav(path, [(30.0, 60.0, 0)])
    sdhip.write_voiceprints(vp, ["A", "B"], np.stack([a, b]))
    gallery(np.stack([a, b]), 2.0)
    turns = diarizer.diarize_wav(path)
    rows = diarizer.last_enrolled()
    assert (rows >= 0).any()
    name = lambda k: "AB"[rows[k]] if rows[k] >= 0 else None
    expect = ["[%g -- %g] --> %s" % (s, e, name(k)) if name(k) else sdhip.format_turn((s, e, k)) for s, e, k in turns]
    rule = "-" * 52
    for flags in ((), ("--stream", "7.5")):
        out = run("--speakers", vp, "--enrolled", "--speakers-threshold", "2", "--rttm", rttm, *flags)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i0 = lines.index(rule)
        assert lines[i0 + 1:lines.index(rule, i0 + 1)] == expect
        ref_rttm = str(tmp_path / "ref.rttm")
        sdhip.write_rttm_named(ref_rttm, path, turns, [name(k) for k in range(len(rows))])
        assert open(rttm).read() == open(ref_rttm).read()
    for bad in (("--enrolled",), ("--speakers", vp, "--enrolled", "--enroll", "C"), ("--speakers", vp, "--enrolled", "--activity", "speech"),
                ("--speakers", vp, "--enrolled", "--dump-steps", str(tmp_path)), ("--speakers", vp, "--enrolled", "--gpus", "2")):
        out = run(*bad)
        assert out.returncode == 2 and out.stderr.startswith("usage:"), (bad, out.stderr)
