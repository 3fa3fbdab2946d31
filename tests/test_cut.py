"""GPU tests of the cut object (csrc/cut.hip: k_assign_cuts, k_activations_cuts, k_topk_cuts; include/sdhip.h: sd_cut_*): every cut of one dendrogram
equals the finalize under the same three options, bit for bit -- turns, labels, confidences, centroids -- on the planted 120 s recording and on made-up
device arrays of the sizes at which the kernels take another path; one call of many cuts equals the cuts one by one under any grouping; the linkage runs
once; a cut survives other calls on its context; tune scores the grid as tests/der_ref.py does."""
import os
import subprocess
import wave
from fractions import Fraction

import numpy as np
import pytest

import sdhip
import synth
from oracle import orc

import activity_ref as ar
import der_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
SD_ERR_ARG = 1
DIM = 192
LINKAGE_KERNELS = ("pdist", "row_nn", "linkage", "linkage_hx", "linkage_heap")      # every stats name of csrc/linkage*.hip
DEFAULT = sdhip.CLUSTERING_THRESHOLD_DEFAULT
THRESHOLDS = (0.0, 0.05, 0.3, DEFAULT, 1.0, 1.5, 2.0)
GRID = [(t, m, k) for t in THRESHOLDS for m in (1, 15, 40) for k in (-1, 1, 3)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


@pytest.fixture
def ctx(diarizer):
    """the shared context with its clustering options at their defaults, before and after"""
    def reset():
        diarizer.set_clustering()
        for k in ("num_clusters", "min_clusters", "max_clusters"):
            diarizer.set_option(k, -1)
        diarizer.set_option("constrained_assignment", 0)
        diarizer.set_option("cut_group_bytes", 1 << 30)
        diarizer.set_enrolled(None)
        diarizer.set_dump_dir(None)
    reset()
    yield diarizer
    reset()


def _finalize(d, job, spec):
    """finalize_dev with the three options of spec set on the context -> (turns, confidence bytes, centroid bytes, counts)"""
    t, m, k = spec
    d.set_clustering("centroid", DEFAULT if t is None else t, 15 if m is None else m)
    d.set_option("num_clusters", -1 if k is None else k)
    try:
        turns = d.finalize_dev(job["d_seg"].data_ptr(), job["d_emb"].data_ptr(), job["nc"], job["n"])
        cen, cnt = d.last_speakers()
        return turns, _bits(d.last_confidence()), _bits(cen), list(cnt)
    finally:
        d.set_clustering()
        d.set_option("num_clusters", -1)


def _after_cut(d):
    cen, cnt = d.last_speakers()
    return _bits(d.last_confidence()), _bits(cen), list(cnt)


@pytest.fixture(scope="module")
def planted(diarizer):
    """the planted 120 s recording through both networks once: device scores and embeddings (the fixture pattern of tests/test_enrolled.py)"""
    import torch
    pcm, sc = ar.planted_120s()
    n, nc = len(pcm), len(sc)
    sched = synth.with_duets(synth.schedule(120.0, 5))
    _, asg = synth.planted_scores(sched, n, 0, nc)
    pe = synth.planted_embeddings(asg, outlier_every=53)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(np.array(pcm)).to(dev), torch.from_numpy(np.array(sc)).to(dev), torch.from_numpy(pe).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, DIM), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    diarizer.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    try:
        diarizer.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    finally:
        diarizer.set_planted(0, 0, 0, 0)
    assert nc == 231
    ref = []
    for s, e, k, ov in sched:                             # the ground truth of the planted recording as turns
        if k >= 0:
            ref.append((s / 16000.0, e / 16000.0, k))
        if ov >= 0:
            ref.append((s / 16000.0, min(n, s + 8000) / 16000.0, ov))
    return dict(pcm=pcm, n=n, nc=nc, d_pcm=d_pcm, d_sc=d_sc, d_pe=d_pe, d_seg=d_seg, d_emb=d_emb, ref=ref)


def _made_up(chunks, live="most", seed=0):
    """device arrays no network made: uniform scores, normal embeddings rounded through f32, 10 % NaN rows (live = 'none' / 'one': no / exactly one live row)"""
    import torch
    rng = np.random.default_rng(1000 * chunks + seed)
    seg = rng.uniform(0.0, 1.0, (chunks, 293, 3)).astype(np.float32)
    emb = rng.standard_normal((chunks * 3, DIM)).astype(np.float32)
    dead = rng.random(chunks * 3) < 0.10
    if live == "none":
        dead[:] = True
    elif live == "one":
        dead[:] = True
        dead[(chunks * 3) // 2] = False
    emb[dead] = np.nan
    dev = torch.device("cuda", 0)
    d_seg, d_emb = torch.from_numpy(seg).to(dev), torch.from_numpy(emb).to(dev)
    torch.cuda.synchronize()
    n = (chunks - 1) * 8000 + 80000
    assert sdhip.num_chunks(n)[0] == chunks
    return dict(d_seg=d_seg, d_emb=d_emb, nc=chunks, n=n, live=int((~dead).sum()))


def _open(d, job):
    return d.cut_open_dev(job["d_seg"].data_ptr(), job["d_emb"].data_ptr(), job["nc"], job["n"])


def _assert_grid(d, job, grid):
    want = [_finalize(d, job, s) for s in grid]
    with _open(d, job) as cut:
        got = cut.turns_many(grid, with_k=True)
        assert _after_cut(d) == want[-1][1:]                         # the context describes the last cut as after that finalize, bit for bit
        for s, (turns, K), w in zip(grid, got, want):
            assert turns == w[0], s
            assert K >= max([t[2] for t in turns] + [0]) + 1, s
        one = cut.turns(*grid[3])
        assert one == want[3][0] and _after_cut(d) == want[3][1:]
    return got, want


# ------------------------------------------------------------------ equality with finalize_dev
def test_every_cut_of_the_planted_recording_is_that_finalize(ctx, planted):
    got, want = _assert_grid(ctx, planted, GRID)
    K = {s: k for s, (_, k) in zip(GRID, got)}
    labels = {s: sorted({t[2] for t in turns}) for s, (turns, _) in zip(GRID, got)}
    with _open(ctx, planted) as cut:
        Z = cut.dendrogram()
        chunks, n, N = cut.info()
    assert (chunks, n) == (planted["nc"], planted["n"]) and N == 693 - int(np.isnan(planted["d_emb"].cpu().numpy()[:, 0]).sum()) and Z.shape == (N - 1, 4)
    mcs = lambda m: min(m, max(1, round(0.1 * N)))

    def sizes(t):
        return np.bincount(sdhip.fcluster(Z, t))[1:]
    # the all-clusters-small branch: at threshold 0 every row is a cluster of its own, none reaches 15: one label
    assert sizes(0.0).max() < mcs(15) and K[(0.0, 15, -1)] == 1 and labels[(0.0, 15, -1)] == [0]
    # the single-cluster branch (max_clusters < 2): num_clusters = 1
    assert all(K[(t, m, 1)] == 1 for t in THRESHOLDS for m in (1, 15, 40))
    # the small-cluster reassignment: the default cut has clusters below 15 rows (the planted outliers) next to large ones, and only the large ones are left
    s = sizes(DEFAULT)
    assert (s < mcs(15)).any() and K[(DEFAULT, 15, -1)] == int((s >= mcs(15)).sum()) and K[(DEFAULT, 1, -1)] == len(s) > K[(DEFAULT, 15, -1)]
    # the constrained re-cut: three speakers asked for where the threshold alone gives another number
    assert K[(DEFAULT, 15, 3)] == 3 != K[(DEFAULT, 15, -1)] and K[(2.0, 15, 3)] == 3 and K[(2.0, 15, -1)] == 1
    assert len({tuple(w[0]) for w in want}) >= 5                     # the grid is not one answer many times


def test_min_and_max_clusters_are_read_from_the_context(ctx, planted):
    ctx.set_option("min_clusters", 2)
    ctx.set_option("max_clusters", 3)
    grid = [(0.3, 15, -1), (DEFAULT, 15, -1), (2.0, 15, -1), (2.0, 15, 1), (DEFAULT, 1, -1)]
    got, _ = _assert_grid(ctx, planted, grid)
    assert got[2][1] == 2 and got[1][1] == 3 and got[3][1] == 1      # one cluster lifted to min_clusters, four lowered to max_clusters; num_clusters overrides both


@pytest.mark.parametrize("chunks,live", [(1, "most"), (2, "most"), (12, "most"), (400, "most"), (12, "none"), (12, "one")])
def test_every_cut_of_made_up_arrays_is_that_finalize(ctx, chunks, live):
    """1, 2 and 12 chunks (one more than the 11 that can cover a frame), 400 chunks (more than 1 024 clusters at threshold 0 and min_cluster_size 1: past the
    LDS tile of k_assign and of k_assign_cuts), no live row, exactly one"""
    job = _made_up(chunks, live)
    assert job["live"] == {"none": 0, "one": 1}.get(live, job["live"])
    got, _ = _assert_grid(ctx, job, GRID)
    if chunks == 400:
        assert dict(zip(GRID, got))[(0.0, 1, -1)][1] > 1024
    if live != "most":
        assert all(k == 1 for _, k in got)


def test_constrained_assignment_gives_the_finalize_too(ctx, planted):
    ctx.set_option("constrained_assignment", 1)
    grid = [(DEFAULT, 15, -1), (0.3, 1, 3), (1.0, 15, -1), (DEFAULT, 40, 1), (DEFAULT, 15, 3)]
    ctx.reset_stats()
    _assert_grid(ctx, planted, grid)
    assert ctx.kernel_stats("assign_cuts")["launches"] == 0 and ctx.kernel_stats("activations_cuts")["launches"] == 2      # cut by cut through the full score table
    ctx.reset_stats()


# ------------------------------------------------------------------ one call against many, under any grouping
def test_one_call_equals_the_cuts_one_by_one_under_any_grouping(ctx, planted):
    rng = np.random.default_rng(8)
    specs = [GRID[i] for i in rng.permutation(len(GRID))[:24]]
    specs = specs + specs[:5] + [specs[0]] * 3 + [(None, None, None)]
    nact = orc.closest_frame(5.0 + (planted["nc"] - 1) * 0.5) + 1
    with _open(ctx, planted) as cut:
        singles = []
        for s in specs:
            singles.append(cut.turns(*s))
            state = _after_cut(ctx)
        assert singles[-1] == _finalize(ctx, planted, (None, None, None))[0]
        ctx.reset_stats()
        assert cut.turns_many(specs) == singles and _after_cut(ctx) == state
        assert ctx.kernel_stats("assign_cuts")["launches"] == ctx.kernel_stats("activations_cuts")["launches"] == ctx.kernel_stats("topk_cuts")["launches"] == 1
        nontrivial = sum(1 for s in specs if s[2] != 1)
        ctx.set_option("cut_group_bytes", 1)                           # every cut a group of its own
        ctx.reset_stats()
        assert cut.turns_many(specs) == singles and _after_cut(ctx) == state
        assert ctx.kernel_stats("assign_cuts")["launches"] == nontrivial and ctx.kernel_stats("topk_cuts")["launches"] == len(specs)
        same = [(DEFAULT, 15, 3)] * 7                                  # three clusters each: a budget of two such tables makes groups of two
        ctx.set_option("cut_group_bytes", 2 * nact * 3 * 8)
        ctx.reset_stats()
        assert cut.turns_many(same) == [cut.turns(*same[0])] * 7
        assert ctx.kernel_stats("assign_cuts")["launches"] == 4 + 1    # (+ the single cut of the comparison)
        ctx.reset_stats()
        assert cut.turns_many(specs) == singles and _after_cut(ctx) == state
        assert 1 < ctx.kernel_stats("topk_cuts")["launches"] < len(specs)
    ctx.reset_stats()


# ------------------------------------------------------------------ the linkage runs once
def test_the_linkage_runs_once_for_open_and_21_cuts(ctx, planted):
    def launches():
        return {k: ctx.kernel_stats(k)["launches"] for k in LINKAGE_KERNELS}
    ctx.reset_stats()
    _finalize(ctx, planted, (None, None, None))
    one = launches()
    assert one["pdist"] == 1 and one["linkage"] + one["linkage_hx"] + one["linkage_heap"] >= 1
    ctx.reset_stats()
    with _open(ctx, planted) as cut:
        assert launches() == one
        cut.turns_many([(t, m, -1) for t in THRESHOLDS for m in (1, 15, 40)])
        assert launches() == one
    ctx.reset_stats()


# ------------------------------------------------------------------ a cut is independent of the context's other work
def test_a_cut_survives_other_calls_and_changes_no_option(ctx, planted):
    grid = [(DEFAULT, 15, -1), (0.3, 1, -1), (1.0, 40, 3)]
    with _open(ctx, planted) as cut:
        before = cut.turns_many(grid)
        other = ctx.diarize(synth.make_pcm(25.0, seed=7))                # another recording through the whole path: every workspace is reused
        job = _made_up(12)
        ctx.finalize_dev(job["d_seg"].data_ptr(), job["d_emb"].data_ptr(), job["nc"], job["n"])
        assert cut.turns_many(grid) == before
        # the context's own options are as they were: a finalize under the defaults gives the default cut
        assert ctx.finalize_dev(planted["d_seg"].data_ptr(), planted["d_emb"].data_ptr(), planted["nc"], planted["n"]) == before[0]
        assert ctx.diarize(synth.make_pcm(25.0, seed=7)) == other
    with pytest.raises(sdhip.SdError):
        cut.turns()                                                     # closed


def test_gallery_and_dump_directory_are_refused_at_open_and_at_the_call(ctx, planted, tmp_path):
    plain = ctx.finalize_dev(planted["d_seg"].data_ptr(), planted["d_emb"].data_ptr(), planted["nc"], planted["n"])
    gal = np.random.default_rng(2).standard_normal((3, DIM))
    with _open(ctx, planted) as cut:
        for arm, disarm in ((lambda: ctx.set_enrolled(gal), lambda: ctx.set_enrolled(None)), (lambda: ctx.set_dump_dir(str(tmp_path)), lambda: ctx.set_dump_dir(None))):
            arm()
            try:
                with pytest.raises(sdhip.SdError) as e:
                    cut.turns()
                assert e.value.code == SD_ERR_ARG
                with pytest.raises(sdhip.SdError) as e:
                    _open(ctx, planted)
                assert e.value.code == SD_ERR_ARG
                with pytest.raises(sdhip.SdError) as e:
                    ctx.cut_open(planted["pcm"])
                assert e.value.code == SD_ERR_ARG
            finally:
                disarm()
            assert cut.turns() == plain
        for bad in ((2.5, None, None), (-0.1, None, None), (None, -1, None), (None, None, -2)):
            with pytest.raises(sdhip.SdError) as e:
                cut.turns(*bad)
            assert e.value.code == SD_ERR_ARG
    assert not os.listdir(tmp_path)
    assert ctx.finalize_dev(planted["d_seg"].data_ptr(), planted["d_emb"].data_ptr(), planted["nc"], planted["n"]) == plain


# ------------------------------------------------------------------ the whole-path forms
def test_whole_path_open_gives_diarize(ctx, planted, golden_dir):
    p = planted
    ctx.set_clustering("centroid", 0.9, 10)
    ctx.set_planted(p["d_sc"].data_ptr(), p["d_pe"].data_ptr(), 0, p["nc"])
    try:
        turns = ctx.diarize(p["pcm"])
        conf = _bits(ctx.last_confidence())
        assert len({t[2] for t in turns}) >= 3
        wavf = np.asarray(p["pcm"], np.float32) / np.float32(32768.0)
        for cut in (ctx.cut_open(p["pcm"]), ctx.cut_open_pcm_dev(p["d_pcm"].data_ptr(), p["n"]), ctx.cut_open_f32(wavf)):
            with cut:
                assert cut.turns() == turns and _bits(ctx.last_confidence()) == conf
                assert cut.turns(DEFAULT, 15) == _finalize(ctx, p, (DEFAULT, 15, -1))[0]
                ctx.set_clustering("centroid", 0.9, 10)
    finally:
        ctx.set_planted(0, 0, 0, 0)
    ctx.set_clustering()
    wav = os.path.join(golden_dir, "multi-speaker_1min.wav")
    with ctx.cut_open_wav(wav) as cut:
        assert cut.turns() == ctx.diarize_wav(wav)
    with pytest.raises(sdhip.SdError):
        ctx.cut_open_wav(os.path.join(golden_dir, "absent.wav"))


# ------------------------------------------------------------------ tune
def test_tune_scores_the_grid_as_the_reference_does(ctx, planted):
    thresholds = [0.3 + (1.2 - 0.3) * i / 5 for i in range(6)]
    sizes = (5, 15)
    with _open(ctx, planted) as cut:
        table, best = ctx.tune(cut, planted["ref"], thresholds, sizes, collar=0.25)
    assert [(r["threshold"], r["min_cluster_size"]) for r in table] == [(t, m) for t in thresholds for m in sizes]
    ders = []
    for row in table:
        turns = _finalize(ctx, planted, (row["threshold"], row["min_cluster_size"], -1))[0]
        want = dr.der(planted["ref"], turns, collar=0.25)
        bound = want["n"] * Fraction(1, 2 ** 52) * want["extent"]
        for k in dr.COMPONENTS:
            assert abs(Fraction(row[k]) - want[k]) <= bound, (row, k)
        assert row["speakers"] >= max(t[2] for t in turns) + 1
        ders.append(row["der"])
    assert best is table[int(np.argmin(ders))] and not any(np.isnan(ders))
    print("DER of the planted 120 s at the default threshold (collar 0.25): %r" % sdhip.der(planted["ref"], _finalize(ctx, planted, (None, None, None))[0], collar=0.25))


def test_cli_tune_prints_the_best_point_of_tune(ctx, weights, tmp_path):
    """the command line has no planted hook: both sides work on what the seeded networks make of the recording"""
    pcm = synth.make_pcm(40.0, seed=5)
    path = str(tmp_path / "rec.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray(pcm, "<i2").tobytes())
    ref = [(s / 16000.0, e / 16000.0, k) for s, e, k, _ in synth.schedule(40.0, 5) if k >= 0]
    rttm = str(tmp_path / "ref.rttm")
    sdhip.write_rttm(rttm, "rec", ref)
    ref_read, _ = sdhip.read_rttm(rttm)
    thresholds = [0.2 + (1.4 - 0.2) * i / 3 for i in range(4)]
    with ctx.cut_open_wav(path) as cut:
        table, best = ctx.tune(cut, ref_read, thresholds, (3, 15), skip_overlap=True)
    out = subprocess.run([EXE, weights[0], weights[1], path, "--tune", rttm, "--thresholds", "0.2:1.4:4", "--min-cluster-sizes", "3,15", "--skip-overlap"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(table) + 1
    for line, row in zip(lines, table):
        f = line.split()
        assert (float(f[1]), int(f[3]), int(f[5]), float(f[7])) == (row["threshold"], row["min_cluster_size"], row["speakers"], row["der"]), line
    f = lines[-1].split()
    assert f[0] == "best" and (float(f[2]), int(f[4]), float(f[6])) == (best["threshold"], best["min_cluster_size"], best["der"])
