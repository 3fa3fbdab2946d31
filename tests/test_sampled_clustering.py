"""GPU tests of "max_num_embeddings" / "clustering_seed" (include/sdhip.h, options): the clustering stage under the option against
tests/sample_ref.py -- K, every hard label, the centroids and their counts, bit for bit --, the option unset or at least as large as the number of
train rows giving the bytes of today, and the equalities the library promises between its entry points still holding under it."""
import numpy as np
import pytest

import sdhip
import synth
from oracle import orc

import enrolled_ref as er
import sample_ref as sf
import speakers_ref as sr
import stream_cases as sc

pytestmark = pytest.mark.gpu

SD_ERR_ARG = 1
DIM = 192


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


@pytest.fixture
def ctx(diarizer):
    """the shared context with its clustering options at their defaults, before and after"""
    def reset():
        diarizer.set_clustering(max_num_embeddings=-1, seed=0)
        for k in ("num_clusters", "min_clusters", "max_clusters"):
            diarizer.set_option(k, -1)
        diarizer.set_option("constrained_assignment", 0)
        diarizer.set_enrolled(None)
        diarizer.set_option_f64("speaker_match_threshold", sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT)
        diarizer.set_planted(0, 0, 0, 0)
    reset()
    yield diarizer
    reset()


CASES = {"planted": dict(small=0), "small cluster": dict(small=5)}


def _emb(name):
    return sr.planted_embeddings(chunks=40, clusters=3, nan_fraction=0.25, **CASES[name])


def _stage(d, emb, **kw):
    hard, K = d.clustering(emb, **kw)
    cen, cnt = d.last_speakers()
    return hard, K, cen, cnt


def _assert_stage(got, want, what):
    hard, K, cen, cnt = got
    assert K == want["K"], what
    assert np.array_equal(hard, want["hard"]), (what, int((hard != want["hard"]).sum()))
    assert list(cnt) == list(want["counts"]), what
    assert _bits(cen) == _bits(want["centroids"]), what


# ------------------------------------------------------------------ 1: the stage against the reference
@pytest.mark.parametrize("name", list(CASES))
def test_stage_under_the_option_is_the_reference(ctx, name):
    emb = _emb(name)
    L = len(sf.train_rows(emb))
    assert 60 <= L <= 110
    seen_k = set()
    for seed in (0, 1):
        for m in (1, 2, 17, L - 1, L, L + 1):
            ctx.set_clustering(max_num_embeddings=m, seed=seed)
            want = sf.sampled_clustering(emb, m, seed)
            assert want["counts"].sum() == min(m, L)
            _assert_stage(_stage(ctx, emb), want, (name, m, seed))
            seen_k.add(want["K"])
    assert 1 in seen_k and max(seen_k) >= 3          # the trivial exit of one row and the full answer both occurred
    for m in (17, L - 1):
        ctx.set_clustering(max_num_embeddings=m, seed=1)
        ctx.set_option("constrained_assignment", 1)
        _assert_stage(_stage(ctx, emb), sf.sampled_clustering(emb, m, 1, constrained=True), (name, m, "constrained"))
        ctx.set_option("constrained_assignment", 0)
        _assert_stage(_stage(ctx, emb, num_clusters=2), sf.sampled_clustering(emb, m, 1, num_clusters=2), (name, m, "num_clusters"))


@pytest.mark.parametrize("case", ["hybrid", "partial small"])
def test_stage_under_an_enrolled_gallery_is_the_reference(ctx, case):
    emb, gal, t = er.case(case)
    L = len(sf.train_rows(emb))
    ctx.set_enrolled(gal)
    ctx.set_option_f64("speaker_match_threshold", t)
    claimed = []
    for m in (17, L - 1):
        ctx.set_clustering(max_num_embeddings=m, seed=0)
        want = sf.sampled_clustering(emb, m, 0, gallery=gal, t=t)
        _assert_stage(_stage(ctx, emb), want, (case, m))
        assert list(ctx.last_enrolled()) == list(want["enrolled"]), (case, m)
        claimed.append(int((np.asarray(want["enrolled"]) >= 0).sum()))
    assert max(claimed) >= 1                          # the voiceprints did claim among the sampled rows


def test_the_option_itself(ctx, tmp_path):
    for bad in (0, -2):
        with pytest.raises(sdhip.SdError) as e:
            ctx.set_option("max_num_embeddings", bad)
        assert e.value.code == SD_ERR_ARG and "max_num_embeddings must be" in str(e.value)
        with pytest.raises(sdhip.SdError):
            ctx.set_clustering(max_num_embeddings=bad)
    for seed in (-2 ** 63, 2 ** 63 - 1):
        ctx.set_option("clustering_seed", seed)
    # the step files describe the reference's flow, which clusters every train row: refused together, and nothing is written
    ctx.set_clustering(max_num_embeddings=17, seed=0)
    ctx.set_dump_dir(str(tmp_path), 1)
    try:
        with pytest.raises(sdhip.SdError) as e:
            ctx.clustering(_emb("planted"))
        assert e.value.code == SD_ERR_ARG and "max_num_embeddings is set" in str(e.value)
    finally:
        ctx.set_dump_dir(None)
    assert not list(tmp_path.iterdir())
    # None leaves both as they are: the sample of (17, seed 5) stays the sample
    emb = _emb("planted")
    ctx.set_clustering(max_num_embeddings=17, seed=5)
    a = _stage(ctx, emb)
    ctx.set_clustering()
    b = _stage(ctx, emb)
    assert np.array_equal(a[0], b[0]) and _bits(a[2]) == _bits(b[2])
    _assert_stage(b, sf.sampled_clustering(emb, 17, 5), "kept")


# ------------------------------------------------------------------ 2: m >= L and the default
@pytest.mark.parametrize("name", list(CASES))
def test_at_or_above_the_number_of_train_rows_nothing_changes(ctx, name):
    emb = _emb(name)
    L = len(sf.train_rows(emb))
    base = _stage(ctx, emb)
    ref_hard, ref_K, tl = orc.clustering(emb)
    assert base[1] == ref_K and np.array_equal(base[0], ref_hard)
    for m, seed in ((L, 0), (L, 9), (L + 1, 3), (10 ** 12, -1), (-1, 77)):
        ctx.set_clustering(max_num_embeddings=m, seed=seed)
        got = _stage(ctx, emb)
        assert got[1] == base[1] and got[0].tobytes() == base[0].tobytes() and _bits(got[2]) == _bits(base[2]) and list(got[3]) == list(base[3]), (m, seed)
    ctx.set_clustering(max_num_embeddings=L - 1, seed=0)
    assert list(_stage(ctx, emb)[3]) != list(base[3])      # one row fewer is another job


# ------------------------------------------------------------------ 3, 4: the entry points under the option
@pytest.fixture(scope="module")
def job75(diarizer):
    """the planted tables of the 75 s recording on the device, as sd_finalize_dev takes them (NaN rows by the reference's rule), and the host copies"""
    import torch
    scores, emb = sc.planted75()
    e = np.array(emb, np.float32)
    e[sc.nan_rows(scores)] = np.nan
    dev = torch.device("cuda", 0)
    d_seg, d_emb = torch.from_numpy(np.array(scores)).to(dev), torch.from_numpy(e).to(dev)
    d_pcm = torch.from_numpy(np.array(sc.pcm75())).to(dev)
    d_sc, d_pe = torch.from_numpy(np.array(scores)).to(dev), torch.from_numpy(np.array(emb)).to(dev)
    torch.cuda.synchronize()
    L = int((~np.isnan(e[:, 0])).sum())
    assert L >= 100
    return dict(d_seg=d_seg, d_emb=d_emb, d_pcm=d_pcm, d_sc=d_sc, d_pe=d_pe, seg=np.array(scores), emb=e, nc=sc.CHUNKS, n=sc.N, L=L)


def _finalize(d, job):
    turns = d.finalize_dev(job["d_seg"].data_ptr(), job["d_emb"].data_ptr(), job["nc"], job["n"])
    cen, cnt = d.last_speakers()
    return turns, _bits(d.last_confidence()), _bits(cen), list(cnt)


@pytest.mark.parametrize("m,seed", [(40, 0), (97, 3)])
def test_whole_path_under_the_option_is_the_oracles_tail(ctx, job75, m, seed):
    assert m < job75["L"]
    ctx.set_clustering(max_num_embeddings=m, seed=seed)
    turns, _, cen, cnt = _finalize(ctx, job75)
    seg, nc, n = job75["seg"], job75["nc"], job75["n"]
    want = sf.sampled_clustering(job75["emb"].astype(np.float64).reshape(nc, 3, DIM), m, seed)
    binar = orc.binarize(seg)
    count, cwin, ft = orc.speaker_count(binar)
    hard = orc.mark_inactive(binar, want["hard"])
    binary, start = orc.reconstruct(seg, hard, count, cwin, ft, n)
    ref = orc.to_annotation(binary, start)
    assert turns == ref and len(turns) >= 4 and want["K"] >= 2
    assert cnt == list(want["counts"]) and sum(cnt) == m and cen == _bits(want["centroids"])
    ctx.set_clustering(max_num_embeddings=-1)
    assert _finalize(ctx, job75)[3] != cnt


def test_a_cut_describes_the_sample_and_equals_the_finalize(ctx, job75):
    m = 40
    ctx.set_clustering(max_num_embeddings=m, seed=2)
    want = _finalize(ctx, job75)
    with ctx.cut_open_dev(job75["d_seg"].data_ptr(), job75["d_emb"].data_ptr(), job75["nc"], job75["n"]) as cut:
        assert cut.info() == (job75["nc"], job75["n"], m)
        assert len(cut.dendrogram()) == m - 1
        ctx.set_clustering(max_num_embeddings=-1, seed=0)          # the option is read at open
        assert cut.turns() == want[0]
        cen, cnt = ctx.last_speakers()
        assert (_bits(ctx.last_confidence()), _bits(cen), list(cnt)) == want[1:]
        assert cut.info()[2] == m


def test_a_stream_under_the_option_is_the_whole_path(ctx, job75):
    pcm = sc.pcm75()
    ctx.set_clustering(max_num_embeddings=25, seed=4)
    ctx.set_planted(job75["d_sc"].data_ptr(), job75["d_pe"].data_ptr(), 0, sc.CHUNKS)
    try:
        with ctx.stream() as s:
            pos = 0
            for n in (600123, 1200000):
                s.push(pcm[pos:n])
                pos = n
                got = s.turns()
                counts = list(ctx.last_speakers()[1])
                assert got == ctx.diarize_dev(job75["d_pcm"].data_ptr(), n) and len(got) >= 2, n
                assert sum(counts) == 25 and list(ctx.last_speakers()[1]) == counts, n
    finally:
        ctx.set_planted(0, 0, 0, 0)


def test_rank_0_of_a_sharded_job_under_the_option_is_the_whole_path(ctx, job75):
    """one rank (and one rank playing three): sd_diarize_sharded* under the option equal sd_diarize_dev and sd_finalize_dev under it"""
    pcm = sc.pcm75()
    m = 40
    assert m < job75["L"]
    ctx.set_clustering(max_num_embeddings=m, seed=8)
    want = _finalize(ctx, job75)
    ctx.set_planted(job75["d_sc"].data_ptr(), job75["d_pe"].data_ptr(), 0, sc.CHUNKS)
    ctx.comm_init(sdhip.comm_unique_id(), 0, 1)

    def after(turns):
        cen, cnt = ctx.last_speakers()
        return turns, _bits(ctx.last_confidence()), _bits(cen), list(cnt)

    try:
        whole = after(ctx.diarize_dev(job75["d_pcm"].data_ptr(), sc.N))
        assert whole == want and sum(whole[3]) == m and len(whole[0]) >= 4
        assert after(ctx.diarize_sharded_dev(job75["d_pcm"].data_ptr(), 0, sc.N, sc.N)) == want
        assert after(ctx.diarize_sharded(pcm, 0, sc.N)) == want
        ctx.set_option("virtual_world", 3)
        assert after(ctx.diarize_sharded_dev(job75["d_pcm"].data_ptr(), 0, sc.N, sc.N)) == want
        ctx.set_option("virtual_world", 0)
        ctx.set_clustering(max_num_embeddings=-1)
        plain = after(ctx.diarize_sharded_dev(job75["d_pcm"].data_ptr(), 0, sc.N, sc.N))
        assert plain[3] != want[3] and sum(plain[3]) == job75["L"]
    finally:
        ctx.set_option("virtual_world", 0)
        ctx.comm_destroy()
        ctx.set_planted(0, 0, 0, 0)


def test_packs_and_groups_under_the_option_equal_the_single_calls(ctx):
    a, b = sc.pcm75()[:700000], synth.make_pcm(45.0, 5)
    live = []
    for p in (a, b):                                   # the train rows each recording has with the real networks
        wav = p.astype(np.float32) / np.float32(32768.0)
        _, masks, _ = ctx.postseg(ctx.segment(wav))
        live.append(int(np.isfinite(ctx.embed(wav, masks)[:, 0]).sum()))
    m = max(1, min(live) // 2)
    assert min(live) > m
    ctx.set_clustering(max_num_embeddings=m, seed=6)
    alone = []
    for p in (a, b):
        t = ctx.diarize(p)
        alone.append((t, list(ctx.last_speakers()[1])))
        assert sum(alone[-1][1]) == m
    many = ctx.diarize_many([a, b])
    for r in range(2):
        ctx.many_select(r)
        assert many[r] == alone[r][0] and list(ctx.last_speakers()[1]) == alone[r][1], r
    with ctx.stream() as sa, ctx.stream() as sb:
        ctx.stream_push_many([sa, sb], [a[:400001], b[:300000]])
        ctx.stream_push_many([sa, sb], [a[400001:], b[300000:]])
        got = ctx.stream_turns_many([sa, sb])
        for r in range(2):
            ctx.many_select(r)
            assert got[r] == alone[r][0] and list(ctx.last_speakers()[1]) == alone[r][1], r
