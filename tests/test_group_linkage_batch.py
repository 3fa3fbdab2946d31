"""GPU tests of the dendrograms-ahead pass of the group calls (csrc/many.hip: dendrograms_ahead; option "linkage_batch"): sd_diarize_many and
sd_stream_turns_many give the same bytes per job -- turns, confidences, centroids, counts, status -- with the pass (one k_linkage_heap_jobs launch, no
k_linkage_heap) and without it (the sequential flow), under "max_num_embeddings", and the jobs that skip the pass (an enrolled gallery, num_clusters = 1)
and the single-job entries launch none of its kernels.  Seeded networks and synthetic audio as in tests/test_many.py."""
import numpy as np
import pytest

import sdhip
import synth
from stream_cases import pcm75

pytestmark = pytest.mark.gpu

SD_ERR_SHORT = 4
SECONDS = (10.0, 17.5, 25.0, 33.0, 45.0)
JOBS_KERNELS = ("pdist_jobs", "row_nn_jobs", "linkage_heap_jobs")

_cache = {}


def recordings():
    """five recordings of 10 - 45 s, each with audio of its own, and one too short for a chunk (read-only)"""
    if not _cache:
        recs = [synth.make_pcm(s + 1.0, seed=5200 + r)[:int(s * 16000) + 17 * r].copy() for r, s in enumerate(SECONDS)]
        recs.insert(3, np.zeros(1, np.int16))
        for p in recs:
            p.setflags(write=False)
        _cache["recs"] = recs
    return _cache["recs"]


def job_bytes(d):
    cen, cnt = d.last_speakers()
    return d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes(), d.last_enrolled().tobytes()


def turn_bytes(turns):
    return np.array([(s, e, l) for s, e, l in turns], np.float64).tobytes()


def group_result(d, call, J):
    """per job of a group call: the error code, or (turn bytes, the job's bytes)"""
    out = []
    for j, g in enumerate(call()):
        if not isinstance(g, list):
            out.append(g)
            continue
        d.many_select(j)
        out.append((turn_bytes(g), job_bytes(d)))
    assert len(out) == J
    return out


def both(d, call, J):
    """the group call with the pass and without it -> (results, launches) of each"""
    res = {}
    try:
        for mode in (1, 0):
            d.set_option("linkage_batch", mode)
            d.reset_stats()
            r = group_result(d, call, J)
            res[mode] = (r, {k: d.kernel_stats(k)["launches"] for k in JOBS_KERNELS + ("linkage_heap",)})
    finally:
        d.set_option("linkage_batch", 0)
    return res


def taken(res, jobs_with_linkage):
    (r1, k1), (r0, k0) = res[1], res[0]
    assert r1 == r0
    assert k1["linkage_heap_jobs"] == 1 and k1["pdist_jobs"] == 1 and k1["row_nn_jobs"] == 1 and k1["linkage_heap"] == 0, k1
    assert k0["linkage_heap_jobs"] == 0 and k0["pdist_jobs"] == 0 and k0["row_nn_jobs"] == 0 and 2 <= k0["linkage_heap"] <= jobs_with_linkage, k0


def skipped(res):
    (r1, k1), (r0, k0) = res[1], res[0]
    assert r1 == r0
    assert all(k1[k] == 0 and k0[k] == 0 for k in JOBS_KERNELS), (k1, k0)
    assert k1["linkage_heap"] == k0["linkage_heap"]


def test_diarize_many_with_and_without_the_pass(diarizer):
    recs = recordings()
    for bad in (2, -1):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.set_option("linkage_batch", bad)
        assert e.value.code == 1
    res = both(diarizer, lambda: diarizer.diarize_many(recs), 6)
    r1 = res[1][0]
    assert r1[3] == SD_ERR_SHORT and all(isinstance(r, tuple) and len(r[0]) > 0 for j, r in enumerate(r1) if j != 3)
    taken(res, 5)
    ms = diarizer.stage_ms()
    assert ms[2] > 0 and ms[3] >= ms[0] + ms[1] + ms[2] - 1e-6


def test_diarize_many_under_max_num_embeddings(diarizer):
    recs = recordings()
    plain = group_result(diarizer, lambda: diarizer.diarize_many(recs), 6)
    try:
        diarizer.set_option("max_num_embeddings", 40)
        res = both(diarizer, lambda: diarizer.diarize_many(recs), 6)
    finally:
        diarizer.set_option("max_num_embeddings", -1)
    taken(res, 5)
    assert res[1][0] != plain                      # the sample took part: the longer recordings have more than 40 train rows


def test_three_streams_after_two_rounds_of_pushes(diarizer):
    pcm = pcm75()
    streams = [diarizer.stream() for _ in range(3)]
    try:
        for rnd in range(2):
            diarizer.stream_push_many(streams, [pcm[96000 * i + rnd * 200000 + 13 * i * rnd:96000 * i + (rnd + 1) * 200000 + 31 * i] for i in range(3)])
        res = both(diarizer, lambda: diarizer.stream_turns_many(streams), 3)
        assert all(isinstance(r, tuple) and len(r[0]) > 0 for r in res[1][0])
        taken(res, 3)
        # a single stream's own call launches none of the pass's kernels, with the option on
        diarizer.set_option("linkage_batch", 1)
        diarizer.reset_stats()
        t = streams[1].turns()
        assert turn_bytes(t) == res[1][0][1][0]
        assert all(diarizer.kernel_stats(k)["launches"] == 0 for k in JOBS_KERNELS) and diarizer.kernel_stats("linkage_heap")["launches"] <= 1
    finally:
        diarizer.set_option("linkage_batch", 0)
        for s in streams:
            s.close()


def test_an_enrolled_gallery_skips_the_pass(diarizer):
    recs = recordings()
    rng = np.random.default_rng(8)
    try:
        diarizer.set_enrolled(rng.standard_normal((3, 192)))
        skipped(both(diarizer, lambda: diarizer.diarize_many(recs), 6))
    finally:
        diarizer.set_enrolled(None)


def test_one_cluster_asked_for_skips_the_pass(diarizer):
    recs = recordings()
    try:
        diarizer.set_option("num_clusters", 1)
        res = both(diarizer, lambda: diarizer.diarize_many(recs), 6)
    finally:
        diarizer.set_option("num_clusters", -1)
    skipped(res)
    assert res[1][1]["linkage_heap"] == 0


def test_single_job_entries_launch_no_jobs_kernel(diarizer):
    import torch
    pcm = recordings()[2]
    n = len(pcm)
    nc = sdhip.num_chunks(n)[0]
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(np.array(pcm)).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, 192), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    diarizer.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    try:
        diarizer.set_option("linkage_batch", 1)
        diarizer.reset_stats()
        turns = diarizer.finalize_dev(d_seg.data_ptr(), d_emb.data_ptr(), nc, n)
        assert turns == diarizer.diarize(pcm) and len(turns) > 0
        assert all(diarizer.kernel_stats(k)["launches"] == 0 for k in JOBS_KERNELS) and 1 <= diarizer.kernel_stats("linkage_heap")["launches"] <= 2
        # a group of one is a single job too: nothing to share a launch with
        diarizer.reset_stats()
        (g,) = diarizer.diarize_many([pcm])
        assert g == turns and all(diarizer.kernel_stats(k)["launches"] == 0 for k in JOBS_KERNELS)
    finally:
        diarizer.set_option("linkage_batch", 0)
