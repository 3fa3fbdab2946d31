"""world_size-2 gloo test (CPU) of the multi-GPU data path: shard planning, the padded
all-gather of per-rank segmentation scores / embeddings, and the rank-0 assembly must reproduce the
single-process arrays.  The per-rank "inference" is a deterministic function of the chunk index
(the HIP kernels need a GPU; tests/test_gpu_parity.py::test_sharded_equals_unsharded covers them)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sdhip


def _fake_infer(lo, hi):
    idx = torch.arange(lo, hi, dtype=torch.float32)
    seg = (idx[:, None, None] * 0.001 + torch.arange(293)[None, :, None] * 1e-6 + torch.arange(3)[None, None, :] * 1e-9).float()
    emb = (torch.arange(lo * 3, hi * 3, dtype=torch.float32)[:, None] + torch.arange(192)[None, :] / 1000.0)
    return seg.contiguous(), emb.contiguous()


def _worker(rank, world, port, n_total, q, share0=None):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    C, _ = sdhip.num_chunks(n_total)
    per, ranges = sdhip.plan_ranks(n_total, world, share0)
    lo, hi = ranges[rank]
    seg = torch.zeros((per, 293, 3))
    emb = torch.zeros((per * 3, 192))
    s, e = _fake_infer(lo, hi)
    seg[:hi - lo] = s
    emb[:(hi - lo) * 3] = e
    gs = [torch.zeros_like(seg) for _ in range(world)]
    ge = [torch.zeros_like(emb) for _ in range(world)]
    dist.all_gather(gs, seg)
    dist.all_gather(ge, emb)
    if rank == 0:
        G, H = torch.cat(gs), torch.cat(ge)
        pieces = sdhip.gather_pieces(per, ranges)
        S = torch.cat([G[o:o + m] for o, m in pieces])
        E = torch.cat([H[3 * o:3 * (o + m)] for o, m in pieces])
        assert S.shape[0] == C
        s0, e0 = _fake_infer(0, C)
        q.put((bool(torch.equal(S, s0)), bool(torch.equal(E, e0)), per, ranges))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gather_reassembles_single_process_arrays():
    n_total = 16000 * 1300                      # 2591 chunks -> shards of 1312 and 1279 chunks
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_total, q)) for r in range(2)]
    for p in procs:
        p.start()
    ok_s, ok_e, per, ranges = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok_s and ok_e
    assert per % 32 == 0 and ranges[0] == (0, per) and ranges[1][0] == per


def _run(world, n_total, share0):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_total, q, share0)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


def test_three_rank_gather_with_reduced_rank0_share():
    """bench.py's plan for N > 1: rank 0 also finalizes and therefore infers a smaller share (here 10 %, and none at all);
    the padded slots are re-assembled in chunk order"""
    n_total = 16000 * 900
    C, _ = sdhip.num_chunks(n_total)
    ok_s, ok_e, per, ranges = _run(3, n_total, 0.1)
    assert ok_s and ok_e
    assert ranges[0][0] == 0 and 0 < ranges[0][1] < C // 3 and ranges[0][1] % 32 == 0 and ranges[1][0] == ranges[0][1] and ranges[-1][1] == C
    ok_s, ok_e, per, ranges = _run(3, n_total, 0.0)
    assert ok_s and ok_e and ranges[0] == (0, 0) and ranges[1][0] == 0


def test_shard_plan_properties():
    for n_total, world in [(57600000, 1), (57600000 * 2, 2), (57600000 * 8, 8), (944000, 4), (100000, 8)]:
        C, _ = sdhip.num_chunks(n_total)
        for share0 in (None, 0.0, 0.03, 1.0 / max(world, 1)):
            p2, r2 = sdhip.plan_ranks(n_total, world, share0)
            assert len(r2) == world and r2[0][0] == 0 and r2[-1][1] == C and p2 % 32 == 0
            assert all(b == c for (a, b), (c, d) in zip(r2, r2[1:])) and all(lo % 32 == 0 or hi == lo for lo, hi in r2)
            assert all(hi - lo <= p2 for lo, hi in r2) and sum(m for _, m in sdhip.gather_pieces(p2, r2)) == C
        per, ranges = sdhip.plan_shards(n_total, world)
        assert per % 32 == 0 and len(ranges) == world
        assert ranges[0][0] == 0 and ranges[-1][1] == C
        for (a, b), (c, d) in zip(ranges, ranges[1:]):
            assert b == c and a <= b
        for lo, hi in ranges:
            assert hi == lo or (lo * 3) % 32 == 0          # every non-empty shard starts on a reference batch boundary
            s0, s1 = sdhip.shard_sample_range(lo, hi, n_total)
            assert 0 <= s0 <= s1 <= n_total


def _bench_module():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_bench_ranks_hold_every_range_a_measured_rank0_share_can_give_them():
    """bench.py --gpus N measures the rank-0 share on a warm-up job and re-plans; every rank synthesises the hull of its ranges under
    the two extreme shares up front, and whatever share the measurement gives must fall inside it (else the first 8-GPU run would
    find out)"""
    bm = _bench_module()
    for world in (2, 3, 4, 8):
        n_total = 57600000 * world
        C, _ = sdhip.num_chunks(n_total)
        for rank in range(world):
            lo, hi = bm.union_chunk_range(sdhip.shard_plan, n_total, world, rank, C)
            for pm in range(0, int(round(1000.0 / world)) + 1):
                _, rg = sdhip.shard_plan(n_total, world, pm)
                l, h = rg[rank]
                assert h <= l or (lo <= l and h <= hi), (world, rank, pm, (l, h), (lo, hi))
            assert hi - lo <= 2.2 * C / world + 64 * (world + 2)                      # at most about two shares of audio per rank


def test_bench_balanced_rank0_share():
    bm = _bench_module()
    C = 57591
    # no finalize cost -> equal shares; finalize as long as a rank's inference -> rank 0 only finalizes
    assert bm.balanced_rank0_permille([1200.0] * 8, [C / 8.0] * 8, 0.0, C, 8)[0] == 125
    assert bm.balanced_rank0_permille([1200.0] * 8, [C / 8.0] * 8, 1500.0, C, 8)[0] == 0
    pm, rate = bm.balanced_rank0_permille([1200.0] * 8, [C / 8.0] * 8, 600.0, C, 8)
    s0, T = pm / 1000.0, 9600.0
    assert abs((s0 * T + 600.0) - (1 - s0) * T / 7) < 0.02 * T / 8 and abs(rate - 9600.0 / C) < 1e-9
    assert bm.balanced_rank0_permille([1200.0, 1200.0], [C / 2.0] * 2, 135.0, C, 2)[0] == 472


def test_bench_multi_rank_control_flow_dry_run():
    """everything AROUND the library in a `bench.py --gpus N` run -- self-launch of N ranks, gloo rendezvous, the hull of chunk ranges every
    rank synthesises, the rank-0 share measured on a warm job and the re-plan (with the library's own sd_shard_plan and its coverage check),
    barriers, max over ranks, the single-job pass, assembly and relay of the one result line -- runs here without GPUs against a stand-in for
    the library (bench.py --dry-run-control-plane).  No 8-GPU box was available to the builder: this is what protects the first real run
    from a mistake in that code.  The line is marked as a dry run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    for n, extra in ((3, []), (2, ["--rank0-share", "0.25"])):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--dry-run-control-plane", "--hours-per-gpu", "0.05",
                              "--steps", "2", "--warmup", "1", "--full"] + extra, capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        assert j["n_gpus"] == n and j["rccl_ranks"] == n and j["metric"].startswith("DRY-RUN") and "dry-run" in j["data"]
        assert j["config"]["single_job_ms"] > 0 and j["value"] > 0 and j["scaling"] == "weak"
        sr = j["strong_scaling_reading"]
        assert sr["scaling"] == "strong" and sr["value"] > 0 and sr["single_job_ms"] > 0 and "no N > 1 number has been measured" in j["multi_gpu_note"]
        if not extra:
            assert "measured on a warm job" in j["config"]["rank0_share"]
        else:
            assert j["config"]["rank0_share"] is None and "[(0, 192), (192, 711)]" in j["config"]["sharding"]     # 25 % of 711 chunks, rounded to 32


def test_bench_plain_run_leaves_every_extra_leg_to_full():
    """a plain `bench.py` run is set-up, warm-up, the timed steps and the line: every leg that needs work of its own -- with N = 1 the host-PCM
    entry, the job without kernel events and the raw workload, with N > 1 the single-job latency and the strong-scaling reading -- runs only
    with --full, and the headline fields are the same with and without it (stand-in for the library, as above)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    head = ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data")
    for n in (1, 2):
        lines = []
        for full in ([], ["--full"]):
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--dry-run-control-plane", "--hours-per-gpu", "0.05",
                                  "--steps", "2", "--warmup", "1"] + full, capture_output=True, text=True, timeout=300, env=env)
            assert out.returncode == 0, out.stderr[-2000:]
            got = [l for l in out.stdout.splitlines() if l.startswith("{")]
            assert len(got) == 1
            lines.append(json.loads(got[0]))
        plain, full = lines
        assert all(plain[k] == full[k] for k in head) and plain["value"] > 0 and plain["ms_per_step"] > 0
        assert plain["cpu_baseline"] is None and plain["workload_dependence"]["value_raw_workload"] is None
        assert plain["roofline"]["recorded_pmc"] is None and plain["roofline"]["mfma_utilisation_pmc"] is None
        if n == 1:
            assert "value_host_pcm" not in plain and "ms_per_step_without_kernel_events" not in plain and plain["value_cold"]["ms"] > 0
            assert full["value_host_pcm"]["same_turns"] is True and full["ms_per_step_without_kernel_events"]["same_turns"] is True
            assert full["workload_dependence"]["value_raw_workload"]["steps"] == 3
        else:
            assert plain["config"]["single_job_ms"] is None and plain["config"]["single_job_note"] is None and plain["strong_scaling_reading"] is None
            assert full["config"]["single_job_ms"] > 0 and full["strong_scaling_reading"]["value"] > 0


def test_bench_eight_rank_control_flow_at_the_eight_hour_size():
    """VERDICT r04 #7, first-contact insurance: the REAL `bench.py --gpus 8` at the size the driver will ask for -- 8 ranks, one hour each,
    every rank synthesising the hull of its chunk ranges (with the 72 000-sample halo), the measured rank-0 share and the re-plan, the
    timed region, the single-job pass and the strong-scaling leg (one hour in total over the 8 ranks) -- end to end against the stand-in
    for the library, well inside the driver's 1 800 s limit (synthesis time included: it is most of the wall here).  Checked: one JSON line,
    n_gpus / rccl_ranks = 8, weak scaling for `value`, a single-job latency, both readings of BASELINE's metric, the plan's geometry."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-run-control-plane", "--steps", "2", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=1500, env=env)
    wall = time.time() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and out.stdout.rstrip().endswith(lines[0])          # the JSON line is the last thing on stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 8 and j["rccl_ranks"] == 8 and j["steps"] == 2 and j["warmup"] == 1 and j["scaling"] == "weak" and j["higher_is_better"] is True
    assert j["metric"].startswith("DRY-RUN") and "dry-run" in j["data"] and j["vs_baseline"] is None
    assert j["config"]["chunks"] == 57591 and j["config"]["audio_seconds"] == 8 * 3600.0 and j["config"]["single_job_ms"] > 0
    assert "measured on a warm job" in j["config"]["rank0_share"] and "ncclAllGather" in j["config"]["sharding"]
    sr = j["strong_scaling_reading"]
    assert sr["scaling"] == "strong" and sr["chunks"] == 7191 and sr["value"] > 0 and sr["steps"] == 3 and sr["single_job_ms"] > 0
    assert "no N > 1 number has been measured" in j["multi_gpu_note"]
    assert wall < 900.0, wall


def test_bench_prints_its_line_even_if_the_strong_scaling_leg_cannot_finish():
    """the strong-scaling leg is the one part of an N > 1 run no box here could exercise with more than one real rank, so it runs LAST and under a
    watchdog: if it does not finish (here: a budget of 0 s) rank 0 still prints the complete line, with the reason in place of the reading, and every
    rank exits at once (exit code 0) instead of waiting in a collective"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run-control-plane", "--hours-per-gpu", "0.05", "--steps", "1", "--warmup", "0",
                          "--full", "--strong-timeout", "0"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["config"]["single_job_ms"] > 0 and "did not finish" in j["strong_scaling_reading"]["error"]
