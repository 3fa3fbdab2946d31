#!/usr/bin/env python3
"""bench.py -- real-time factor of the MI355X diarization hot path (BASELINE.json metric).

One step = one pass of the whole path (int16 PCM resident in HBM -> speaker turns on the host) over N hours
of synthetic 16 kHz mono audio on N GPUs.  N = 1 is BASELINE.json configs[2] (1 h, single GPU, full pipeline)
through sd_diarize_dev; N > 1 goes through sd_diarize_sharded_dev: every rank runs segmentation + embeddings
for its contiguous chunk range (multiple of 32 chunks), the library all-gathers segmentation
scores and embeddings with RCCL on its own stream, rank 0 runs counting / clustering / reconstruction.

Workload: the audio comes from a 4-talker turn schedule; with seeded random weights the networks do
not follow the talkers, so -- exactly as the survey prescribes -- the networks run at full cost and their outputs
are then replaced by the schedule-derived scores and talker embeddings (sd_set_planted): masks are partial, about
60 % of the items are live, clustering sees 4 speakers, reconstruction emits hundreds of turns.  `--workload raw`
gives the degenerate case of round 1 (K = 1, one turn) for comparison.

Prints ONE JSON line on rank 0.  A plain run does what that line's headline needs and nothing else: set-up (weights, audio,
planted outputs, sd_create, the cold first job), the W warm-up steps, the K timed steps, --dump-outputs, the line.  What it reports
beside the headline comes from those jobs alone, e.g.
  roofline     : the dominant kernel (f32-MFMA conv_gemm) measured live with HIP events on the library's own
                 stream over the timed region
`--full` adds every leg that needs work of its own: the same job through the host-PCM entry and without kernel events, the fp16
and x3 modes, the raw workload, the PMC recording quoted in `roofline`, and
  cpu_baseline : the oracle ("port") timed on this box's host cores on a bounded sample, beside the reference's own compiled
                 clustering / finalize (N = 1 only)
and with N > 1 the single-job latency and the strong-scaling reading.
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

T_PROCESS = time.perf_counter()
ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

HOUR = 3600
SR = 16000
F32_MFMA_PEAK_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
F16_MFMA_PEAK_TFLOPS = 2500.0         # same table: "Peak BF16/FP16 MFMA ~2.5 PF dense"


def git_blob_sha1(path):
    """`git hash-object` of a file (the GPU box has no .git)"""
    data = open(path, "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def cpu_baseline(ws, we, seconds, planted, threads=None):
    """oracle pipeline (torch CPU + C restatement) on `seconds` of the same synthetic audio and the same planted workload"""
    import synth
    from oracle import pipeline_oracle
    pcm = synth.make_pcm(seconds, seed=1234)
    pl = None
    if planted:
        nc = synth.num_chunks(len(pcm))
        sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(seconds, 1234)), len(pcm), 0, nc)
        pl = (sc, synth.planted_embeddings(asg))
    # threads actually used: the cores this process may run on, capped at 32 (torch's intra-op pool
    # collapses on small batches when handed hundreds of threads)
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    torch.set_num_threads(threads or max(1, min(32, avail)))
    t0 = time.time()
    turns = pipeline_oracle.diarize_ref(pcm, ws, we, planted=pl)
    dt = time.time() - t0
    nc = (seconds * SR - 80000) // 8000 + 1
    return {"value": round(seconds / dt, 4), "unit": "x real-time (audio-s / wall-s)", "cores": torch.get_num_threads(),
            "kind": "port", "sample": "first %d s of the synthetic hour (seed 1234, %s workload): %d chunks, %d embedding items, oracle "
            "pipeline (torch-CPU PyanNet/ECAPA fp32 + C restatement), %.1f s wall" % (seconds, "planted" if planted else "raw", nc, 3 * nc, dt),
            "turns": len(turns)}


def reference_clustering_baseline(d, seconds=1800):
    """the one stage of the path whose REFERENCE code builds here: pipeline/src/clustering/clustering.cpp, compiled in place into
    oracle/_ref/libref_clustering.so (oracle/Makefile; the prebuilt .so travels to the GPU box).  Clustering::cluster (pdist + centroid
    linkage + fcluster) on the live planted embeddings of the first `seconds` of the synthetic hour, one host thread as the reference
    runs it, next to the library's sd_cluster on the same rows (host -> device copy included); labels must be identical."""
    import synth
    from oracle import orc
    R = orc.ref()
    if R is None:
        return None
    n = seconds * SR
    nc = synth.num_chunks(n)
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(float(HOUR), 1234, limit=n)), n, 0, nc)
    emb = synth.planted_embeddings(asg).astype(np.float64)
    live = (sc > 0.4442333667381752).sum(1).reshape(-1) > 12
    X = np.ascontiguousarray(emb[live] / np.linalg.norm(emb[live], axis=1, keepdims=True))
    N = len(X)
    T_ref = np.zeros(N, np.int32)
    t0 = time.perf_counter()
    R.ref_cluster(X, N, 192, orc.THRESH_F32, T_ref)
    cpu_s = time.perf_counter() - t0
    d.cluster(X, orc.THRESH_F32)
    t0 = time.perf_counter()
    T_gpu = d.cluster(X, orc.THRESH_F32)
    gpu_ms = (time.perf_counter() - t0) * 1e3
    return {"kind": "reference", "what": "Clustering::cluster of the reference's own clustering.cpp (oracle/_ref, built in place) on the %d live planted embeddings of the "
            "first %d s, 1 host thread, against sd_cluster on the same rows" % (N, seconds), "N": N, "cores": 1, "cpu_s": round(cpu_s, 2),
            "gpu_ms": round(gpu_ms, 2), "ratio": round(cpu_s * 1e3 / gpu_ms, 1), "same_labels": bool(np.array_equal(T_ref, T_gpu))}


def reference_finalize_baseline(d, scores, emb32, n_total, turns, dev):
    """Everything of the reference's speakerDiarization() behind the two networks -- binarize_swf, speaker_count (trim + aggregate +
    np_rint), Cluster::clustering, the inactive rule, reconstruct / to_diarization, to_annotation, finalResult -- run by the REFERENCE'S
    OWN compiled C++ (oracle/_ref/libref_glue.so: the ORT-free line ranges of speakerDiarizer.cpp built unedited, oracle/Makefile) on
    the scores and embeddings of the job that was just timed, one host thread as the reference runs it, next to sd_finalize_dev on the
    same device-resident inputs; the turns must be the job's own, order included."""
    from oracle import orc
    if orc.refglue() is None:
        return None
    G = orc.RefGlue()
    C = scores.shape[0]
    t0 = time.perf_counter()
    t_ref, K = G.finalize(scores, emb32.astype(np.float64), n_total)
    cpu_s = time.perf_counter() - t0
    d_seg, d_emb = torch.from_numpy(scores).to(dev), torch.from_numpy(emb32).to(dev)
    torch.cuda.synchronize()
    d.finalize_dev(d_seg.data_ptr(), d_emb.data_ptr(), C, n_total)
    t0 = time.perf_counter()
    t_gpu = d.finalize_dev(d_seg.data_ptr(), d_emb.data_ptr(), C, n_total)
    gpu_ms = (time.perf_counter() - t0) * 1e3
    return {"kind": "reference", "what": "the reference's own compiled glue (oracle/_ref/libref_glue.so) from segmentation scores + embeddings to sorted turns on the "
            "timed job's %d chunks / %d live items, 1 host thread, against sd_finalize_dev on the same inputs resident in HBM" % (C, int((~np.isnan(emb32[:, 0])).sum())),
            "cores": 1, "cpu_s": round(cpu_s, 2), "gpu_ms": round(gpu_ms, 2), "ratio": round(cpu_s * 1e3 / gpu_ms, 1), "K": K, "turns": len(t_ref),
            "same_turns_as_sd_finalize_dev": t_ref == t_gpu, "same_turns_as_the_timed_job": t_ref == turns}


def union_chunk_range(plan, n_total, world, rank, C):
    """chunks rank `rank` can be given under any rank-0 share between 0 and 1 / world (plan = sdhip.shard_plan): the hull of its ranges
    under the two extreme plans, widened by 32 * (world + 1) chunks: every range starts on a multiple of 32 chunks and the per-rank share
    is rounded up to one, so rank r's bounds wander by up to 32 r chunks between neighbouring shares"""
    lo_u, hi_u = None, None
    for pm in (0, int(round(1000.0 / world))):
        _, rg = plan(n_total, world, pm)
        l, h = rg[rank]
        if h > l:
            lo_u = l if lo_u is None else min(lo_u, l)
            hi_u = h if hi_u is None else max(hi_u, h)
    if lo_u is None:
        return 0, 0
    return max(0, lo_u - 32 * (world + 1)), min(C, hi_u + 32 * (world + 1))


def balanced_rank0_permille(infer_ms, chunks, finalize_ms, C, world):
    """rank-0 share (per mille of the chunks) at which rank 0's inference + finalize takes as long as another rank's inference.
    infer_ms[r] / chunks[r]: inference time and chunk count of rank r in a measured job; finalize_ms: rank 0's count + clustering +
    reconstruction of the whole job.  With T = inference of all C chunks on one rank: s0 * T + F = (1 - s0) * T / (world - 1)."""
    rate = sum(infer_ms) / max(sum(chunks), 1.0)
    T = rate * C
    s0 = (1.0 - (world - 1) * finalize_ms / max(T, 1e-9)) / world
    s0 = max(0.0, min(1.0 / world, s0))
    return int(round(1000 * s0)), rate


class ControlPlaneStandIn:
    """`--dry-run-control-plane`: stands in for sdhip.Diarizer so that everything AROUND the library in a multi-rank run -- self-launch,
    rendezvous, the union of chunk ranges, the measured rank-0 share and the re-plan, barriers, max over ranks, assembly of the result line --
    can run on a box without GPUs (tests/test_distributed_cpu.py).  It does no diarization: a call checks, exactly as the library does, that
    the samples it is handed cover the rank's chunk range under the plan in force (the real sd_shard_plan), sleeps for a time proportional to
    its chunks (rank 0 also for a finalize that grows with the job), and meets the other ranks in a gloo all-reduce where the library has its
    RCCL all-gather.  The line it leads to says "dry-run" in `metric` and `data` and can never be mistaken for a measurement."""

    def __init__(self, rank, world, dist, plan, num_chunks):
        self.rank, self.world, self.dist, self.plan, self.num_chunks = rank, world, dist, plan, num_chunks
        self.opt = {"rank0_permille": -1}
        self.st = [0.0, 0.0, 0.0, 0.0]
        self.jobs = 0
        self.comm = 0

    def set_option(self, k, v):
        self.opt[k] = int(v)

    def set_planted(self, *a):
        pass

    def comm_init(self, ident, rank, world):
        assert len(ident) == 128 and rank == self.rank and world == self.world
        self.comm = world

    def comm_info(self):
        return self.rank, self.comm

    def diarize_sharded_dev(self, ptr, first, samples, n_total):
        import torch
        C, _ = self.num_chunks(n_total)
        per, ranges = self.plan(n_total, self.world, self.opt["rank0_permille"])
        lo, hi = ranges[self.rank]
        t0 = time.perf_counter()
        if hi > lo:
            need_lo, need_hi = lo * 8000, min(n_total, (hi - 1) * 8000 + 80000)
            if not ptr or first > need_lo or first + samples < need_hi:
                raise RuntimeError("rank %d: samples [%d,%d) do not cover chunks [%d,%d)" % (self.rank, first, first + samples, lo, hi))
            time.sleep(2e-5 * (hi - lo))
        t1 = time.perf_counter()
        flag = torch.zeros(1, dtype=torch.float64)
        if self.world > 1:
            self.dist.all_reduce(flag)                       # where the library has its all-gather
        fin = 0.0
        if self.rank == 0:
            time.sleep(4e-6 * C)
            fin = 4e-3 * C
        self.st = [0.3 * (t1 - t0) * 1e3, 0.7 * (t1 - t0) * 1e3, fin, (time.perf_counter() - t0) * 1e3]
        self.jobs += 1
        return [(0.5, 1.5, 0), (2.0, 3.0, 1)] if self.rank == 0 else []

    def diarize_dev(self, ptr, n_total):
        return self.diarize_sharded_dev(ptr, 0, n_total, n_total)

    def diarize(self, pcm):
        return self.diarize_sharded_dev(1, 0, len(pcm), len(pcm))

    def stage_ms(self):
        return list(self.st)

    def kernel_stats(self, name):
        return {"ms": 1.0 * self.jobs, "launches": self.jobs, "flops": 1e9 * self.jobs, "bytes": 1e6 * self.jobs}

    def reset_stats(self):
        self.jobs = 0

    def read_ws(self, name, dtype, count, offset=0):
        return np.ones(count, dtype)

    def close(self):
        pass


def dump_outputs(out_dir, turns):
    """the turns one timed step returned, as float64 arrays in the order the library returned them (a few hundred turns per hour: far below 64 MB)"""
    os.makedirs(out_dir, exist_ok=True)
    t = np.asarray([(s, e, k) for (s, e, k) in turns], np.float64).reshape(-1, 3)
    for j, name in enumerate(("turns_start", "turns_end", "turns_label")):
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(t[:, j]))


def self_launch(n):
    """`python bench.py --gpus N` (no torchrun): start N ranks as child processes of this one, which never touches the GPU.
    stdout of rank 0 is relayed (the JSON line); every rank's stderr goes to this process's stderr with a rank prefix.  The first
    rank that exits non-zero ends the job: the others are terminated by their exact pids.  Returns the exit code."""
    import socket
    import subprocess
    import threading
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                    "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")})
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    lines0 = []

    def pump(r, stream, is_out):
        for line in stream:
            if is_out and r == 0:
                lines0.append(line)
            else:
                sys.stderr.write("[rank %d] %s" % (r, line))
                sys.stderr.flush()

    threads = [threading.Thread(target=pump, args=(r, p.stdout, True), daemon=True) for r, p in enumerate(procs)]
    threads += [threading.Thread(target=pump, args=(r, p.stderr, False), daemon=True) for r, p in enumerate(procs)]
    for t in threads:
        t.start()
    failed = None
    live = set(range(n))
    while live and failed is None:
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is None:
                continue
            live.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
        time.sleep(0.05)
    if failed is not None:
        t_end = time.time() + 5.0                      # the others usually fail by themselves (their reasons are worth reading)
        while time.time() < t_end and any(procs[r].poll() is None for r in live):
            time.sleep(0.05)
        for r in live:
            if procs[r].poll() is None:
                procs[r].kill()
        for p in procs:
            p.wait()
    for t in threads:
        t.join(timeout=5.0)
    if failed is not None:
        codes = [p.returncode for p in procs]
        sys.stderr.write("bench.py --gpus %d: rank %d exited with code %s (all ranks: %s); no result line\n" % (n, failed[0], failed[1], codes))
        return 1
    out = [l for l in lines0 if l.strip().startswith("{")]
    if len(out) != 1:
        sys.stderr.write("bench.py --gpus %d: rank 0 printed %d result lines\n" % (n, len(out)))
        return 1
    try:
        got = json.loads(out[0]).get("n_gpus")
    except Exception:
        got = None
    if got != n:
        sys.stderr.write("bench.py --gpus %d: the result line says n_gpus = %r; refused\n" % (n, got))
        return 1
    sys.stdout.write(out[0])
    sys.stdout.flush()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hours-per-gpu", type=float, default=1.0)
    ap.add_argument("--cpu-seconds", type=int, default=60, help="--full: audio seconds for the cpu_baseline sample (0 = skip)")
    ap.add_argument("--ref-finalize", type=int, default=1, help="--full, N = 1, planted workload of at most 1 h: also run the REFERENCE's own compiled glue (oracle/_ref/"
                    "libref_glue.so) from scores + embeddings to turns on the timed job and report it under cpu_baseline.reference_finalize (~45 s of host time; 0 = skip)")
    ap.add_argument("--workload", default="planted", choices=["planted", "raw"], help="planted = SURVEY 8d (network outputs replaced by the "
                    "schedule-derived scores / talker embeddings after the networks ran); raw = whatever the random-weight networks say (K = 1)")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16", "x3"], help="f32 = the measured configuration (f32 MFMA); f16 = "
                    "BASELINE configs[4]: ECAPA conv layers on the fp16 MFMA with f32 accumulation (secondary, tolerance-checked mode); x3 = f32 tensors, "
                    "both operands of the ECAPA conv layers split into hi + lo fp16 halves on the fp16 MFMA (opt-in mode; an f32 run with --full reports it in its `x3` object)")
    ap.add_argument("--rank0-share", type=float, default=-1.0, help="fraction of the chunks rank 0 infers itself (it also finalizes: count / "
                    "clustering / reconstruction).  The other ranks return from the sharded call once the exchange is done, so rank 0's "
                    "finalize(k) overlaps their inference(k+1); a smaller rank-0 share balances the two. -1 = measured: the warm-up job runs with equal "
                    "shares and its stage times give the balance point; 1/N = equal shares, 0 = rank 0 only finalizes")
    ap.add_argument("--fp16-steps", type=int, default=3, help="--full, N = 1, f32 run: also time this many steps in fp16 mode (BASELINE configs[4]) and put them, with the "
                    "cosine distances of the fp16 embeddings to the f32 ones, into the `fp16` object of the result line (0 = skip)")
    ap.add_argument("--raw-steps", type=int, default=3, help="--full, N = 1, planted run: also time this many jobs on the RAW network outputs (every item live and full length) -> workload_dependence.value_raw_workload")
    ap.add_argument("--x3-steps", type=int, default=3, help="--full, N = 1, f32 run: also time this many steps with ecapa_precision = 3 (f32 tensors, split fp16 operands on the "
                    "MFMA) and put them into the `x3` object of the result line (0 = skip)")
    ap.add_argument("--strong-steps", type=int, default=3, help="--full, N > 1: also time this many jobs of ONE hour in total sharded over the N GPUs (the strong reading of the "
                    "metric; 0 = skip); reported as `strong_scaling_reading`")
    ap.add_argument("--strong-timeout", type=int, default=600, help="--full, N > 1: seconds the strong-scaling leg may take before the line is printed without it")
    ap.add_argument("--dry-run-control-plane", action="store_true", help="no GPU work: a stand-in for the library (ControlPlaneStandIn) lets the multi-rank control "
                    "flow of this script run on a box without GPUs; the line says dry-run and is not a measurement")
    ap.add_argument("--force-dist", action="store_true", help="take the multi-rank code path (RCCL communicator inside the library, "
                    "all-gather, assembly) even with one rank")
    ap.add_argument("--opt", action="append", default=[], help="library option key=value (sd_set_option), e.g. emb_batch_items=1536; tuning only")
    ap.add_argument("--full", action="store_true", help="also run every leg that needs work of its own (the options marked --full; with N = 1 also the "
                    "host-PCM entry and the job without kernel events, with N > 1 the single-job latency) and quote the PMC recording in `roofline`; "
                    "a plain run does only set-up, warm-up and the timed steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step returned (the speaker "
                    "turns) as DIR/turns_start.npy, DIR/turns_end.npy, DIR/turns_label.npy (float64): two builds compared output for output")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:
        a.cpu_seconds, a.fp16_steps, a.x3_steps, a.raw_steps, a.strong_steps = 0, 0, 0, 0, 0

    # ---- N > 1 without a launcher: this process becomes the launcher.  It starts N fresh children (one rank per GPU) with
    # RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, BEFORE anything here touches the GPU (no torch.cuda call above this line), relays
    # rank 0's JSON line and exits non-zero if any rank does.  Nothing re-execs: the children are new processes.
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a.gpus))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        # a line whose n_gpus is not what was asked for would be mistaken for the N-GPU number
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: refusing to measure a different job than the one asked for" % (a.gpus, world))
    dry = a.dry_run_control_plane
    gpu_sync = (lambda: None) if dry else torch.cuda.synchronize
    if dry:
        dev = torch.device("cpu")
        a.cpu_seconds, a.fp16_steps, a.x3_steps = 0, 0, 0
    else:
        ndev = torch.cuda.device_count()                 # (counting devices does not initialise the GPU)
        if ndev <= 0:
            raise SystemExit("bench.py rank %d: needs a GPU: libsdhip has no CPU fallback" % rank)
        if local >= ndev:
            raise SystemExit("bench.py rank %d: LOCAL_RANK %d but this node has %d GPU%s" % (rank, local, ndev, "" if ndev == 1 else "s"))
        if not torch.cuda.is_available():
            raise SystemExit("bench.py rank %d: needs a GPU: libsdhip has no CPU fallback" % rank)
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    use_dist = world > 1 or a.force_dist
    dist = None
    if world > 1:
        # control plane only (rendezvous-id broadcast, barriers, max over ranks): the data-path collective is the
        # RCCL all-gather inside libsdhip.so
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29577")
        import torch.distributed as dist
        import datetime
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=600))      # a rank that dies must not leave the others waiting for half an hour

    import sdhip
    import synth
    import weightpack as nn                     # seeded synthetic weights + .sdw container (package data, not the oracle)

    tmp = tempfile.mkdtemp(prefix="sdw_r%d_" % rank)
    ws, we = nn.synth_segmentation_weights(4321), nn.synth_embedding_weights(4322)
    nn.save_pack(os.path.join(tmp, "segment.sdw"), ws)
    nn.save_pack(os.path.join(tmp, "embedding.sdw"), we)

    # ---- the job: `world` x hours_per_gpu of audio; rank r owns a contiguous, 32-aligned chunk range
    per_samples = int(round(a.hours_per_gpu * HOUR * SR))
    n_total = per_samples * world
    C, _ = sdhip.num_chunks(n_total)
    # rank 0 also finalizes (count / clustering / reconstruction), so it is given a smaller share of the chunks.  The share is not a
    # constant of this script: the first warm-up job runs with equal shares, its stage times (every rank's inference, rank 0's finalize)
    # give the share that balances rank 0's inference + finalize against the others' inference, and the plan is changed before the
    # timed region.  Every rank therefore synthesises the chunks it can be given under ANY share between 0 and 1 / N.
    permille = -1
    if world > 1:
        permille = int(round(1000 * a.rank0_share)) if a.rank0_share >= 0 else int(round(1000.0 / world))
    per, ranges = sdhip.shard_plan(n_total, world, permille)
    lo_u, hi_u = ranges[rank]
    if world > 1 and a.rank0_share < 0:
        ul, uh = union_chunk_range(sdhip.shard_plan, n_total, world, rank, C)
        lo_u, hi_u = min(lo_u, ul), max(hi_u, uh)
    lo, hi = lo_u, hi_u                       # chunks this rank holds samples and planted outputs for
    first, need_hi = sdhip.shard_sample_range(lo, hi, n_total)
    # synthesise only what this rank can read: its own hour(s) + the 72 000-sample halo of the next one
    pieces, turns_sched, pos = [], [], first
    h_lo, h_hi = first // per_samples, max(first, need_hi - 1) // per_samples
    for h in range(h_lo, min(h_hi, world - 1) + 1):
        for (s, e, k, ov) in synth.with_duets(synth.schedule(a.hours_per_gpu * HOUR, 1234 + h, limit=None if h < h_hi else max(1, need_hi - h * per_samples))):
            turns_sched.append((s + h * per_samples, e + h * per_samples, k, ov))
    while pos < need_hi:
        h = pos // per_samples
        off = pos - h * per_samples
        take = min(per_samples - off, need_hi - pos)
        seg_pcm = synth.make_pcm(a.hours_per_gpu * HOUR, seed=1234 + h, limit=off + take)
        pieces.append(seg_pcm[off:off + take])
        pos += take
    pcm_host = np.concatenate(pieces) if pieces else np.zeros(1, np.int16)
    planted = a.workload == "planted"
    if planted and hi > lo:
        p_scores, p_assign = synth.planted_scores(turns_sched, n_total, lo, hi)
        p_emb = synth.planted_embeddings(p_assign, chunk_lo=lo)
        d_ps, d_pe = torch.from_numpy(p_scores).to(dev), torch.from_numpy(p_emb).to(dev)

    # ---- cold start: context creation (weights -> HBM), PCM upload, first job with cold workspaces
    t_lib = time.perf_counter()
    if not dry:
        sdhip.lib()                              # dlopen of libsdhip.so (+ librccl.so behind it): process start-up, like the HIP runtime's initialisation above
    lib_load_ms = (time.perf_counter() - t_lib) * 1e3
    gpu_sync()
    t_cold = time.perf_counter()
    d = (ControlPlaneStandIn(rank, world, dist, sdhip.shard_plan, sdhip.num_chunks) if dry else
         sdhip.Diarizer(os.path.join(tmp, "segment.sdw"), os.path.join(tmp, "embedding.sdw"), local))
    if a.precision != "f32":
        d.set_option("ecapa_precision", 1 if a.precision == "f16" else 3)
        if a.precision == "x3":
            d.set_option("seg_precision", 3)
    for kv in a.opt:
        k, v = kv.split("=")
        d.set_option(k, int(v))
    t_created = time.perf_counter()
    d_pcm = torch.from_numpy(pcm_host).to(dev)
    gpu_sync()
    t_uploaded = time.perf_counter()
    if planted and hi > lo:
        d.set_planted(d_ps.data_ptr(), d_pe.data_ptr(), lo, hi - lo)
    if use_dist:
        if rank == 0:
            ident = [bytes(128) if dry else sdhip.comm_unique_id()]
        else:
            ident = [None]
        if world > 1:
            dist.broadcast_object_list(ident, src=0)
        d.set_option("rank0_permille", permille)
        d.comm_init(ident[0], rank, world)
    my_lo, my_hi = ranges[rank]                # the rank's chunk range under the plan in force

    turns_box = [None]

    def step():
        if use_dist:
            t = d.diarize_sharded_dev(d_pcm.data_ptr() if hi > lo else 0, first, int(d_pcm.numel()) if hi > lo else 0, n_total)
            if rank == 0:
                turns_box[0] = t
        else:
            turns_box[0] = d.diarize_dev(d_pcm.data_ptr(), n_total)

    def fence():
        gpu_sync()
        if world > 1:
            dist.barrier()
        gpu_sync()

    step()
    fence()
    cold_ms = (time.perf_counter() - t_cold) * 1e3
    share_note = None
    if world > 1 and a.rank0_share < 0:
        # the balance point from the job that just ran (equal shares): rank 0 spends s0 * T + F, the others (1 - s0) * T / (N - 1), where
        # T = inference time of the whole recording on one rank and F = finalize; equal at s0 = (1 - (N - 1) * F / T) / N
        step()                                   # a warm job with the equal shares: its stage times are the measurement
        fence()
        st = d.stage_ms()
        mine = torch.tensor([st[0] + st[1], st[2] if rank == 0 else 0.0, float(my_hi - my_lo)], dtype=torch.float64)
        allv = [torch.zeros(3, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(allv, mine)
        pm_new, rate = balanced_rank0_permille([float(v[0]) for v in allv], [float(v[2]) for v in allv], float(allv[0][1]), C, world)
        per_new, ranges_new = sdhip.shard_plan(n_total, world, pm_new)
        fits = torch.tensor([1.0 if (ranges_new[rank][1] <= ranges_new[rank][0] or (lo <= ranges_new[rank][0] and ranges_new[rank][1] <= hi)) else 0.0], dtype=torch.float64)
        dist.all_reduce(fits, op=dist.ReduceOp.MIN)
        if float(fits.item()) > 0.5:
            permille, per, ranges = pm_new, per_new, ranges_new
            my_lo, my_hi = ranges[rank]
            d.set_option("rank0_permille", permille)
            share_note = ("measured on a warm job with equal shares: inference %.3f ms per chunk and rank, finalize %.1f ms -> rank 0 infers %.1f %% of the chunks"
                          % (rate, float(allv[0][1]), permille / 10.0))
            step()
            fence()
        else:
            share_note = "balanced share %d per mille needs chunks outside what a rank synthesised: equal shares kept" % pm_new
    # W untimed warm-up steps BEHIND the cold job (which is a measurement of its own, `value_cold`, not a warm-up: a context's first embedding call plans
    # small batches so that a one-shot CLI process does not pay ~1.6 s of hipMalloc for the full activation arena, and the SECOND job grows it --
    # + 8 ms at 1 h, + 1.7 s at the 8-h size; with the cold job counted as a warm-up that growth fell into the first timed step of `--warmup 1` runs)
    for _ in range(max(0, a.warmup)):
        step()
    d.set_option("profile", 1)
    d.reset_stats()
    fence()
    t0 = time.perf_counter()
    step_marks = [t0]
    for _ in range(a.steps):
        step()
        step_marks.append(time.perf_counter())      # (the call returns the turns, i.e. it has synchronised: a timestamp, no extra fence inside the bracket)
    fence()
    dt = time.perf_counter() - t0
    step_ms = sorted((step_marks[i + 1] - step_marks[i]) * 1e3 for i in range(a.steps))
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    ms_per_step = dt / max(a.steps, 1) * 1e3
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, turns_box[0] or [])
    audio_s = n_total / SR
    stats_live = d.kernel_stats("items_live")
    live_local = stats_live["flops"] / max(stats_live["launches"], 1)
    # dominant kernel: k_conv_gemm.  f32 mode: every launch is the f32-MFMA instantiation.  fp16 mode: the roofline is that of the fp16
    # instantiations (ECAPA per-frame layers: k_conv_gemm_h256 + k_conv_gemm<F16>); the f32 launches left (PyanNet) are listed beside it
    cg_all = d.kernel_stats({"f16": "conv_gemm_f16", "x3": "conv_gemm_x3"}.get(a.precision, "conv_gemm"))      # every MFMA convolution launch of the precision
    cg = d.kernel_stats({"f16": "conv_w256_f16", "x3": "conv_w256_x3"}.get(a.precision, "conv_w256_f32"))       # the dominant kernel alone: k_conv_gemm_w256
    if a.precision == "x3":          # executed MFMA work: three fp16 products per algorithmic multiply-add
        cg, cg_all = dict(cg, flops=3.0 * cg["flops"]), dict(cg_all, flops=3.0 * cg_all["flops"])
    cg_f32 = d.kernel_stats("conv_gemm_f32")
    cg_e, cg_s = d.kernel_stats("conv_w256_ecapa"), d.kernel_stats("conv_w256_seg")
    stages = d.stage_ms()
    extra = {}
    for k in ("stft_mel", "lstm_rec", "pdist", "linkage", "linkage_hx", "linkage_heap", "row_nn", "se_apply", "asp_pool", "rccl_all_gather"):
        s = d.kernel_stats(k)
        if s["launches"] == 0:
            continue
        extra[k] = {"ms_per_step": round(s["ms"] / max(a.steps, 1), 3), "launches_per_step": s["launches"] // max(a.steps, 1)}
        if k == "stft_mel" and s["ms"] > 0:
            # front end (north star: HBM GB/s for the STFT).  Bytes = what the launch really touches by SURVEY 8(d)'s rule: the selected samples of the live
            # items + their mask rows read, the stored frames x 96 floats written (a partial item reads fewer than 80 000 samples and stores fewer than 501
            # rows).  The kernel is not HBM-bound: it is bound by VALU issue on the fp64 FFT the reference's precision asks for (1.9 G VALU
            # wave-instructions per launch = more than 43 % of the chip's VALU issue slots for its whole duration).
            extra[k].update({"hbm_GBps_algorithmic": round(s["bytes"] / s["ms"] / 1e6, 1), "hbm_frac_of_8TBps": round(s["bytes"] / s["ms"] / 1e6 / 8000.0, 4),
                             "algorithmic_MB_per_launch": round(s["bytes"] / max(s["launches"], 1) / 1e6, 1), "GFLOPs_fft_fp64_plus_mel_f32": round(s["flops"] / s["ms"] / 1e6, 1),
                             "bound": "per-tile latency chain (gather, three LDS exchanges, mel pass): neither HBM nor the fp64 FFT alone -- the kernel without its FFT arithmetic takes 5.5 of 7.2 ms"})
            # the bound it really has: vector-ALU time.  Of the billed FLOPs 15 000 per frame are the fp64 FFT (fp64 vector peak 78.6 TFLOP/s), 2 x 201 x 80 the f32
            # mel contraction (f32 vector peak 157.3 TFLOP/s): the fraction of the launch's duration those FLOPs would need at the two peaks
            f64_share = 15000.0 / (15000.0 + 201.0 * 80 * 2)
            extra[k].update({"fft_fp64_TFLOPs": round(s["flops"] * f64_share / s["ms"] / 1e9, 2), "frac_of_fp64_vector_peak": round(s["flops"] * f64_share / s["ms"] / 1e9 / 78.6, 4),
                             "frac_of_vector_alu_roofline": round((s["flops"] * f64_share / 78.6e12 + s["flops"] * (1.0 - f64_share) / 157.3e12) / (s["ms"] * 1e-3), 4),
                             "ms_at_60pct_hbm": round(s["bytes"] / max(s["launches"], 1) / (0.6 * 8e12) * 1e3, 3),
                             "ms_at_vector_alu_peaks": round((s["flops"] * f64_share / 78.6e12 + s["flops"] * (1.0 - f64_share) / 157.3e12) / max(s["launches"], 1) * 1e3, 3),
                             "roofline_note": "the north star's '>= 60 % of the HBM roofline on the STFT' is out of reach with the reference's fp64 STFT (sd.cpp:1980-2013): the launch's arithmetic "
                                              "alone needs `ms_at_vector_alu_peaks` at 100 % of the fp64 / f32 vector peaks, more than twice `ms_at_60pct_hbm`; ablations in profiles/r05_frontend_ablation_a.txt / _b.txt"})
    kst = d.kernel_stats("clusters_K")

    # ---- one job at a time (no overlap between consecutive jobs): the latency a single recording sees on N GPUs
    single_job_ms = None
    if world > 1:
        if a.full:
            d.set_option("profile", 0)
            lat = []
            for _ in range(2):
                fence()
                t1 = time.perf_counter()
                step()
                fence()
                tl = torch.tensor([time.perf_counter() - t1], dtype=torch.float64)
                dist.all_reduce(tl, op=dist.ReduceOp.MAX)
                lat.append(float(tl.item()) * 1e3)
            single_job_ms = round(min(lat), 2)
        ll = torch.tensor([live_local], dtype=torch.float64)
        dist.all_reduce(ll, op=dist.ReduceOp.SUM)
        live_total = float(ll.item())
    else:
        live_total = live_local

    # ---- the STRONG reading of BASELINE's metric ("1 h 16 kHz mono on 1 / 2 / 4 / 8 MI355X"): ONE hour in total, sharded over the N ranks
    # (`value` above is the weak reading: N hours on N GPUs).  Same communicator, same library calls; every rank synthesises its slice of that hour
    # (the hull of its ranges under any rank-0 share), the share is balanced from a measured warm job as above, then `steps` jobs are timed.
    def strong_leg():
        """runs on EVERY rank (collectives inside); returns the `strong_scaling_reading` object"""
        n_s = per_samples if a.hours_per_gpu <= 1.0 else int(round(HOUR * SR))
        C_s, _ = sdhip.num_chunks(n_s)
        pm_s = int(round(1000.0 / world))
        per_s, ranges_s = sdhip.shard_plan(n_s, world, pm_s)
        ul, uh = union_chunk_range(sdhip.shard_plan, n_s, world, rank, C_s)
        lo_s, hi_s = min(ranges_s[rank][0], ul), max(ranges_s[rank][1], uh)
        if ranges_s[rank][1] <= ranges_s[rank][0] and uh <= ul:
            lo_s, hi_s = 0, 0
        first_s, need_s = sdhip.shard_sample_range(lo_s, hi_s, n_s) if hi_s > lo_s else (0, 0)
        sec_s = n_s / SR
        pcm_s = synth.make_pcm(sec_s, seed=1234, limit=max(need_s, 1))[first_s:need_s] if hi_s > lo_s else np.zeros(1, np.int16)
        d_pcm_s = torch.from_numpy(np.ascontiguousarray(pcm_s)).to(dev)
        if planted and hi_s > lo_s:
            sched_s = synth.with_duets(synth.schedule(sec_s, 1234))
            ps_s, as_s = synth.planted_scores(sched_s, n_s, lo_s, hi_s)
            pe_s = synth.planted_embeddings(as_s, chunk_lo=lo_s)
            d_ps_s, d_pe_s = torch.from_numpy(ps_s).to(dev), torch.from_numpy(pe_s).to(dev)
            d.set_planted(d_ps_s.data_ptr(), d_pe_s.data_ptr(), lo_s, hi_s - lo_s)
        else:
            d.set_planted(0, 0, 0, 0)
        d.set_option("profile", 0)
        d.set_option("rank0_permille", pm_s)

        def step_s():
            return d.diarize_sharded_dev(d_pcm_s.data_ptr() if hi_s > lo_s else 0, first_s, int(d_pcm_s.numel()) if hi_s > lo_s else 0, n_s)

        step_s(); fence()
        step_s(); fence()                        # warm, equal shares: the measurement for the balance
        st = d.stage_ms()
        mine = torch.tensor([st[0] + st[1], st[2] if rank == 0 else 0.0, float(ranges_s[rank][1] - ranges_s[rank][0])], dtype=torch.float64)
        allv = [torch.zeros(3, dtype=torch.float64) for _ in range(world)]
        if world > 1:
            dist.all_gather(allv, mine)
        else:
            allv = [mine]
        pm_b, _ = balanced_rank0_permille([float(v[0]) for v in allv], [float(v[2]) for v in allv], float(allv[0][1]), C_s, world) if world > 1 else (pm_s, 0.0)
        _, rg_b = sdhip.shard_plan(n_s, world, pm_b)
        fits = torch.tensor([1.0 if (rg_b[rank][1] <= rg_b[rank][0] or (lo_s <= rg_b[rank][0] and rg_b[rank][1] <= hi_s)) else 0.0], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(fits, op=dist.ReduceOp.MIN)
        if float(fits.item()) > 0.5:
            pm_s, ranges_s = pm_b, rg_b
            d.set_option("rank0_permille", pm_s)
        step_s(); fence()
        t1 = time.perf_counter()
        turns_s = None
        for _ in range(a.strong_steps):
            turns_s = step_s()
        fence()
        ts_ = torch.tensor([time.perf_counter() - t1], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(ts_, op=dist.ReduceOp.MAX)
        ms_s = float(ts_.item()) / a.strong_steps * 1e3
        lat_s = []
        for _ in range(2):
            fence()
            t1 = time.perf_counter()
            step_s()
            fence()
            tl = torch.tensor([time.perf_counter() - t1], dtype=torch.float64)
            if world > 1:
                dist.all_reduce(tl, op=dist.ReduceOp.MAX)
            lat_s.append(float(tl.item()) * 1e3)
        strong = {"what": "the strong reading of the metric: ONE recording of %g h sharded over the %d GPUs (`value` is the weak reading: %g h per GPU)" % (sec_s / HOUR, world, a.hours_per_gpu),
                  "value": round(sec_s / (ms_s / 1e3), 2), "unit": "x real-time", "ms_per_step": round(ms_s, 2), "steps": a.strong_steps, "scaling": "strong",
                  "single_job_ms": round(min(lat_s), 2), "chunks": C_s, "turns": len(turns_s or []),
                  "sharding": "ranges %s, rank 0 infers %.1f %% of the chunks" % (ranges_s[:8], 100.0 * (ranges_s[0][1] - ranges_s[0][0]) / max(C_s, 1))}
        # back to the headline job's plan and planted outputs
        d.set_option("rank0_permille", permille)
        if planted and hi > lo:
            d.set_planted(d_ps.data_ptr(), d_pe.data_ptr(), lo, hi - lo)
        return strong

    # ---- N = 1 extras: the same job handed over as HOST PCM (sd_diarize: H2D copy inside the call), the cold first job, and the fp16 mode
    extra_lines = {}
    turns = turns_box[0] or []
    if world == 1 and not use_dist:
        d.set_option("profile", 0)
        if a.full:
            ts = []
            for _ in range(2):
                gpu_sync()
                t1 = time.perf_counter()
                th = d.diarize(pcm_host[:n_total])
                ts.append(time.perf_counter() - t1)
            extra_lines["value_host_pcm"] = {"value": round(audio_s / min(ts), 2), "ms": round(min(ts) * 1e3, 2), "same_turns": th == turns_box[0],
                                             "what": "sd_diarize: int16 PCM in pageable host memory, the 2 * n byte H2D copy and its buffer inside the timed call"}
            # the same job without the HIP-event pairs the timed region carries around every launch (option profile = 1): what the events cost
            tp = []
            for _ in range(3):
                gpu_sync()
                t1 = time.perf_counter()
                tq = d.diarize_dev(d_pcm.data_ptr(), n_total)
                gpu_sync()
                tp.append(time.perf_counter() - t1)
            extra_lines["ms_per_step_without_kernel_events"] = {"ms": round(min(tp) * 1e3, 2), "value": round(audio_s / min(tp), 2), "same_turns": tq == turns_box[0],
                                                                "what": "sd_diarize_dev with profile = 0, best of 3; the timed region above runs with profile = 1 because the roofline "
                                                                        "object is measured live over it"}
        # (the set-up's cold job: no work of its own, so a plain run reports it too)
        extra_lines["value_cold"] = {"value": round(audio_s / (cold_ms / 1e3), 2), "ms": round(cold_ms, 1),
                                     "parts_ms": {"sd_create": round((t_created - t_cold) * 1e3, 1), "pcm_upload": round((t_uploaded - t_created) * 1e3, 1),
                                                  "first_job": round(cold_ms - (t_uploaded - t_cold) * 1e3, 1),
                                                  "library_load_before_the_timer": round(lib_load_ms, 1)},
                                     "what": "what a one-shot user of the CLI sees: sd_create + PCM upload + first job with cold workspaces"}
        def secondary_mode(opt, steps, scope_wide, scope_all, kernel, what, mfma_per_flop):
            """the same job `steps` times with ecapa_precision = opt; its own roofline (the wide kernel of the mode against the fp16 MFMA peak) and the
            cosine distances of its REAL embeddings to the f32 ones"""
            d.set_option("ecapa_precision", opt)
            d.set_option("seg_precision", -1)        # auto (the library's default): any fp16-pipe mode of ECAPA takes the split-operand LSTM too (round 6; before: x3 only)
            d.set_option("profile", 1)
            step()
            d.reset_stats()
            fence()
            t1 = time.perf_counter()
            for _ in range(steps):
                step()
            fence()
            ms_m = (time.perf_counter() - t1) / steps * 1e3
            turns_m = turns_box[0]
            wm, allm = d.kernel_stats(scope_wide), d.kernel_stats(scope_all)
            st_m = d.stage_ms()
            d.set_option("profile", 0)
            cosd = None
            if True:
                # accuracy on the REAL embeddings (planted workload: the planted ones replace them in the timed jobs, so: scores planted, embeddings kept)
                # (segmentation + embedding stages only, sd_shard_infer_dev: the real embeddings of a random-weight network carry exact
                # duplicates, which would send the finalize stage down its 0.8 s tie fallback four times for nothing)
                if planted:
                    d.set_planted(d_ps.data_ptr(), 0, lo, hi - lo)
                seg_t = torch.zeros((C, 293, 3), dtype=torch.float32, device=dev)
                emb_t = torch.zeros((C * 3, 192), dtype=torch.float32, device=dev)
                d.shard_infer_dev(d_pcm.data_ptr(), 0, n_total, n_total, 0, C, seg_t.data_ptr(), emb_t.data_ptr())
                gpu_sync()
                em = emb_t.cpu().numpy().astype(np.float64)
                d.set_option("ecapa_precision", 0)
                d.set_option("seg_precision", -1)
                d.shard_infer_dev(d_pcm.data_ptr(), 0, n_total, n_total, 0, C, seg_t.data_ptr(), emb_t.data_ptr())
                gpu_sync()
                e32 = emb_t.cpu().numpy().astype(np.float64)
                del seg_t, emb_t
                if planted:
                    d.set_planted(d_ps.data_ptr(), d_pe.data_ptr(), lo, hi - lo)
                lv = ~np.isnan(e32[:, 0])
                same_nan = bool(np.array_equal(np.isnan(em[:, 0]), ~lv))
                cd = 1.0 - (em[lv] * e32[lv]).sum(1) / np.linalg.norm(em[lv], axis=1) / np.linalg.norm(e32[lv], axis=1)
                cosd = {"items": int(lv.sum()), "max": float("%.3g" % cd.max()), "q99": float("%.3g" % np.quantile(cd, 0.99)), "median": float("%.3g" % np.median(cd)),
                        "above_1e-3": int((cd > 1e-3).sum()), "same_nan_rows": same_nan}
            d.set_option("ecapa_precision", 0)
            d.set_option("seg_precision", -1)
            tf = wm["flops"] / max(wm["ms"], 1e-9) / 1e9
            rl = {"bound": "mfma", "kernel": kernel, "achieved": round(tf * mfma_per_flop, 1), "peak": F16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                  "frac": round(tf * mfma_per_flop / F16_MFMA_PEAK_TFLOPS, 4), "kernel_ms_per_step": round(wm["ms"] / steps, 2), "launches_per_step": wm["launches"] // steps,
                  "all_conv_launches_of_the_mode_TFLOPs_algorithmic": round(allm["flops"] / max(allm["ms"], 1e-9) / 1e9, 1)}
            if mfma_per_flop != 1:
                rl["achieved_algorithmic"] = round(tf, 1)
                rl["note"] = ("`achieved` counts the MFMA work the kernel executes: %d fp16 products (hi*hi, lo*hi, hi*lo) per algorithmic multiply-add; "
                              "`achieved_algorithmic` = the layer's 2 M N K over the same time, comparable with the f32 line's `roofline.achieved`" % mfma_per_flop)
            return {"what": what, "value": round(audio_s / (ms_m / 1e3), 2), "ms_per_step": round(ms_m, 2), "steps": steps, "same_turns_as_f32": turns_m == turns,
                    "stage_ms_last_step": {"segmentation": round(st_m[0], 1), "embedding": round(st_m[1], 1), "finalize": round(st_m[2], 1)},
                    "roofline": rl, "cosine_distance_to_f32_embeddings": cosd}

        if a.precision == "f32" and a.fp16_steps > 0:
            extra_lines["fp16"] = secondary_mode(1, a.fp16_steps, "conv_w256_f16", "conv_gemm_f16", "k_conv_gemm_pp (conv_gemm_p.hip, round 6: v_mfma_f32_16x16x32_f16, LDS-DMA staged, every wave interleaves its reads and DMAs with its MFMAs, the queue is never drained; "
                                                 "bound by what a CU takes in -- 24 - 27 B per clock = 2 400 - 2 700 cycles per 64 KB K-tile against 2 048 of MFMA, profiles/r06_g256_lab.txt; `peak` is 2.4 GHz x the pipe's "
                                                 "per-clock rate, the chip holds ~ 1.75 GHz under this load; the vendor library's GEMM reaches 1.09 / 1.36 PFLOP/s at the tdnn / MFA shapes on the same box)",
                                                 "BASELINE configs[4]: the same job with the per-frame ECAPA layers on the fp16 MFMA (fp16 weights and activations, f32 accumulation); "
                                                 "secondary mode, never the headline value", 1)
        if a.precision == "f32" and a.fp16_steps > 0 and planted and "fp16" in extra_lines and a.hours_per_gpu <= 2.0:        # (a second context: beside an 8-h job's 80 GB distance matrix the two activation arenas run the GPU out of memory)
            # BASELINE configs[4]'s tolerance on a network whose SE gates are NOT saturated: the same seeded conv weights with BatchNorm statistics learnt from one
            # calibration batch (oracle/nn_oracle.calibrated_embedding_weights; the plain pack above is the stress case: BN = identity, gates pinned at 0 / 1)
            try:
                wc = nn.calibrated_embedding_weights(4322)
                nn.save_pack(os.path.join(tmp, "embedding_cal.sdw"), wc)
                d2 = sdhip.Diarizer(os.path.join(tmp, "segment.sdw"), os.path.join(tmp, "embedding_cal.sdw"), local)
                d2.set_planted(d_ps.data_ptr(), 0, lo, hi - lo)
                res = {}
                embs = {}
                seg2 = torch.zeros((C, 293, 3), dtype=torch.float32, device=dev)
                emb2 = torch.zeros((C * 3, 192), dtype=torch.float32, device=dev)
                for mode, name in ((0, "f32"), (1, "fp16"), (3, "x3")):
                    d2.set_option("ecapa_precision", mode)
                    # inference only (sd_shard_infer_dev): the REAL embeddings of a random-weight network carry exact duplicates, which send the
                    # finalize stage down its tie fallback -- not what this object is about
                    d2.shard_infer_dev(d_pcm.data_ptr(), 0, n_total, n_total, 0, C, seg2.data_ptr(), emb2.data_ptr())
                    gpu_sync()
                    t1 = time.perf_counter()
                    d2.shard_infer_dev(d_pcm.data_ptr(), 0, n_total, n_total, 0, C, seg2.data_ptr(), emb2.data_ptr())
                    gpu_sync()
                    res[name] = {"inference_ms": round((time.perf_counter() - t1) * 1e3, 1)}
                    embs[name] = emb2.cpu().numpy().astype(np.float64)
                lv = ~np.isnan(embs["f32"][:, 0])
                for name in ("fp16", "x3"):
                    e = embs[name]
                    cd = 1.0 - (e[lv] * embs["f32"][lv]).sum(1) / np.linalg.norm(e[lv], axis=1) / np.linalg.norm(embs["f32"][lv], axis=1)
                    res[name]["cosine_distance_to_f32_embeddings"] = {"items": int(lv.sum()), "max": float("%.3g" % cd.max()), "q99": float("%.3g" % np.quantile(cd, 0.99)),
                                                                      "median": float("%.3g" % np.median(cd)), "above_1e-3": int((cd > 1e-3).sum()),
                                                                      "same_nan_rows": bool(np.array_equal(np.isnan(e[:, 0]), ~lv))}
                d2.close()
                extra_lines["fp16"]["calibrated_pack"] = {"what": "the tolerance check of BASELINE configs[4] on the calibrated seeded pack (BatchNorm statistics from one calibration batch: SE gates "
                                                                  "unsaturated as in a trained ECAPA; same conv weights): real embeddings of the planted masks, segmentation + embedding stages only, one warm pass per mode (turns: tests/test_planted.py)", **res}
            except Exception as e:
                extra_lines["fp16"]["calibrated_pack"] = {"error": str(e)[:300]}
        if a.precision == "f32" and a.x3_steps > 0:
            extra_lines["x3"] = secondary_mode(3, a.x3_steps, "conv_w256_x3", "conv_gemm_x3", "k_conv_gemm_w256<3> (v_mfma_f32_32x32x16_f16 on split operands)",
                                               "options ecapa_precision = 3 + seg_precision = 3: f32 tensors in HBM as in the headline run; every ECAPA conv layer and PyanNet's LSTM (input "
                                               "projections of layers 1-3, recurrence) split both MFMA operands into hi + lo fp16 halves (22 bits) and run hi*hi + lo*hi + hi*lo on the "
                                               "fp16 MFMA with f32 accumulation -- f32-grade scores and embeddings (see the cosine distances) from the fp16 matrix pipe; opt-in, not "
                                               "the headline value", 3)

    # ---- what the headline depends on: the same pipeline on the RAW outputs of the random-weight networks -- every item live and full length
    # (14 382 of them at 1 h, K = 1) -- i.e. SURVEY 8(d)'s nominal FLOPs with no dead rows to skip, against the planted hour's live, partly filled items
    raw_line = None
    if world == 1 and not use_dist and planted and a.raw_steps > 0 and a.hours_per_gpu <= 2.0:
        try:
            d.set_option("profile", 0)
            d.set_planted(0, 0, 0, 0)
            d.diarize_dev(d_pcm.data_ptr(), n_total)
            gpu_sync()
            tr = []
            for _ in range(a.raw_steps):
                t1 = time.perf_counter()
                turns_raw = d.diarize_dev(d_pcm.data_ptr(), n_total)
                tr.append((time.perf_counter() - t1) * 1e3)
            st_r = d.stage_ms()
            raw_line = {"value": round(audio_s / (sorted(tr)[len(tr) // 2] / 1e3), 2), "unit": "x real-time", "ms_per_step_median": round(sorted(tr)[len(tr) // 2], 2),
                        "ms_per_step_min_max": [round(min(tr), 2), round(max(tr), 2)], "steps": a.raw_steps, "turns": len(turns_raw),
                        "stage_ms_last_step": {"segmentation": round(st_r[0], 1), "embedding": round(st_r[1], 1), "finalize": round(st_r[2], 1)},
                        "what": "the same call on the raw outputs of the random-weight networks: every embedding item live and full length (no dead rows to skip), nearly all "
                                "of them exact duplicates for the clustering (K = 1): the nominal per-item work of SURVEY 8(d); `value` above is the planted hour"}
        except Exception as e:
            raw_line = {"error": str(e)[:300]}
        finally:
            d.set_planted(d_ps.data_ptr(), d_pe.data_ptr(), lo, hi - lo)
    if rank == 0:
        ach = cg["flops"] / max(cg["ms"], 1e-9) / 1e9      # TFLOP/s
        peak = F32_MFMA_PEAK_TFLOPS if a.precision == "f32" else F16_MFMA_PEAK_TFLOPS
        # HBM traffic of the dominant kernel comes from a separate rocprofv3 --pmc pass (the counters cannot be read from inside
        # the run).  A recording is only quoted when it was made with the very kernel source that is running now.
        traffic, traffic_src, mfma_util, recorded = None, None, None, None
        pmc_path = os.path.join(ROOT, "profiles", "pmc_conv_gemm_bench.json")
        if a.full and world == 1 and a.precision == "f32" and os.path.exists(pmc_path):
            try:
                pj = json.load(open(pmc_path))
                cur = "+".join(git_blob_sha1(os.path.join(PKG, "csrc", f)) for f in ("conv_gemm.hip", "conv_gemm_h.hip", "conv_narrow.hip"))
                if pj.get("conv_gemm_blob") == cur and pj.get("workload", "raw") == a.workload and float(pj.get("hours_per_gpu", 1.0)) == float(a.hours_per_gpu):
                    pk = pj["per_kernel"]["k_conv_gemm_w256<0>"]
                    traffic, traffic_src = pk["fetch_x2_bytes_per_launch"] + pk["write_bytes_per_launch"], pj["source"] + " -- this field: the k_conv_gemm_w256<0> launches alone"
                    mfma_util = {"k_conv_gemm_w256<0>": pj.get("mfma", {}).get("k_conv_gemm_w256<0>"), "all_kernels": pj.get("mfma"),
                                 "traffic_all_mfma_conv_launches_bytes_per_launch": pj["bytes_per_launch"]}
                else:
                    recorded = {"note": "PMC recording is of another kernel source, workload or size: not quoted", "recorded_blob": pj.get("conv_gemm_blob"),
                                "current_blob": cur, "recorded_workload": pj.get("workload", "raw"), "recorded_hours_per_gpu": pj.get("hours_per_gpu", 1.0)}
            except Exception:
                pass
        out = {
            "metric": ("DRY-RUN of the control plane, not a measurement: " if dry else "") + "real-time factor (audio-sec/wall-sec), %g h 16 kHz mono per GPU" % a.hours_per_gpu,
            "value": round(audio_s / (ms_per_step / 1e3), 2),
            "unit": "x real-time",
            "n_gpus": world, "rccl_ranks": d.comm_info()[1], "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "ms_per_step_min_median_max": [round(step_ms[0], 2), round(step_ms[len(step_ms) // 2], 2), round(step_ms[-1], 2)] if step_ms else None,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 tensors; MFMA operands split into hi + lo fp16 halves (x3)" if a.precision == "x3" else a.precision, "data": "dry-run (stand-in for the library, no GPU work)" if dry else "synthetic",
            "config": {"workload": "%g h synthetic 16 kHz mono per GPU (%g h total), full pipeline: PyanNet segmentation + post-seg + STFT/fbank + "
                                   "ECAPA-TDNN + centroid AHC + reconstruction; %s" % (a.hours_per_gpu, audio_s / HOUR,
                                   "planted multi-speaker workload (SURVEY 8d): both networks run at full cost, then their outputs are replaced by the scores / "
                                   "talker embeddings of the 4-talker schedule the audio was synthesised from" if planted else
                                   "raw outputs of the random-weight networks (degenerate: K = 1)"),
                       "audio_seconds": audio_s, "chunks": C, "embedding_items": 3 * C, "live_items": int(round(live_total)),
                       "K": int(round(kst["flops"] / max(kst["launches"], 1))), "turns": len(turns),
                       "turns_crc32": zlib.crc32("\n".join(sdhip.format_turn(t) for t in turns).encode()),
                       "weights": "seeded synthetic (seg 4321, emb 4322): the reference's ONNX blobs are not in the checkout",
                       "entry_point": "sd_diarize_sharded_dev (RCCL communicator inside libsdhip.so, %d rank%s)" % (world, "" if world == 1 else "s") if use_dist else "sd_diarize_dev",
                       "rccl_ranks": d.comm_info()[1],
                       "sharding": None if not use_dist else "contiguous 32-aligned chunk ranges %s, ncclAllGather of scores+embeddings in slots of %d chunks on the library's "
                                   "stream, clustering on rank 0, which infers %.1f %% of the chunks" % (ranges[:8], per, 100.0 * (ranges[0][1] - ranges[0][0]) / max(C, 1)),
                       "stage_ms_last_step_rank0": {"segmentation": round(stages[0], 1), "embedding": round(stages[1], 1), "finalize (count+clustering+reconstruction)": round(stages[2], 1)},
                       "cold_ms": round(cold_ms, 1),
                       "cold_ms_covers": "sd_create (weights -> HBM; fp16 weight forms only when their mode is selected), PCM upload, %sfirst job with cold workspaces (hipMalloc of ~28 GB of workspaces, first launches)" % ("RCCL communicator, " if use_dist else ""),
                       "single_job_ms": single_job_ms,
                       "single_job_note": None if single_job_ms is None else "one recording at a time (barrier after every job): infer + all-gather + finalize in series; `value` is the "
                                          "pipelined rate of back-to-back jobs (rank 0 finalizes job k while the others infer job k+1)"},
            "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(ach / peak, 4), "traffic": traffic, "traffic_source": traffic_src,
                         "kernel": "k_conv_gemm_w256<0> (v_mfma_f32_32x32x2_f32, 256 x 256 tile): every ECAPA layer with Cout >= 256 + PyanNet's LSTM input projections" if a.precision == "f32" else
                                   "k_conv_gemm_w256<3> (v_mfma_f32_32x32x16_f16 on split operands; `achieved` = executed MFMA work = 3 x the algorithmic FLOPs): the wide ECAPA layers" if a.precision == "x3" else
                                   "k_conv_gemm_pp (v_mfma_f32_16x16x32_f16, fp16 activations, LDS-DMA staged, never drained): the wide ECAPA layers",
                         "all_mfma_conv_launches": {"what": "k_conv_gemm_w256 + k_conv_gemm (128 x 128 tile: Res2Net, ASP tdnn%s) %s" %
                                                            ((", PyanNet) + k_conv_narrow (SincNet", "of the step") if a.precision == "f32" else ("", "in fp16")),
                                                    "achieved": round(cg_all["flops"] / max(cg_all["ms"], 1e-9) / 1e9, 2),
                                                    "frac": round(cg_all["flops"] / max(cg_all["ms"], 1e-9) / 1e9 / peak, 4),
                                                    "launches_per_step": cg_all["launches"] // max(a.steps, 1),
                                                    "kernel_ms_per_step": round(cg_all["ms"] / max(a.steps, 1), 2),
                                                    "algorithmic_gflop_per_step": round(cg_all["flops"] / (3.0 if a.precision == "x3" else 1.0) / max(a.steps, 1) / 1e9, 1)},
                         "f32_launches_beside": None if a.precision == "f32" else {"what": "PyanNet layers, f32 MFMA", "kernel_ms_per_step": round(cg_f32["ms"] / max(a.steps, 1), 2),
                                                                                   "TFLOPs": round(cg_f32["flops"] / max(cg_f32["ms"], 1e-9) / 1e9, 1)},
                         "by_caller": None if a.precision != "f32" else {
                             "what": "the same kernel's launches split by caller: the ECAPA layers (Cout >= 256; all of round 2's launches) and, since round 3, PyanNet's LSTM input "
                                     "projections (K = 256, moved here from the 128 x 128 kernel: 103 -> 120 TF for them, and a lower average for this kernel)",
                             "ecapa_layers": {"achieved": round(cg_e["flops"] / max(cg_e["ms"], 1e-9) / 1e9, 2), "frac": round(cg_e["flops"] / max(cg_e["ms"], 1e-9) / 1e9 / peak, 4),
                                              "launches_per_step": cg_e["launches"] // max(a.steps, 1), "kernel_ms_per_step": round(cg_e["ms"] / max(a.steps, 1), 2)},
                             "lstm_input_projections": {"achieved": round(cg_s["flops"] / max(cg_s["ms"], 1e-9) / 1e9, 2), "launches_per_step": cg_s["launches"] // max(a.steps, 1),
                                                        "kernel_ms_per_step": round(cg_s["ms"] / max(a.steps, 1), 2)}},
                         "launches_per_step": cg["launches"] // max(a.steps, 1),
                         "avg_launch_ms": round(cg["ms"] / max(cg["launches"], 1), 4),
                         "kernel_ms_per_step": round(cg["ms"] / max(a.steps, 1), 2),
                         "algorithmic_gflop_per_step": round(cg["flops"] / (3.0 if a.precision == "x3" else 1.0) / max(a.steps, 1) / 1e9, 1),
                         "algorithmic_bytes_per_launch": round(cg["bytes"] / max(cg["launches"], 1)),
                         "mfma_utilisation_pmc": mfma_util, "recorded_pmc": recorded},
            "other_kernels": extra,
        }
        if world == 1 and a.cpu_seconds > 0:
            out["cpu_baseline"] = cpu_baseline(ws, we, a.cpu_seconds, planted)
            try:
                out["cpu_baseline"]["reference_clustering"] = reference_clustering_baseline(d)
            except Exception as e:                      # (the baseline beside the baseline must never cost the line)
                out["cpu_baseline"]["reference_clustering"] = {"error": str(e)[:200]}
            if planted and not use_dist and a.ref_finalize and C <= 7300:
                try:
                    step()                                                                  # the secondary modes ran last: leave the headline job's buffers behind
                    gpu_sync()
                    e32 = d.read_ws("dz_emb", np.float32, C * 3 * 192).reshape(-1, 192)     # the job's embeddings: planted rows, NaN rows by the reference's rule
                    out["cpu_baseline"]["reference_finalize"] = reference_finalize_baseline(d, p_scores, e32, n_total, turns, dev)
                except Exception as e:
                    out["cpu_baseline"]["reference_finalize"] = {"error": str(e)[:200]}
        else:
            out["cpu_baseline"] = None
        out["config"]["rank0_share"] = share_note
        # the headline's dependence on the workload, in the line itself: executed MFMA work of the step against SURVEY 8(d)'s nominal 57.66 GFLOP per chunk
        nominal_gflop = 57.66 * C
        exec_gflop = cg_all["flops"] / (3.0 if a.precision == "x3" else 1.0) / max(a.steps, 1) / 1e9
        out["workload_dependence"] = {"executed_fraction_of_nominal_flops": round(exec_gflop / nominal_gflop, 4), "executed_gflop_per_step": round(exec_gflop, 1),
                                      "nominal_gflop_per_step": round(nominal_gflop, 1), "live_items": int(round(live_total)), "embedding_items": 3 * C,
                                      "value_raw_workload": raw_line,
                                      "what": "`value` is measured on the planted hour: dead items (no active speaker: the reference's NaN rows) and the frames beyond an item's "
                                              "last valid one are not computed (exact: tests/test_gpu_parity.py::test_ecapa_dead_row_skipping_is_invisible), so the step executes this "
                                              "fraction of SURVEY 8(d)'s nominal FLOPs; `value_raw_workload` is the same call with nothing to skip"}
        out.update(extra_lines)
        if world > 1:
            out["multi_gpu_note"] = ("no N > 1 number has been measured by the builder: the container has no GPU and gpurun boxes have one; the RCCL path has run as a "
                                     "world of one and as `virtual_world` on one GPU, the control flow of this script at N = 8 / 8 h against a stand-in on CPUs "
                                     "(tests/test_distributed_cpu.py).  `value` = N x %g h on N GPUs (weak); `strong_scaling_reading.value` (--full) = one hour on N GPUs." % a.hours_per_gpu)
    # ---- the strong-scaling leg runs LAST, behind the complete headline numbers and under a watchdog: it is the one part of an N > 1 run that no box
    # available to the builder could exercise with more than one real rank.  If it raises on a rank or does not finish in time, rank 0 still prints the
    # line (with the reason in place of the reading) and every rank leaves at once instead of waiting in a collective.
    strong = None
    if use_dist and a.strong_steps > 0:
        import threading

        line_lock = threading.Lock()
        printed = [False]

        def bail(reason):
            # The strong reading is an EXTRA of the line: when only it fails (hung collective, exception) the contract's measurement is complete, so rank 0
            # prints the line with the reason in place of the reading and every rank leaves with code 0 -- a launcher that discards the output of a failed
            # rank set must not lose a valid weak-scaling number over it.  The failure is not silent: it is in the line (`strong_scaling_reading.error`)
            # and on stderr of every rank.  (ADVICE r05 asked for a non-zero code here; what it also asked for is done: one print only -- the lock keeps
            # the watchdog thread and the main thread from both printing -- and no exit path that skips the line.)
            with line_lock:
                if rank == 0 and not printed[0]:
                    printed[0] = True
                    out["strong_scaling_reading"] = {"error": reason}
                    print(json.dumps(out), flush=True)
            print("bench.py rank %d: %s" % (rank, reason), file=sys.stderr)
            sys.stdout.flush(); sys.stderr.flush()
            os._exit(0)
        wd = threading.Timer(float(a.strong_timeout), bail, args=("the strong-scaling leg did not finish within %d s; every other number of the line is complete" % a.strong_timeout,))
        wd.daemon = True
        wd.start()
        try:
            strong = strong_leg()
        except Exception as e:             # (the other ranks are inside a collective by now: their watchdogs end them)
            bail("the strong-scaling leg raised on rank %d: %s" % (rank, repr(e)[:300]))
        wd.cancel()
    if rank == 0:
        if use_dist:
            out["strong_scaling_reading"] = strong
        if use_dist and a.strong_steps > 0:
            with line_lock:
                if not printed[0]:
                    printed[0] = True
                    print(json.dumps(out), flush=True)
        else:
            print(json.dumps(out), flush=True)
        os.dup2(2, 1)          # the JSON line stays the last thing on stdout: whatever a library printf()s at teardown goes to stderr
    d.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
