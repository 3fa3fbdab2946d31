#!/usr/bin/env python3
"""What "max_num_embeddings" and the stream window buy on long and endless audio, in ONE process:
  1 unused feature   sd_finalize_dev at the planted hour of bench.py, this library against the PARENT revision's (check it out in a second tree, `make`
                     there, pass its libsdhip.so), options unset, alternating order
  2 sampling         sd_finalize_dev at the planted hour and at the 8-hour size of tools/finalize_scale.py for max_num_embeddings unset, 8000, 4000, 2000,
                     1000; at the hour also K and the DER (sd_der, collar 0.25 s) against synth.schedule; and the stream's turns() at one hour with and
                     without the option (10 s pieces; the two settings take turns at being the first call after a push, which also infers the pending chunks)
  3 window           one stream fed 10 s pieces for an hour, set_window at 10 minutes (38 blocks) against no window: push + turns() and the device memory
                     in use above what it was when the stream was opened (hipMemGetInfo: the stream's tail and caches and whatever the context's
                     workspaces grew by), at 10 min and at 1 h, and the bytes that come back when the stream is closed; then the same for S streams
                     through sd_stream_push_many / sd_stream_turns_many (real networks: a planted workload means one recording and is refused there, so
                     the clustering of those runs sees the few embeddings the seeded networks give synthetic audio)
One warm-up round, then five rounds; medians with the min - max of each five.
    python tools/long_audio_times.py [--out profiles/long_audio_times.txt] [--hours 8] [--streams 64] [--group-minutes 60] <parent libsdhip.so>"""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import torch
import sdhip
import synth
import weightpack as nn

args = sys.argv[1:]
opt = {"--out": os.path.join(ROOT, "profiles", "long_audio_times.txt"), "--hours": "8", "--streams": "64", "--group-minutes": "60"}
while args[:1] and args[0] in opt:
    opt[args[0]] = args[1]
    args = args[2:]
if len(args) != 1:
    sys.exit(__doc__)
parent_path = os.path.abspath(args[0])
REPS = 5
SETTINGS = (None, 8000, 4000, 2000, 1000)
PIECE = 160000                                   # 10 s
WINDOW_BLOCKS = 38                               # ceil(600 s / 16 s)
lines = []


def say(text=""):
    lines.append(text)
    print(text, flush=True)


class Parent:
    """the finalize of another build of the library, bound by hand (that build knows nothing of the new entries)"""

    def __init__(self, path, seg, emb):
        L = self.L = C.CDLL(path)
        L.sd_create.restype = C.c_void_p
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [C.c_void_p]
        L.sd_finalize_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.POINTER(sdhip.Turn)), C.POINTER(C.c_int64)]
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path

    def finalize_dev(self, d_seg, d_emb, nc, n):
        p, nt = C.POINTER(sdhip.Turn)(), C.c_int64(0)
        rc = self.L.sd_finalize_dev(self.h, C.c_void_p(d_seg), C.c_void_p(d_emb), nc, n, C.byref(p), C.byref(nt))
        assert rc == 0, rc
        out = [(p[i].start, p[i].end, int(p[i].label)) for i in range(nt.value)]
        self.L.sd_free_turns(p)
        return out

    def close(self):
        self.L.sd_destroy(self.h)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    v = sorted(v)
    return "%9.2f  (%9.2f - %9.2f)" % (v[len(v) // 2], v[0], v[-1])


def set_sampling(d, m):
    d.set_clustering(max_num_embeddings=-1 if m is None else m, seed=0)


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def sampling_table(d, title, ps, pe, nc, n, ref):
    say(title)
    for m in SETTINGS:
        set_sampling(d, m)
        ts = []
        for rep in range(REPS + 1):
            t, turns = timed(lambda: d.finalize_dev(ps, pe, nc, n))
            if rep:
                ts.append(t)
        st = d.stage_ms()
        cnt = d.last_speakers()[1]
        extra = ""
        if ref is not None:
            extra = ", DER %.4f" % sdhip.der(ref, turns, collar=0.25)["der"]
        say("    max_num_embeddings %-6s %s   clustering stage %8.2f, rows clustered %6d, K %d%s" % ("unset" if m is None else m, stats(ts), st[2], int(cnt.sum()), len(cnt), extra))
    set_sampling(d, None)


def main():
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    old = Parent(parent_path, seg, emb)
    seconds = 3600.0
    pcm = synth.make_pcm(seconds, seed=1234)
    n, nc = len(pcm), synth.num_chunks(len(pcm))
    sched = synth.with_duets(synth.schedule(seconds, 1234))
    sc, asg = synth.planted_scores(sched, n, 0, nc)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(pcm).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, 192), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    d.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    d.set_planted(0, 0, 0, 0)
    ps, pe = d_seg.data_ptr(), d_emb.data_ptr()
    ref = []
    for s, e, k, ov in sched:                             # the ground truth of the planted recording as turns
        if k >= 0:
            ref.append((s / 16000.0, e / 16000.0, k))
        if ov >= 0:
            ref.append((s / 16000.0, min(n, s + 8000) / 16000.0, ov))
    say("long_audio_times: one process, one context per library; ms, median of %d (min - max) after one warm-up round" % REPS)
    say()

    # ---- 1
    runs = {"this": [], "parent": []}
    same = True
    for rep in range(REPS + 1):
        order = ("this", "parent") if rep % 2 else ("parent", "this")
        got = {}
        for who in order:
            t, got[who] = timed(lambda: (d if who == "this" else old).finalize_dev(ps, pe, nc, n))
            if rep:
                runs[who].append(t)
        same = same and got["this"] == got["parent"]
    say("1 the feature unused: sd_finalize_dev of the planted hour (%d chunks, %d rows), options unset; same turns: %s" % (nc, nc * 3, same))
    say("    this library   %s" % stats(runs["this"]))
    say("    parent library %s" % stats(runs["parent"]))
    med = {k: sorted(v)[REPS // 2] for k, v in runs.items()}
    say("    each median inside the other's min - max: %s" % (min(runs["parent"]) <= med["this"] <= max(runs["parent"]) and min(runs["this"]) <= med["parent"] <= max(runs["this"])))
    say()
    old.close()

    # ---- 2
    sampling_table(d, "2 sampling: sd_finalize_dev of the planted hour; DER against synth.schedule, collar 0.25 s", ps, pe, nc, n, ref)
    hours = float(opt["--hours"])
    n8 = int(hours * 3600 * 16000)
    c8, _ = sdhip.num_chunks(n8)
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    K8 = 6                                                # the arrays of tools/finalize_scale.py
    spk = torch.randint(0, K8, (c8, 3), generator=g)
    active = torch.rand((c8, 3), generator=g) < torch.tensor([0.9, 0.5, 0.05])
    seg8 = torch.rand((c8, 293, 3), generator=g) * 0.3
    on = (torch.rand((c8, 293, 3), generator=g) < 0.7) & active[:, None, :]
    seg8 = torch.where(on, 0.6 + 0.4 * torch.rand((c8, 293, 3), generator=g), seg8).float()
    cen8 = torch.randn((K8, 192), generator=g)
    emb8 = (cen8[spk] + 0.6 * torch.randn((c8, 3, 192), generator=g)).float()
    emb8[~active] = float("nan")
    d_seg8, d_emb8 = seg8.to(dev), emb8.reshape(c8 * 3, 192).to(dev)
    torch.cuda.synchronize()
    sampling_table(d, "  sd_finalize_dev at the %.0f-hour size of tools/finalize_scale.py (%d chunks, %d live rows)" % (hours, c8, int(active.sum())), d_seg8.data_ptr(), d_emb8.data_ptr(), c8, n8, None)
    del d_seg8, d_emb8, seg8, emb8, on
    # the stream's turns() at one hour
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    first = {None: [], 2000: []}
    fin = {None: [], 2000: []}
    with d.stream() as s:
        head = n - 10 * PIECE
        for i in range(0, head, 6 * PIECE):
            s.push(pcm[i:min(head, i + 6 * PIECE)])
        for j in range(10):
            s.push(pcm[head + j * PIECE:head + (j + 1) * PIECE])
            for q, m in enumerate((None, 2000) if j % 2 == 0 else (2000, None)):
                set_sampling(d, m)
                t, _ = timed(s.turns)
                fin[m].append(d.stage_ms()[2])
                if q == 0:
                    first[m].append(t)
        info = s.info()
    set_sampling(d, None)
    say("  stream at one hour (%d / %d chunks sealed), 10 s pieces: turns() as the first call after a push (pending inference + finalize), and its finalize stage alone (ten calls)" % (info[1], info[2]))
    for m in (None, 2000):
        say("    max_num_embeddings %-6s turns() %s   finalize %s" % ("unset" if m is None else m, stats(first[m]), stats(fin[m])))
    say()

    # ---- 3
    say("3 window: 10 s pieces for an hour, set_window(%d) = 10 minutes against no window; update = push + turns(); memory = device bytes in use above the level at open" % WINDOW_BLOCKS)
    marks = {60: "10 min", 360: "1 h"}
    for window in (WINDOW_BLOCKS, -1):
        base = used_bytes()
        s = d.stream()
        s.set_window(window)
        upd = {k: [] for k in marks}
        mem = {}
        for j in range(1, 361):
            near = [k for k in marks if k - 4 <= j <= k]
            t0 = time.perf_counter()
            s.push(pcm[(j - 1) * PIECE:j * PIECE])
            if near:
                s.turns()
                upd[near[0]].append((time.perf_counter() - t0) * 1e3)
            if j in marks:
                mem[j] = used_bytes() - base
        before = used_bytes()
        info, origin = s.info(), s.origin()
        s.close()
        freed = before - used_bytes()
        for k in marks:
            say("    %-9s at %-6s update %s   memory %8.1f MiB" % ("window" if window >= 0 else "no window", marks[k], stats(upd[k]), mem[k] / 2.0 ** 20))
        say("    %-9s at the end: %d chunks held (%d sealed), origin %d s; closing the stream gave back %.1f MiB" % ("window" if window >= 0 else "no window", info[2], info[1], origin // 16000, freed / 2.0 ** 20))
    d.set_planted(0, 0, 0, 0)
    S, minutes = int(opt["--streams"]), int(opt["--group-minutes"])
    pieces = minutes * 6
    gmarks = {k: v for k, v in marks.items() if k <= pieces}
    say("  %d streams through sd_stream_push_many / sd_stream_turns_many, %d minutes of 10 s pieces each, real networks" % (S, minutes))
    for window in (WINDOW_BLOCKS, -1):
        base = used_bytes()
        ss = [d.stream() for _ in range(S)]
        for s in ss:
            s.set_window(window)
        upd = {k: [] for k in gmarks}
        mem = {}
        for j in range(1, pieces + 1):
            near = [k for k in gmarks if k - 4 <= j <= k]
            t0 = time.perf_counter()
            d.stream_push_many(ss, [pcm[(j - 1) * PIECE:j * PIECE]] * S)
            if near:
                d.stream_turns_many(ss)
                upd[near[0]].append((time.perf_counter() - t0) * 1e3)
            if j in gmarks:
                mem[j] = used_bytes() - base
        before = used_bytes()
        for s in ss:
            s.close()
        freed = before - used_bytes()
        for k in gmarks:
            say("    %-9s at %-6s update of all %d %s   memory %8.1f MiB" % ("window" if window >= 0 else "no window", gmarks[k], S, stats(upd[k]), mem[k] / 2.0 ** 20))
        say("    %-9s closing the %d streams gave back %.1f MiB" % ("window" if window >= 0 else "no window", S, freed / 2.0 ** 20))
    d.close()
    os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
    with open(opt["--out"], "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", opt["--out"])


if __name__ == "__main__":
    main()
