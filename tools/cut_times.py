#!/usr/bin/env python3
"""Times the cut object (sd_cut_open_dev + sd_cut_turns_many) against the loop of sd_finalize_dev calls it replaces, in ONE process, on the planted hour
of bench.py (synth.py's audio and schedule, seeded weight packs; both networks run once, every side then works on the same device scores and
embeddings).  For T = 8, 32 and 128 thresholds between 0.3 and 1.2:
  (a) open plus one sd_cut_turns_many          this library
  (b) T x (set the threshold, sd_finalize_dev)  the PARENT revision's library (check it out in a second tree, `make` there, pass its libsdhip.so)
  (c) open alone                                this library
  (d) one plain sd_finalize_dev                 this library and the parent's: the untouched path must not have moved
One warm-up round, then five rounds of (a), (b), the pair of (d) in alternating order, (c); medians with the min - max of each five; the turns of (a) and (b) must be the same.
    python tools/cut_times.py [--out profiles/cut_times.txt] [--seconds 3600] <parent libsdhip.so>"""
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
out_path = os.path.join(ROOT, "profiles", "cut_times.txt")
seconds = 3600.0
while args[:1] and args[0] in ("--out", "--seconds"):
    if args[0] == "--out":
        out_path = args[1]
    else:
        seconds = float(args[1])
    args = args[2:]
if len(args) != 1:
    sys.exit(__doc__)
parent_path = os.path.abspath(args[0])
REPS = 5


class Parent:
    """the finalize of another build of the library: the entries it needs, bound by hand (that build knows nothing of the sd_cut_* entries)"""

    def __init__(self, path, seg, emb):
        L = self.L = C.CDLL(path)
        L.sd_create.restype = C.c_void_p
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [C.c_void_p]
        L.sd_finalize_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.POINTER(sdhip.Turn)), C.POINTER(C.c_int64)]
        L.sd_set_option_f64.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path

    def set_threshold(self, t):
        assert self.L.sd_set_option_f64(self.h, b"clustering_threshold", float(t)) == 0

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


def main():
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    old = Parent(parent_path, seg, emb)
    pcm = synth.make_pcm(seconds, seed=1234)
    n, nc = len(pcm), synth.num_chunks(len(pcm))
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(seconds, 1234)), n, 0, nc)
    pe = synth.planted_embeddings(asg)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(pcm).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(pe).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, 192), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    d.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    d.set_planted(0, 0, 0, 0)
    ps, pe_ = d_seg.data_ptr(), d_emb.data_ptr()
    default = sdhip.CLUSTERING_THRESHOLD_DEFAULT

    def side_a(ths):
        with d.cut_open_dev(ps, pe_, nc, n) as cut:
            return cut.turns_many([(t, None, None) for t in ths])

    def side_b(ths):
        out = []
        for t in ths:
            old.set_threshold(t)
            out.append(old.finalize_dev(ps, pe_, nc, n))
        old.set_threshold(default)
        return out

    def side_c():
        d.cut_open_dev(ps, pe_, nc, n).close()

    lines = ["sd_cut_open_dev + sd_cut_turns_many against the loop of sd_finalize_dev calls on the parent revision's library; the planted %.0f s (%d chunks, %d rows);"
             % (seconds, nc, nc * 3), "one process, one context per library; ms, median of %d (min - max)" % REPS, ""]
    for T in (8, 32, 128):
        ths = [0.3 + (1.2 - 0.3) * i / (T - 1) for i in range(T)]
        runs = {"a": [], "b": [], "c": [], "d": [], "d(parent)": []}
        same = True
        for rep in range(REPS + 1):      # round 0 warms every path up (workspaces grow to the case's size)
            ta, a = timed(lambda: side_a(ths))
            tb, b = timed(lambda: side_b(ths))
            if rep % 2:                  # the pair of (d) in alternating order: neither library always runs behind the other
                td, plain = timed(lambda: d.finalize_dev(ps, pe_, nc, n))
                tdp, plain_p = timed(lambda: old.finalize_dev(ps, pe_, nc, n))
            else:
                tdp, plain_p = timed(lambda: old.finalize_dev(ps, pe_, nc, n))
                td, plain = timed(lambda: d.finalize_dev(ps, pe_, nc, n))
            tc, _ = timed(side_c)
            same = same and a == b and plain == plain_p
            if rep > 0:
                for k, v in zip(("a", "b", "c", "d", "d(parent)"), (ta, tb, tc, td, tdp)):
                    runs[k].append(v)
        lines.append("T = %d thresholds 0.3 .. 1.2; same turns on both sides: %s" % (T, same))
        lines.append("    (a) open + one sd_cut_turns_many        %s" % stats(runs["a"]))
        lines.append("    (b) T x sd_finalize_dev, parent library %s" % stats(runs["b"]))
        lines.append("    (c) open alone                          %s" % stats(runs["c"]))
        lines.append("    (d) one sd_finalize_dev, this library   %s" % stats(runs["d"]))
        lines.append("    (d) one sd_finalize_dev, parent library %s" % stats(runs["d(parent)"]))
        lines.append("    (a) below the minimum of (b): %s" % (sorted(runs["a"])[REPS // 2] < min(runs["b"])))
        print("\n".join(lines[-7:]), flush=True)
        assert same, "the cut and the finalize loop disagree"
    d.close()
    old.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
