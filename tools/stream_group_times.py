#!/usr/bin/env python3
"""Times the group calls of the incremental path -- sd_stream_push_many, sd_stream_turns_many -- against the loop of sd_stream_push / sd_stream_turns
calls they replace, in ONE process, for S = 1, 8 and 64 live streams of synthetic audio (synth.py, seeded weight packs; stream i hears the audio
from 8 s * i on) fed in 10 s pieces from the host, so every item is live.  Three arms hold S streams each and take every round one after the other:
"group" (the new calls), "loop" (single calls on this library) and, with the parent revision's libsdhip.so as argument (check out the parent in a
second tree, `make` there), "loop(parent)": the yardstick -- the new code is never compared with itself alone.  Measured, ms, median of five
(min - max):
  push, sealing   the first five rounds from the third on in which a block of 32 chunks becomes sealed in every stream
  push, plain     the first five rounds from the third on in which none does
  turns, 1 min    the updates at pieces 4 .. 8     turns, 10 min    the updates at pieces 58 .. 62  (two more before each run unmeasured: workspaces grow)
with the stage times of the median run (sd_stage_ms: segmentation, embedding, clustering = the per-stream finalizes; the loop's are sums over its
calls) and, for the group call, the share of the sequential finalizes.  The turns of the three arms are compared at every measured update.
    python tools/stream_group_times.py [--out profiles/stream_group_times.txt] [--streams 1,8,64] [parent libsdhip.so]"""
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
import sdhip
import synth
import weightpack as nn

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "stream_group_times.txt")
sizes = (1, 8, 64)
while args[:1] and args[0].startswith("--"):
    if args[0] == "--out":
        out_path = args[1]
    elif args[0] == "--streams":
        sizes = tuple(int(v) for v in args[1].split(","))
    else:
        sys.exit(__doc__)
    args = args[2:]
parent_path = os.path.abspath(args[0]) if args else None
PIECE = 160000
LAST = 62
TURN_MARKS = (("turns, 1 min", range(4, 9)), ("turns, 10 min", range(58, 63)))
TURN_WARM = (2, 3, 56, 57)


class Group:
    """S streams of this library through the group calls"""
    name = "group"

    def __init__(self, d, S):
        self.d, self.s = d, [d.stream() for _ in range(S)]

    def push(self, pieces):
        self.d.stream_push_many(self.s, pieces)
        return np.array(self.d.stage_ms()[:3])

    def turns(self):
        t = self.d.stream_turns_many(self.s)
        return t, np.array(self.d.stage_ms()[:3])

    def close(self):
        for s in self.s:
            s.close()


class Loop(Group):
    """... through one call per stream"""
    name = "loop"

    def push(self, pieces):
        st = np.zeros(3)
        for s, p in zip(self.s, pieces):
            s.push(p)
            st += self.d.stage_ms()[:3]
        return st

    def turns(self):
        out, st = [], np.zeros(3)
        for s in self.s:
            out.append(s.turns())
            st += self.d.stage_ms()[:3]
        return out, st


class OldLoop:
    """the loop on another build of the library: the entries it needs, bound by hand (that build knows nothing of the group calls)"""
    name = "loop(parent)"

    def __init__(self, path, seg, emb, S):
        L = self.L = C.CDLL(path)
        vp, i64 = C.c_void_p, C.c_int64
        L.sd_create.restype = vp
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [vp]
        L.sd_stream_open.argtypes = [vp, C.POINTER(vp)]
        L.sd_stream_push.argtypes = [vp, vp, i64]
        L.sd_stream_turns.argtypes = [vp, C.POINTER(C.POINTER(sdhip.Turn)), C.POINTER(i64)]
        L.sd_stream_close.argtypes = [vp]
        L.sd_stream_close.restype = None
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        L.sd_stage_ms.argtypes = [vp, C.POINTER(C.c_double)]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path
        self.s = []
        for _ in range(S):
            h = vp(None)
            assert L.sd_stream_open(self.h, C.byref(h)) == 0
            self.s.append(h)

    def stage(self):
        a = (C.c_double * 4)()
        self.L.sd_stage_ms(self.h, a)
        return np.array(a[:3])

    def push(self, pieces):
        st = np.zeros(3)
        for s, p in zip(self.s, pieces):
            rc = self.L.sd_stream_push(s, C.c_void_p(p.ctypes.data), len(p))
            assert rc == 0, rc
            st += self.stage()
        return st

    def turns(self):
        out, st = [], np.zeros(3)
        for s in self.s:
            p, nt = C.POINTER(sdhip.Turn)(), C.c_int64(0)
            rc = self.L.sd_stream_turns(s, C.byref(p), C.byref(nt))
            assert rc == 0, rc
            out.append([(p[i].start, p[i].end, int(p[i].label)) for i in range(nt.value)])
            self.L.sd_free_turns(p)
            st += self.stage()
        return out, st

    def close(self):
        for s in self.s:
            self.L.sd_stream_close(s)
        self.L.sd_destroy(self.h)


def timed(f, *a):
    t0 = time.perf_counter()
    r = f(*a)
    return (time.perf_counter() - t0) * 1e3, r


def main():
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    pcm = synth.make_pcm(LAST * 10.0 + 8.0 * 64 + 10.0, seed=1234)
    sealing = [j for j in range(3, LAST + 1) if sdhip.sealed_chunks(j * PIECE) > sdhip.sealed_chunks((j - 1) * PIECE)][:5]
    plain = [j for j in range(3, LAST + 1) if sdhip.sealed_chunks(j * PIECE) == sdhip.sealed_chunks((j - 1) * PIECE)][:5]
    lines = ["sd_stream_push_many / sd_stream_turns_many against the loop of single-stream calls; S live streams fed in 10 s pieces from the host, one process;",
             "ms, median of 5 (min - max); stages of the median run: segmentation + embedding + clustering (the per-stream finalizes)",
             "loop(parent) = the loop on the parent revision's library%s" % ("" if parent_path else ": NOT MEASURED (no library given)"),
             "push, sealing: rounds %s; push, plain: rounds %s" % (sealing, plain), ""]
    for S in sizes:
        arms = ([OldLoop(parent_path, seg, emb, S)] if parent_path else []) + [Loop(d, S), Group(d, S)]
        runs = {(what, a.name): [] for a in arms for what in ("push, sealing", "push, plain", "turns, 1 min", "turns, 10 min")}
        same, compared = True, 0
        for j in range(1, LAST + 1):
            pieces = [pcm[128000 * i + (j - 1) * PIECE:128000 * i + j * PIECE] for i in range(S)]
            what = "push, sealing" if j in sealing else "push, plain" if j in plain else None
            for a in arms:
                ms, st = timed(a.push, pieces)
                if what:
                    runs[(what, a.name)].append((ms, st))
            if j % 10 == 0:
                print("S = %d: %d rounds of %d" % (S, j, LAST), file=sys.stderr, flush=True)
            mark = [w for w, r in TURN_MARKS if j in r]
            if not mark and j not in TURN_WARM:
                continue
            got = []
            for a in arms:
                ms, (t, st) = timed(a.turns)
                got.append(t)
                if mark:
                    runs[(mark[0], a.name)].append((ms, st))
            if mark:
                compared += 1
                same = same and all(g == got[0] for g in got[1:]) and all(len(t) >= 1 for t in got[0])
        lines.append("S = %d streams; the same turns in every arm at the %d measured updates: %s" % (S, compared, same))
        for what in ("push, sealing", "push, plain", "turns, 1 min", "turns, 10 min"):
            for a in arms:
                v = sorted(runs[(what, a.name)], key=lambda x: x[0])
                med = v[len(v) // 2]
                tail = ""
                if a.name == "group" and what.startswith("turns"):
                    tail = "   finalizes = %.0f %% of the call" % (100.0 * med[1][2] / med[0])
                lines.append("    %-14s %-13s %9.2f  (%9.2f - %9.2f)   %8.2f + %8.2f + %8.2f%s" % (what, a.name, med[0], v[0][0], v[-1][0], med[1][0], med[1][1], med[1][2], tail))
        print("\n".join(lines[-(1 + 4 * len(arms)):]), flush=True)
        for a in arms:
            a.close()
    d.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
