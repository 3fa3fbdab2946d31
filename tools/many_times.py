#!/usr/bin/env python3
"""Times sd_diarize_many_dev against the loop of sd_diarize_dev calls it replaces, in ONE process on ONE context, on recordings cut from the
synthetic audio of synth.py (seeded weight packs): R = 1, 8 and 64 recordings of 60 s, 64 of 10 s, 64 of mixed lengths from 5 to 120 s.
One warm-up pair per case, then five alternating pairs; medians with the min - max of each five, the stage times (sd_stage_ms: segmentation,
embedding, clustering; the loop's are sums over its calls) of the median run, and whether both gave the same turns.  With an older build of the
library as argument (check out the parent revision in a second tree, `make` there, pass its libsdhip.so) the loop is also timed on that build, in
the same rounds: that column is the yardstick -- the new code is never compared with itself alone.
    python tools/many_times.py [--out profiles/many_times.txt] [parent libsdhip.so]"""
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
out_path = os.path.join(ROOT, "profiles", "many_times.txt")
if args[:1] == ["--out"]:
    out_path, args = args[1], args[2:]
parent_path = os.path.abspath(args[0]) if args else None
REPS = 5


class OldLoop:
    """the loop on another build of the library: the five entries it needs, bound by hand (that build knows nothing of the *_many entries)"""

    def __init__(self, path, seg, emb):
        L = self.L = C.CDLL(path)
        L.sd_create.restype = C.c_void_p
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [C.c_void_p]
        L.sd_diarize_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.POINTER(sdhip.Turn)), C.POINTER(C.c_int64)]
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        L.sd_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path

    def diarize_dev(self, ptr, n):
        p, nt = C.POINTER(sdhip.Turn)(), C.c_int64(0)
        rc = self.L.sd_diarize_dev(self.h, C.c_void_p(ptr), n, C.byref(p), C.byref(nt))
        assert rc == 0, rc
        out = [(p[i].start, p[i].end, int(p[i].label)) for i in range(nt.value)]
        self.L.sd_free_turns(p)
        return out

    def stage_ms(self):
        a = (C.c_double * 4)()
        self.L.sd_stage_ms(self.h, a)
        return list(a)

    def close(self):
        self.L.sd_destroy(self.h)


def run_loop(d, ptrs, lens):
    t0 = time.perf_counter()
    turns, st = [], np.zeros(3)
    for p, n in zip(ptrs, lens):
        turns.append(d.diarize_dev(p, n))
        st += d.stage_ms()[:3]
    return (time.perf_counter() - t0) * 1e3, st, turns


def run_many(d, ptrs, lens):
    t0 = time.perf_counter()
    turns = d.diarize_many_dev(ptrs, lens)
    return (time.perf_counter() - t0) * 1e3, np.array(d.stage_ms()[:3]), turns


def main():
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    old = OldLoop(parent_path, seg, emb) if parent_path else None
    pcm = synth.make_pcm(600.0, seed=1234)
    d_pcm = torch.from_numpy(pcm).to("cuda:0")
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    mixed = [int(v) for v in rng.integers(5 * 16000, 120 * 16000 + 1, 64)]
    cases = [("1 x 60 s", [960000]), ("8 x 60 s", [960000] * 8), ("64 x 60 s", [960000] * 64), ("64 x 10 s", [160000] * 64), ("64 x 5 - 120 s", mixed)]
    lines = ["sd_diarize_many_dev against the loop of sd_diarize_dev calls; one process, one context per library; ms, median of %d (min - max)" % REPS,
             "loop(parent) = the loop on the parent revision's library%s" % ("" if old else ": NOT MEASURED (no library given)"), ""]
    for name, lens in cases:
        # recording r starts (r * 8 s) into the 600 s of audio, wrapped so that it fits: device pointers into one buffer, 2 bytes per sample
        offs = [(r * 128000) % (len(pcm) - n) for r, n in enumerate(lens)]
        ptrs = [d_pcm.data_ptr() + 2 * o for o in offs]
        runs = {"loop(parent)": [], "loop": [], "many": []}
        for rep in range(REPS + 1):      # round 0 warms every path up (workspaces grow to the case's size)
            got = {}
            if old:
                got["loop(parent)"] = run_loop(old, ptrs, lens)
            got["loop"] = run_loop(d, ptrs, lens)
            got["many"] = run_many(d, ptrs, lens)
            same = got["loop"][2] == got["many"][2] and (not old or got["loop(parent)"][2] == got["loop"][2])
            if rep > 0:
                for k, v in got.items():
                    runs[k].append(v[:2])
        lines.append("%-15s %6.1f s of audio, %d recordings; same turns everywhere: %s" % (name, sum(lens) / 16000.0, len(lens), same))
        for k in ("loop(parent)", "loop", "many"):
            if not runs[k]:
                continue
            v = sorted(runs[k], key=lambda x: x[0])
            med = v[len(v) // 2]
            lines.append("    %-13s %9.2f  (%9.2f - %9.2f)   stages of the median run: segmentation %8.2f  embedding %8.2f  clustering %8.2f"
                         % (k, med[0], v[0][0], v[-1][0], med[1][0], med[1][1], med[1][2]))
        print("\n".join(lines[-4:]), flush=True)
    d.close()
    if old:
        old.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
