#!/usr/bin/env python3
"""Times sd_diarize_many_audio against the flow `speakerDiarizer --many --resample` had before it -- per recording sd_resample (upload, k_resample,
synchronise, download), then sd_diarize_many_f32, which uploads the 16 kHz floats again -- in ONE process, on recordings cut from the synthetic audio of
synth.py (seeded weight packs): 64 x 60 s and 64 x 10 s at 8 kHz as int16 and as mu-law, and 64 x 60 s at 16 kHz int16 against sd_diarize_many.  One
warm-up and five rounds, the arms alternating inside a round; medians with min - max; the turns of every arm compared.  With the parent revision's
library as argument (check out the parent in a second tree, `make` there, pass its libsdhip.so) the old flow, sd_diarize_many_f32 and sd_diarize_many
are also timed on that build in the same rounds: the new code is never compared with itself alone.
The old flow's host work is part of its time, as it was part of the command line's: int16 -> float (wav_read_f32's division), and for mu-law the table
look-up a caller had to do himself, since the parent reads no G.711.
    python tools/many_audio_times.py [--out profiles/many_audio_times.txt] [parent libsdhip.so]"""
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
out_path = os.path.join(ROOT, "profiles", "many_audio_times.txt")
if args[:1] == ["--out"]:
    out_path, args = args[1], args[2:]
parent_path = os.path.abspath(args[0]) if args else None
REPS = 5

ESTIMATE = """Estimate, written before the run: the networks dominate (README: 2 161 ms for 64 x 60 s), so the call's time barely moves.  What goes away is, per
recording, one upload of 4 n bytes, one k_resample launch, one synchronisation, one download of 8 n bytes and a second upload of 8 n bytes: 64 x 60 s at
8 kHz are 31 M input samples, about 0.6 GB over the bus instead of 61 MB (int16) or 31 MB (mu-law) -- some tens of milliseconds at 60 s, and a larger
share of the call at 10 s.  k_many_ingest itself should run near the memory roof: 246 MB written, 31 - 61 MB read, well under a millisecond."""


class Old:
    """another build of the library: the entries the old flow needs, bound by hand (that build knows nothing of sd_diarize_many_audio)"""

    def __init__(self, path, seg, emb):
        L = self.L = C.CDLL(path)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        L.sd_create.restype = vp
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [vp]
        L.sd_resample_len.restype = i64
        L.sd_resample_len.argtypes = [i64, i32, i32]
        L.sd_resample.argtypes = [vp, vp, i64, i32, i32, vp, i64, C.POINTER(i64)]
        for f in (L.sd_diarize_many, L.sd_diarize_many_f32):
            f.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path

    def resample(self, x, sr):
        no = C.c_int64(0)
        out = np.zeros(self.L.sd_resample_len(len(x), sr, 16000), np.float32)
        rc = self.L.sd_resample(self.h, x.ctypes.data, len(x), sr, 16000, out.ctypes.data, len(out), C.byref(no))
        assert rc == 0 and no.value == len(out), rc
        return out

    def _many(self, fn, recs):
        R = len(recs)
        rows = (C.c_void_p * R)(*[p.ctypes.data for p in recs])
        n = (C.c_int64 * R)(*[len(p) for p in recs])
        turns, nt, st = (C.POINTER(sdhip.Turn) * R)(), (C.c_int64 * R)(), (C.c_int32 * R)()
        rc = fn(self.h, rows, n, R, turns, nt, st)
        assert rc == 0, rc
        out = []
        for r in range(R):
            out.append([(turns[r][i].start, turns[r][i].end, int(turns[r][i].label)) for i in range(nt[r])] if st[r] == 0 else int(st[r]))
            self.L.sd_free_turns(turns[r])
        return out

    def diarize_many_f32(self, recs):
        return self._many(self.L.sd_diarize_many_f32, recs)

    def diarize_many(self, recs):
        return self._many(self.L.sd_diarize_many, recs)

    def close(self):
        self.L.sd_destroy(self.h)


def mulaw_table():
    u = ~np.arange(256, dtype=np.int64) & 0xFF
    s = ((((u & 15) << 3) + 132) << ((u >> 4) & 7)) - 132
    return np.where(u & 0x80, -s, s).astype(np.int16)


def mulaw_encode(table, v):
    order = np.argsort(table, kind="stable")
    s = table[order].astype(np.int32)
    i = np.clip(np.searchsorted(s, v), 1, 255)
    return order[np.where(np.abs(s[i - 1] - v) <= np.abs(s[i] - v), i - 1, i)].astype(np.uint8)


def old_flow(lib, recs, sr, table):
    """-> (ms of the call, ms in front of sd_diarize_many_f32, turns)"""
    t0 = time.perf_counter()
    ys = []
    for p in recs:
        x = (table[p] if p.dtype == np.uint8 else p).astype(np.float32) / np.float32(32768.0)
        ys.append(lib.resample(x, sr))
    t1 = time.perf_counter()
    turns = lib.diarize_many_f32(ys)
    return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, turns


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, 0.0, out


def summary(name, v, extra=""):
    ms = sorted(x[0] for x in v)
    front = sorted(x[1] for x in v)
    s = "    %-34s %9.2f  (%9.2f - %9.2f)" % (name, ms[len(ms) // 2], ms[0], ms[-1])
    if front[-1] > 0:
        s += "   in front of sd_diarize_many_f32: %8.2f  (%8.2f - %8.2f)" % (front[len(front) // 2], front[0], front[-1])
    return s + extra


def main():
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d = sdhip.Diarizer(seg, emb, 0)
    old = Old(parent_path, seg, emb) if parent_path else None
    pcm = synth.make_pcm(600.0, seed=1234)
    pcm8 = np.ascontiguousarray(pcm[::2])
    table = mulaw_table()
    mu8 = mulaw_encode(table, pcm8.astype(np.int32))
    lines = ["sd_diarize_many_audio against the flow it replaces (per recording sd_resample, then sd_diarize_many_f32); one process, one context per library;",
             "ms, median of %d (min - max); parent = the same flow on the parent revision's library%s" % (REPS, "" if old else ": NOT MEASURED (no library given)"),
             "", ESTIMATE, ""]
    for name, sec, src in (("64 x 60 s, 8 kHz int16", 60, pcm8), ("64 x 60 s, 8 kHz mu-law", 60, mu8), ("64 x 10 s, 8 kHz int16", 10, pcm8), ("64 x 10 s, 8 kHz mu-law", 10, mu8)):
        n = sec * 8000
        recs = [src[(r * 64000) % (len(src) - n):][:n] for r in range(64)]
        enc = sdhip.ENC_MULAW if src.dtype == np.uint8 else sdhip.ENC_S16
        audio = [sdhip.Audio(p, 8000, enc) for p in recs]
        runs = {"many_audio": [], "old flow": [], "old flow (parent)": []}
        same = True
        for rep in range(REPS + 1):
            got = {}
            if old:
                got["old flow (parent)"] = old_flow(old, recs, 8000, table)
            got["old flow"] = old_flow(d, recs, 8000, table)
            got["many_audio"] = timed(lambda: d.diarize_many_audio(audio))
            same = same and got["old flow"][2] == got["many_audio"][2] and (not old or got["old flow (parent)"][2] == got["old flow"][2])
            if rep > 0:
                for k, v in got.items():
                    runs[k].append(v[:2])
        # the kernel alone, events around the launch (option "profile"): one more call
        d.set_option("profile", 1)
        d.reset_stats()
        d.diarize_many_audio(audio)
        k = d.kernel_stats("many_ingest")
        d.set_option("profile", 0)
        up_new = sum(p.nbytes for p in recs)
        up_old = sum(4 * len(p) + 4 * 2 * len(p) for p in recs)
        lines.append("%s: %d s of audio; same turns in every arm and round: %s" % (name, 64 * sec, same))
        for key in ("old flow (parent)", "old flow", "many_audio"):
            if runs[key]:
                lines.append(summary(key, runs[key]))
        lines.append("    bytes uploaded: many_audio %.1f MB; old flow %.1f MB up (inputs, then the 16 kHz floats again) and %.1f MB down" % (up_new / 1e6, up_old / 1e6, sum(8 * len(p) for p in recs) / 1e6))
        lines.append("    k_many_ingest: %d launch, %.3f ms for %.1f MB read and written = %.0f GB/s" % (k["launches"], k["ms"], k["bytes"] / 1e6, k["bytes"] / 1e6 / max(k["ms"], 1e-9)))
        print("\n".join(lines[-6:]), flush=True)

    # 16 kHz int16: the new entry against sd_diarize_many, and the existing entries against the parent's -- unused, the feature must cost nothing
    n = 60 * 16000
    recs = [pcm[(r * 128000) % (len(pcm) - n):][:n] for r in range(64)]
    f32 = [p.astype(np.float32) / np.float32(32768.0) for p in recs]
    audio = [sdhip.Audio(p, 16000, sdhip.ENC_S16) for p in recs]
    runs = {"many_audio": [], "sd_diarize_many": [], "sd_diarize_many (parent)": [], "sd_diarize_many_f32": [], "sd_diarize_many_f32 (parent)": []}
    same = True
    for rep in range(REPS + 1):
        got = {}
        if old:
            got["sd_diarize_many (parent)"] = timed(lambda: old.diarize_many(recs))
            got["sd_diarize_many_f32 (parent)"] = timed(lambda: old.diarize_many_f32(f32))
        got["sd_diarize_many"] = timed(lambda: d.diarize_many(recs))
        got["sd_diarize_many_f32"] = timed(lambda: d.diarize_many_f32(f32))
        got["many_audio"] = timed(lambda: d.diarize_many_audio(audio))
        ref = got["sd_diarize_many"][2]
        same = same and all(v[2] == ref for v in got.values())
        if rep > 0:
            for k, v in got.items():
                runs[k].append(v[:2])
    lines.append("64 x 60 s, 16 kHz int16: 3840 s of audio; same turns in every arm and round: %s" % same)
    for key in runs:
        if runs[key]:
            lines.append(summary(key, runs[key]))
    print("\n".join(lines[-6:]), flush=True)
    d.close()
    if old:
        old.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
