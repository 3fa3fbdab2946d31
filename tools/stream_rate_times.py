#!/usr/bin/env python3
"""Times what streams at another sample rate (sd_stream_set_input_rate) cost, in ONE process, one warm-up and five rounds per figure, medians with
min - max, synthetic audio (synth.py) and seeded weight packs:
 (a) unused, the feature costs nothing: a plain stream on this library against the parent revision's libsdhip.so (check out the parent in a second
     tree, `make` there, pass its path) in alternating rounds -- single push of a 10 s piece that seals no block / that seals one, turns() at
     1 min and at 10 min, and for 64 streams the group push (not sealing / sealing) and sd_stream_turns_many at 1 min;
 (b) the price of the resampling: 64 streams fed 10 s pieces at 8 kHz through sd_stream_push_many against the same library fed the same audio
     already resampled (the pieces y[F(n_prev) : F(n)] of sd_resample), per round that seals and per round that does not, and the kernel's own
     time per launch (sd_kernel_stats under option "profile").
ESTIMATE, written before the first run: (a) every median inside the other arm's range -- the plain paths run the same launches; (b) one launch of
64 rows x 160 000 outputs x 137 taps = 2.8 GFLOP on taps that sit in L2: about 0.1 - 0.2 ms of kernel time, under 1 ms per call with the table
upload, against group pushes of tens of ms (not sealing) to seconds (sealing).
    python tools/stream_rate_times.py [--out profiles/stream_rate_times.txt] [parent libsdhip.so]"""
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
out_path = os.path.join(ROOT, "profiles", "stream_rate_times.txt")
if args[:1] == ["--out"]:
    out_path, args = args[1], args[2:]
parent_path = os.path.abspath(args[0]) if args else None
PIECE = 160000
ROUNDS = 6            # the first is the warm-up
S = 64


class Lib:
    """the entries both builds have, bound by hand so that both arms go through the same Python"""

    def __init__(self, path, seg, emb, name):
        self.name = name
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
        L.sd_stream_push_many.argtypes = [vp, vp, vp, i64]
        L.sd_stream_turns_many.argtypes = [vp, i64, vp, vp, vp]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path

    def open(self, n):
        out = []
        for _ in range(n):
            h = C.c_void_p(None)
            assert self.L.sd_stream_open(self.h, C.byref(h)) == 0
            out.append(h)
        return out

    def close(self, streams):
        for s in streams:
            self.L.sd_stream_close(s)

    def push(self, s, p):
        assert self.L.sd_stream_push(s, C.c_void_p(p.ctypes.data), len(p)) == 0

    def turns(self, s):
        p, nt = C.POINTER(sdhip.Turn)(), C.c_int64(0)
        assert self.L.sd_stream_turns(s, C.byref(p), C.byref(nt)) == 0
        out = [(p[i].start, p[i].end, int(p[i].label)) for i in range(nt.value)]
        self.L.sd_free_turns(p)
        return out

    def push_many(self, streams, pieces):
        n = len(streams)
        hs = (C.c_void_p * n)(*[s.value for s in streams])
        ps = (C.c_void_p * n)(*[p.ctypes.data for p in pieces])
        ns = (C.c_int64 * n)(*[len(p) for p in pieces])
        assert self.L.sd_stream_push_many(hs, ps, ns, n) == 0

    def turns_many(self, streams):
        n = len(streams)
        hs = (C.c_void_p * n)(*[s.value for s in streams])
        t, nt, st = (C.POINTER(sdhip.Turn) * n)(), (C.c_int64 * n)(), (C.c_int32 * n)()
        assert self.L.sd_stream_turns_many(hs, n, t, nt, st) == 0
        out = []
        for i in range(n):
            out.append([(t[i][k].start, t[i][k].end, int(t[i][k].label)) for k in range(nt[i])])
            self.L.sd_free_turns(t[i])
        return out


def timed(f, *a):
    t0 = time.perf_counter()
    r = f(*a)
    return (time.perf_counter() - t0) * 1e3, r


def line(what, arm, v):
    v = sorted(v)
    return "    %-28s %-8s %9.2f  (%9.2f - %9.2f)" % (what, arm, v[len(v) // 2], v[0], v[-1]), v


def main():
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    pcm = synth.make_pcm(60 * 10.0 + 8.0 * S + 10.0, seed=1234)
    lines = [__doc__.split("ESTIMATE")[0].rstrip(), "ESTIMATE" + __doc__.split("ESTIMATE")[1].split("    python")[0].rstrip(), "",
             "MEASURED (ms, median of 5 (min - max))", ""]
    arms = [Lib(os.path.join(PKG, "libsdhip.so"), seg, emb, "this")]
    if parent_path:
        arms.insert(0, Lib(parent_path, seg, emb, "parent"))
    # ---- (a) plain streams, this library against the parent's, alternating
    lines.append("(a) plain streams%s" % ("" if parent_path else "; parent: NOT MEASURED (no library given)"))
    whats = ("push, not sealing", "push, sealing", "turns at 1 min", "turns at 10 min", "64: push_many, not sealing", "64: push_many, sealing", "64: turns_many at 1 min")
    runs = {(w, a.name): [] for w in whats for a in arms}
    same = True
    for r in range(ROUNDS):
        got = []
        for a in arms:
            s = a.open(1)
            rec = {}
            for j in range(1, 61):
                ms, _ = timed(a.push, s[0], pcm[(j - 1) * PIECE:j * PIECE])
                if j == 2:
                    rec["push, not sealing"] = ms
                if j == 3:
                    rec["push, sealing"] = ms
                if j in (6, 60):
                    ms, t = timed(a.turns, s[0])
                    rec["turns at 1 min" if j == 6 else "turns at 10 min"] = ms
                    got.append(t)
            a.close(s)
            s = a.open(S)
            for j in range(1, 7):
                ms, _ = timed(a.push_many, s, [pcm[128000 * i + (j - 1) * PIECE:128000 * i + j * PIECE] for i in range(S)])
                if j == 2:
                    rec["64: push_many, not sealing"] = ms
                if j == 3:
                    rec["64: push_many, sealing"] = ms
            ms, t = timed(a.turns_many, s)
            rec["64: turns_many at 1 min"] = ms
            got.append(t)
            a.close(s)
            if r > 0:
                for w in whats:
                    runs[(w, a.name)].append(rec[w])
        n = len(got) // len(arms)
        same = same and all(got[k] == got[k + n] for k in range(n) if len(arms) == 2)
        print("(a) round %d of %d" % (r + 1, ROUNDS), file=sys.stderr, flush=True)
    for w in whats:
        vs = {}
        for a in arms:
            text, vs[a.name] = line(w, a.name, runs[(w, a.name)])
            lines.append(text)
        if len(arms) == 2:
            mp, mt = vs["parent"][2], vs["this"][2]
            inside = vs["parent"][0] <= mt <= vs["parent"][-1] and vs["this"][0] <= mp <= vs["this"][-1]
            lines.append("        each median inside the other's range: %s%s" % (inside, "" if inside else "; this / parent = %.3f" % (mt / mp)))
    if len(arms) == 2:
        lines.append("    the same turns from both libraries at every update: %s" % same)
    # ---- (b) 64 streams at 8 kHz against the same audio already resampled
    d = sdhip.Diarizer(seg, emb, 0)
    n8 = PIECE // 2
    x8 = [np.ascontiguousarray(pcm[128000 * i:128000 * i + 6 * PIECE:2]) for i in range(S)]      # 8 kHz: every other sample
    y16 = [d.resample(x.astype(np.float32) / np.float32(32768.0), 8000) for x in x8]
    F = [sdhip.resample_final_len(j * n8, 8000) for j in range(7)]
    rated, plain, kernel = {"not sealing": [], "sealing": []}, {"not sealing": [], "sealing": []}, []
    d.set_option("profile", 1)
    for r in range(ROUNDS):
        sa, sb = [d.stream() for _ in range(S)], [d.stream() for _ in range(S)]
        for s in sa:
            s.set_input_rate(8000)
        for j in range(1, 7):
            d.reset_stats()
            ma, _ = timed(d.stream_push_many, sa, [x[(j - 1) * n8:j * n8] for x in x8])
            k = d.kernel_stats("resample_jobs")
            assert k["launches"] == 1
            mb, _ = timed(d.stream_push_many_f32, sb, [y[F[j - 1]:F[j]] for y in y16])
            sealing = sdhip.sealed_chunks(F[j]) > sdhip.sealed_chunks(F[j - 1])
            if r > 0 and j >= 2:
                rated["sealing" if sealing else "not sealing"].append(ma)
                plain["sealing" if sealing else "not sealing"].append(mb)
                kernel.append(k["ms"])
        ta, tb = d.stream_turns_many(sa), d.stream_turns_many(sb)
        assert ta == tb and all(a.info() == b.info() for a, b in zip(sa, sb))
        for s in sa + sb:
            s.close()
        print("(b) round %d of %d" % (r + 1, ROUNDS), file=sys.stderr, flush=True)
    d.set_option("profile", 0)
    lines += ["", "(b) 64 streams, 10 s pieces at 8 kHz (80 000 int16 inputs each) through sd_stream_push_many, against sd_stream_push_many_f32 of the same audio",
              "    already resampled (160 000 floats each); option \"profile\" on in both; the turns and sd_stream_info of the two sets are the same"]
    for what in ("not sealing", "sealing"):
        ta, va = line("push_many, " + what, "8 kHz", rated[what])
        tb, vb = line("push_many, " + what, "16 kHz", plain[what])
        lines += [ta, tb, "        difference of the medians: %+.2f ms (%d rounds)" % (va[len(va) // 2] - vb[len(vb) // 2], len(va))]
    lines.append(line("k_resample_jobs, one launch", "kernel", kernel)[0])
    d.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
