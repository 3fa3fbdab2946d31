#!/usr/bin/env python3
"""Times what streams in their own encoding (sd_stream_set_input_format, sd_stream_push_many_audio) cost and give, in ONE process, one warm-up and five
rounds per figure, medians with min - max, synthetic audio (synth.py) and seeded weight packs:
 (a) unused, the feature costs nothing: streams without a format on this library against the parent revision's libsdhip.so (check out the parent in a
     second tree, `make` there, pass its path) in alternating rounds -- single push of a 10 s piece that seals no block / that seals one, turns() at
     1 min and at 10 min, and for 64 streams the group push (not sealing / sealing) and sd_stream_turns_many at 1 min; option "profile" is off
     in both arms, so the brackets that now count k_group_append and k_pcm_to_f32 record no events and the comparison is like for like;
 (b) the _audio group push: 64 mono mu-law streams, and 32 stereo mu-law calls (64 legs, each call's array given to both of its legs), fed 10 s pieces
     at 8 kHz through sd_stream_push_many_audio, against the host decoding (a table look-up, for the stereo calls with the de-interleaving) followed by
     sd_stream_push_many_f32 on 64 streams of rate 8 000 of the same library, per round that seals and per round that does not, the same turns in both
     arms; and the kernel's own time per launch (sd_kernel_stats under option "profile").
ESTIMATE, written before the first run: (a) every median inside the other arm's range -- the typed paths run the same launches; (b) k_group_ingest's
traffic is its stores, about 20 MB out for 64 streams x 10 s at 8 kHz (64 x 80 000 floats), with 5 MB of codes in: tens of microseconds.  The gain is
the upload -- 5 MB of mu-law in place of 20 MB of float (10 MB of int16), and for 32 stereo calls 5 MB once in place of 20 MB -- and the host's decode
loop: a few milliseconds of a group push that takes tens of ms when it seals nothing and hundreds when it seals.
    python tools/stream_audio_times.py [--out profiles/stream_audio_times.txt] [parent libsdhip.so]"""
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
out_path = os.path.join(ROOT, "profiles", "stream_audio_times.txt")
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
    lines.append("(a) streams without a format%s" % ("" if parent_path else "; parent: NOT MEASURED (no library given)"))
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
    # ---- (b) 64 legs at 8 kHz in mu-law against the host decode and the f32 group push
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ingest_ref as G
    table = (G.mulaw_table().astype(np.float64) / 32768.0).astype(np.float32)
    order = np.argsort(G.mulaw_table(), kind="stable")
    levels = G.mulaw_table()[order]

    def encode(v):
        i = np.clip(np.searchsorted(levels, v), 1, 255)
        return order[np.where(np.abs(levels[i - 1] - v) <= np.abs(levels[i] - v), i - 1, i)].astype(np.uint8)

    d = sdhip.Diarizer(seg, emb, 0)
    n8 = PIECE // 2
    legs = [encode(np.ascontiguousarray(pcm[128000 * i:128000 * i + 6 * PIECE:2])) for i in range(S)]      # 8 kHz: every other sample
    calls = [np.stack([legs[2 * q], legs[2 * q + 1]], 1).reshape(-1) for q in range(S // 2)]
    F = [sdhip.resample_final_len(j * n8, 8000) for j in range(7)]
    d.set_option("profile", 1)
    out_b = []
    for case in ("64 mono mu-law streams", "32 stereo mu-law calls (64 legs)"):
        stereo = case.startswith("32")
        new, old, kernel = {"not sealing": [], "sealing": []}, {"not sealing": [], "sealing": []}, []
        for r in range(ROUNDS):
            sa, sb = [d.stream() for _ in range(S)], [d.stream() for _ in range(S)]
            for i, s in enumerate(sa):
                s.set_input_rate(8000)
                s.set_input_format(G.ENC_MULAW, 2 if stereo else 1, i % 2 if stereo else 0)
            for s in sb:
                s.set_input_rate(8000)
            for j in range(1, 7):
                lo, hi = (j - 1) * n8, j * n8
                if stereo:
                    pieces = [calls[i // 2][2 * lo:2 * hi] for i in range(S)]        # the same pointer and frames for both legs of a call
                else:
                    pieces = [legs[i][lo:hi] for i in range(S)]
                d.reset_stats()
                ma, _ = timed(d.stream_push_many_audio, sa, pieces)
                k = d.kernel_stats("group_ingest")
                assert k["launches"] == 1 and d.kernel_stats("resample_jobs")["launches"] == 1

                def host_flow():
                    if stereo:
                        xs = []
                        for q in range(S // 2):
                            both = table[calls[q][2 * lo:2 * hi]].reshape(-1, 2)
                            xs += [np.ascontiguousarray(both[:, 0]), np.ascontiguousarray(both[:, 1])]
                    else:
                        xs = [table[legs[i][lo:hi]] for i in range(S)]
                    d.stream_push_many_f32(sb, xs)
                mb, _ = timed(host_flow)
                sealing = sdhip.sealed_chunks(F[j]) > sdhip.sealed_chunks(F[j - 1])
                if r > 0 and j >= 2:
                    new["sealing" if sealing else "not sealing"].append(ma)
                    old["sealing" if sealing else "not sealing"].append(mb)
                    kernel.append(k["ms"])
            ta, tb = d.stream_turns_many(sa), d.stream_turns_many(sb)
            assert ta == tb and all(a.info() == b.info() for a, b in zip(sa, sb))
            for s in sa + sb:
                s.close()
            print("(b) %s: round %d of %d" % (case, r + 1, ROUNDS), file=sys.stderr, flush=True)
        out_b += ["", "(b) %s, 10 s pieces at 8 kHz (80 000 frames each) through sd_stream_push_many_audio, against the host's table look-up%s and" % (case, " with de-interleaving" if stereo else ""),
                  "    sd_stream_push_many_f32 on 64 streams of rate 8 000; option \"profile\" on in both; the turns and sd_stream_info of the two sets are the same"]
        for what in ("not sealing", "sealing"):
            ta, va = line("push_many, " + what, "_audio", new[what])
            tb, vb = line("push_many, " + what, "host+f32", old[what])
            out_b += [ta, tb, "        difference of the medians: %+.2f ms (%d rounds)" % (va[len(va) // 2] - vb[len(vb) // 2], len(va))]
        out_b.append(line("k_group_ingest, one launch", "kernel", kernel)[0])
    d.set_option("profile", 0)
    d.close()
    lines += out_b
    lines += ["", "NOT MEASURED: the _dev forms, other encodings and channel counts, the single sd_stream_push_audio, more than 64 streams, real speech,",
              "the upload and the kernel apart from the call (beyond the kernel's own time above)" + ("." if parent_path else ", and the parent's library in (a): no path was given.")]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
