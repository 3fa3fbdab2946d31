#!/usr/bin/env python3
"""What a speaker roster costs a stream's update, in ONE process: sd_stream_turns of the planted hour of bench.py on three streams that
hold the same hour -- one without a roster, one with a roster attached, one on the PARENT revision's library (check it out in a second tree, `make`
there, pass its libsdhip.so) -- with nothing pushed in between, so a call is the finalize of 7 191 chunks and, for the second stream, the roster update
over its 21 573 rows behind it.  One warm-up round, then five rounds in which the three take turns; medians with the min - max of each five.
    python tools/roster_times.py [--out profiles/roster_times.txt] <parent libsdhip.so>"""
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
out_path = os.path.join(ROOT, "profiles", "roster_times.txt")
if args[:1] == ["--out"]:
    out_path, args = args[1], args[2:]
if len(args) != 1:
    sys.exit(__doc__)
parent_path = os.path.abspath(args[0])
REPS = 5
lines = []


def say(text=""):
    lines.append(text)
    print(text, flush=True)


class ParentStream:
    """a stream of another build of the library, bound by hand (that build knows nothing of the new entries)"""

    def __init__(self, path, seg, emb):
        L = self.L = C.CDLL(path)
        vp, i64 = C.c_void_p, C.c_int64
        L.sd_create.restype = vp
        L.sd_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.sd_destroy.argtypes = [vp]
        L.sd_set_planted.argtypes = [vp, vp, vp, i64, i64]
        L.sd_stream_open.argtypes = [vp, C.POINTER(vp)]
        L.sd_stream_push_dev.argtypes = [vp, vp, i64]
        L.sd_stream_turns.argtypes = [vp, C.POINTER(C.POINTER(sdhip.Turn)), C.POINTER(i64)]
        L.sd_stream_close.argtypes = [vp]
        L.sd_stream_close.restype = None
        L.sd_free_turns.argtypes = [C.POINTER(sdhip.Turn)]
        self.h = L.sd_create(seg.encode(), emb.encode(), 0)
        assert self.h, "sd_create failed on " + path
        self.s = vp(None)
        assert L.sd_stream_open(self.h, C.byref(self.s)) == 0

    def set_planted(self, d_sc, d_em, lo, chunks):
        assert self.L.sd_set_planted(self.h, C.c_void_p(d_sc or None), C.c_void_p(d_em or None), lo, chunks) == 0

    def push_dev(self, ptr, n):
        rc = self.L.sd_stream_push_dev(self.s, C.c_void_p(ptr), n)
        assert rc == 0, rc

    def turns(self):
        p, nt = C.POINTER(sdhip.Turn)(), C.c_int64(0)
        rc = self.L.sd_stream_turns(self.s, C.byref(p), C.byref(nt))
        assert rc == 0, rc
        out = [(p[i].start, p[i].end, int(p[i].label)) for i in range(nt.value)]
        self.L.sd_free_turns(p)
        return out

    def close(self):
        self.L.sd_stream_close(self.s)
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
    old = ParentStream(parent_path, seg, emb)
    seconds = 3600.0
    pcm = synth.make_pcm(seconds, seed=1234)
    n, nc = len(pcm), synth.num_chunks(len(pcm))
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(seconds, 1234)), n, 0, nc)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(pcm).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
    torch.cuda.synchronize()
    plain, named, roster = d.stream(), d.stream(), sdhip.Roster()
    named.set_roster(roster)
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    old.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    piece = 16000 * 600                                     # ten minutes at a time
    for lo in range(0, n, piece):
        m = min(piece, n - lo)
        for s in (plain, named, old):
            s.push_dev(d_pcm.data_ptr() + 2 * lo, m)
    runs = (("without a roster", plain.turns), ("with a roster", named.turns), ("parent library", old.turns))
    ts = {name: [] for name, _ in runs}
    turns = {}
    for rep in range(REPS + 1):                             # round 0: warm-up (it also infers the pending chunks)
        order = runs[rep % 3:] + runs[:rep % 3]
        for name, fn in order:
            t, out = timed(fn)
            turns[name] = out
            if rep:
                ts[name].append(t)
    named.turns()                                           # (once more, outside the timing: the map of the last job)
    ids = d.last_roster_ids()
    same = turns["without a roster"] == turns["parent library"] and turns["with a roster"] == sdhip.relabel_turns_map(turns["without a roster"], ids)
    say("sd_stream_turns of the planted hour (%d chunks, %d table rows, %d turns, K = %d), nothing pushed between the calls; ms, median (min - max) of %d" %
        (nc, 3 * nc, len(turns["with a roster"]), len(ids), REPS))
    for name, _ in runs:
        say("    %-18s %s" % (name, stats(ts[name])))
    lo_, hi_ = min(ts["without a roster"]), max(ts["without a roster"])
    med = sorted(ts["with a roster"])[REPS // 2]
    say("    median with a roster inside the range without one: %s" % ("yes" if lo_ <= med <= hi_ else "NO"))
    say("    same turns in all three (the roster's under its map of the raw labels): %s; roster entries %d, updates %d" % ("yes" if same else "NO", roster.info()[0], roster.info()[1]))
    # the update alone, on the host: the same centroids and counts through sd_roster_update with as many row labels as the hour has rows
    cen, cnt = d.last_speakers()
    rows = (np.arange(3 * nc) % len(cen)).astype(np.int32)
    alone = sdhip.Roster()
    prev = alone.update(cen, cnt, rows)[rows]
    us = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        alone.update(cen, cnt, rows, prev)
        us.append((time.perf_counter() - t0) * 1e3)
    say("    sd_roster_update alone (K = %d, P = %d, %d rows and as many previous ids; through ctypes): %s" % (len(cen), alone.info()[0], len(rows), stats(us)))
    alone.close()
    d.set_planted(0, 0, 0, 0)
    for s in (plain, named):
        s.close()
    roster.close()
    old.close()
    d.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


main()
