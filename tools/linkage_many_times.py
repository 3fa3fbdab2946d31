#!/usr/bin/env python3
"""Times the batched small-N linkage (sd_linkage_many; the dendrograms-ahead pass of the group calls, option "linkage_batch") against what it replaces, in
ONE process: this library and the parent revision's libsdhip.so (check out the parent in a second tree, `make` there, pass the path of its library; its
own sdhip.py next to it is loaded as a second module) in alternating rounds, one warm-up and five measured rounds, ms, median (min - max).
  linkage     sd_linkage_many of 64 jobs of N = 100, 400, 1000 unit rows (d = 192, centroid) with 256 and with 1024 threads per job and with the automatic
              choice, against the loop of 64 sd_linkage_ex calls on this library and on the parent's; every Z compared
  many        sd_diarize_many of 64 recordings of 60 s: this library with the pass, without it ("linkage_batch" 0), the parent's
  streams     64 live streams fed through sd_stream_push_many in 60 s pieces: sd_stream_turns_many at 1 min and at 10 min, the same three arms; one stream's own
              sd_stream_turns and sd_stream_turns_many of that one stream, this library against the parent's (unused, the feature must cost nothing);
              at 10 min also under "max_num_embeddings" 1000, which brings every job below the 1500 rows up to which a job is batched
  --hour      the 64 streams under a window of 38 blocks fed on to 1 h: sd_stream_turns_many, the same three arms
Turns are compared in every round.  The estimate written down before the first run stands at the top of the output.
    python tools/linkage_many_times.py [--out profiles/linkage_many_times.txt] [--streams 64] [--hour] <parent libsdhip.so>"""
import importlib.util
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

ESTIMATE = """estimate, written before the first run: the README's 64-stream update at 10 min spends 971 of 1 337 ms in 64 sequential finalizes, 15 ms each, of which
the one-workgroup linkage should be about 10 ms (k_linkage_heap: about 20 ms at 1000 rows).  With the pass the finalize share should fall towards (slowest job +
J x the non-linkage part): about 15 ms for the launch -- 64 workgroups on 64 of 256 CUs, each slowed a little by the others' traffic -- plus 64 x 5 ms, plus
64 x 0.3 ms for forming the rows a second time: about 360 ms of finalizes and an update near 730 ms.  At 1 min (108 ms of finalizes, linkage well under 1 ms
each) a gain of a few tens of ms at most.  sd_linkage_many of 64 jobs against the loop: near 64 x at N = 1000 if the workgroups do not disturb each other, less
where launch overhead dominates (N = 100).  If the streams hold 1500 train rows or more at 10 min they take the single route and nothing changes."""


def load_parent(lib_path):
    spec = importlib.util.spec_from_file_location("sdhip_parent", os.path.join(os.path.dirname(os.path.abspath(lib_path)), "sdhip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.samefile(mod.LIB_PATH, lib_path), (mod.LIB_PATH, lib_path)
    return mod


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def rounds(arms, same, warm=1, n=5):
    """arms: [(name, f)], taken one after the other in every round; same(results of one round) -> bool.  -> {name: sorted ms}, all rounds equal"""
    ms = {name: [] for name, _ in arms}
    ok = True
    for r in range(warm + n):
        got = []
        for name, f in arms:
            t, res = timed(f)
            got.append(res)
            if r >= warm:
                ms[name].append(t)
        ok = ok and same(got)
    return {k: sorted(v) for k, v in ms.items()}, ok


def fmt(v):
    return "%9.2f  (%9.2f - %9.2f)" % (v[len(v) // 2], v[0], v[-1])


def report(lines, title, ms, ok, extra=None):
    lines.append("%s; the same result in every arm and round: %s" % (title, ok))
    for name, v in ms.items():
        lines.append("    %-28s %s%s" % (name, fmt(v), "   " + extra[name] if extra and name in extra else ""))
    print("\n".join(lines[-(1 + len(ms)):]), flush=True)


def main():
    args = sys.argv[1:]
    out_path, S, hour = os.path.join(ROOT, "profiles", "linkage_many_times.txt"), 64, False
    while args[:1] and args[0].startswith("--"):
        if args[0] == "--out":
            out_path, args = args[1], args[2:]
        elif args[0] == "--streams":
            S, args = int(args[1]), args[2:]
        elif args[0] == "--hour":
            hour, args = True, args[1:]
        else:
            sys.exit(__doc__)
    if len(args) != 1:
        sys.exit(__doc__)
    old = load_parent(args[0])
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d, p = sdhip.Diarizer(seg, emb, 0), old.Diarizer(seg, emb, 0)
    lines = ["batched small-N linkage against what it replaces; one process, this library and the parent's in alternating rounds; ms, median of 5 (min - max)", ESTIMATE, ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    # ---- linkage
    rng = np.random.default_rng(64)
    for N in (100, 400, 1000):
        Xs = [rng.standard_normal((N, 192)) for _ in range(64)]
        Xs = [X / np.linalg.norm(X, axis=1, keepdims=True) for X in Xs]

        def many(threads):
            def f():
                d.set_option("linkage_batch_threads", threads)
                try:
                    return [z.tobytes() for z in d.linkage_many(Xs, "centroid")[0]]
                finally:
                    d.set_option("linkage_batch_threads", 0)
            return f
        arms = [("sd_linkage_many, auto", many(0)), ("sd_linkage_many, 256 threads", many(256)), ("sd_linkage_many, 1024 threads", many(1024)),
                ("loop of sd_linkage_ex", lambda: [d.linkage_ex(X, "centroid").tobytes() for X in Xs]),
                ("loop of sd_linkage_ex (parent)", lambda: [p.linkage_ex(X, "centroid").tobytes() for X in Xs])]
        ms, ok = rounds(arms, lambda got: all(g == got[0] for g in got[1:]))
        report(lines, "linkage, 64 jobs of N = %d" % N, ms, ok)
        flush()

    # ---- the group calls: this library with and without the pass, the parent's
    def with_batch(mode, f):
        def g():
            d.set_option("linkage_batch", mode)
            try:
                r = f()
            finally:
                d.set_option("linkage_batch", 0)
            return r, d.stage_ms()[2]
        return g

    def three(title, f_new, f_old):
        fin = {}

        def keep(name, f):
            def g():
                r, c2 = f()
                fin.setdefault(name, []).append(c2)
                return r
            return g
        arms = [("this library, linkage_batch 1", keep("this library, linkage_batch 1", with_batch(1, f_new))),
                ("this library, linkage_batch 0", keep("this library, linkage_batch 0", with_batch(0, f_new))),
                ("parent", keep("parent", lambda: (f_old(), p.stage_ms()[2])))]
        d.reset_stats()
        ms, ok = rounds(arms, lambda got: all(g == got[0] for g in got[1:]) and all(isinstance(t, list) and len(t) >= 1 for t in got[0]))
        launches = d.kernel_stats("linkage_heap_jobs")["launches"], d.kernel_stats("linkage_heap")["launches"], d.kernel_stats("linkage")["launches"]
        extra = {k: "finalizes %8.2f (median)" % sorted(v[1:])[len(v[1:]) // 2] for k, v in fin.items()}
        report(lines, title, ms, ok, extra)
        lines.append("    (this library, all 12 calls: %d k_linkage_heap_jobs launches, %d k_linkage_heap, %d cooperative)" % launches)
        flush()
        return ms

    pcm = synth.make_pcm((3600.0 if hour else 600.0) + 8.0 * S + 10.0, seed=1234)
    recs = [pcm[128000 * i:128000 * i + 960000] for i in range(S)]
    three("many, %d recordings of 60 s" % S, lambda: d.diarize_many(recs), lambda: p.diarize_many(recs))

    sn, so = [d.stream() for _ in range(S)], [p.stream() for _ in range(S)]
    PIECE = 960000

    def push(j):
        pieces = [pcm[128000 * i + (j - 1) * PIECE:128000 * i + j * PIECE] for i in range(S)]
        d.stream_push_many(sn, pieces)
        p.stream_push_many(so, pieces)

    def marks(label):
        ms = three("streams, %d, update at %s" % (S, label), lambda: d.stream_turns_many(sn), lambda: p.stream_turns_many(so))
        one, ok1 = rounds([("this library", lambda: sn[0].turns()), ("parent", lambda: so[0].turns())], lambda got: got[0] == got[1] and len(got[0]) >= 1)
        report(lines, "one stream's own sd_stream_turns at %s" % label, one, ok1)
        grp, ok2 = rounds([("this library", lambda: d.stream_turns_many(sn[:1])), ("parent", lambda: p.stream_turns_many(so[:1]))], lambda got: got[0] == got[1])
        report(lines, "sd_stream_turns_many of one stream at %s" % label, grp, ok2)
        for name, v in (("one stream", one), ("group of one", grp)):
            a, b = v["this library"], v["parent"]
            lines.append("    %s: each median inside the other side's range: %s" % (name, b[0] <= a[2] <= b[-1] and a[0] <= b[2] <= a[-1]))
        flush()
        return ms

    push(1)
    marks("1 min")
    for j in range(2, 11):
        push(j)
    ms10 = marks("10 min")
    for x in (d, p):
        x.set_option("max_num_embeddings", 1000)
    three("streams, %d, update at 10 min under max_num_embeddings 1000" % S, lambda: d.stream_turns_many(sn), lambda: p.stream_turns_many(so))
    for x in (d, p):
        x.set_option("max_num_embeddings", -1)
    a, b = ms10["this library, linkage_batch 1"], ms10["parent"]
    lines.append("acceptance for the default: median with the pass %.2f ms %s the parent's minimum %.2f ms" % (a[2], "below" if a[2] < b[0] else "NOT below", b[0]))
    flush()
    if hour:
        for s in sn + so:
            s.set_window(38)
        for j in range(11, 61):
            push(j)
            if j % 10 == 0:
                print("pushed %d min" % j, file=sys.stderr, flush=True)
        marks("1 h under a window of 38 blocks")
    for s in sn + so:
        s.close()
    d.close()
    p.close()
    flush()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
