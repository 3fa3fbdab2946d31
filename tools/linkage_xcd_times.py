#!/usr/bin/env python3
"""Times the mid-size linkage jobs run one per XCD (option "linkage_batch_xcd"; k_linkage_rg_jobs) against what they replace, in ONE process: this
library and the parent revision's libsdhip.so (check out the parent in a second tree, `make` there, pass the path of its library; its own sdhip.py next to it
is loaded as a second module) in alternating rounds, one warm-up and five measured rounds, ms, median (min - max), results compared in every round.
  linkage     sd_linkage_many with the key at 1 of 8, 16 and 64 jobs of N = 1 500, 2 000, 4 000 and 8 000 unit rows (d = 192, centroid) against the parent's loop
              of sd_linkage_ex; one job alone on both libraries, and with it the per-job slow-down of eight at once.  "linkage_batch_bytes" is raised to 48 GiB
              for these calls so that the 64 squares of a call are one group (8 000 rows: 512 MB each)
  streams     64 live streams fed through sd_stream_push_many in 60 s pieces, sd_stream_turns_many under "linkage_batch" 1 at 10 min -- and, with --hour, under
              a window of 38 blocks at 1 h --: the key at 1, the key at 0, the parent's; one stream's own sd_stream_turns, this library against the parent's
  finalize    sd_finalize_dev of the planted hour of bench.py, this library against the parent's (unused, the feature must cost nothing: each median inside
              the other arm's min - max; the shared body of k_linkage_rg is on this path)
  --zero      the further arm of option "linkage_batch_xcd_zero" (k_linkage_hx_jobs; output to profiles/linkage_xcd_zero_times.txt): in the linkage
              part 5 % of every job's rows are copies of other rows of the job and the arms are the new key at 1, the new key at 0 (every job ties at height 0
              and is redone alone) and the parent's loop; in the streams part the new key at 1 is a fourth arm, and the parent's arm prints what its jobs met
              (linkage_tie_fallbacks, linkage_zero_phase_jobs, linkage_hx_jobs per update: the counters say a tie and whether the zero phase finished the job,
              which it can only after a tie at height 0); in the finalize part sd_linkage_ex of one such job is timed on both libraries too
The estimate written down before the first run stands at the top of the output.
    python tools/linkage_xcd_times.py [--zero] [--out profiles/linkage_xcd_times.txt] [--part linkage|streams|finalize] [--streams 64] [--hour] <parent libsdhip.so>"""
import os
import sys
import tempfile

import numpy as np

from linkage_many_times import ROOT, load_parent, report, rounds      # (it puts the package on sys.path)

import sdhip
import synth
import weightpack as nn

ESTIMATE = """estimate, written before the first run: the 64-stream update at 10 min (986 ms, 982 on the parent) is 64 sequential finalizes of about 15 ms, of which
the cooperative linkage of 1 500 - 2 100 rows is 10 - 12 ms (a merge 5.8 us, profiles/r05_linkage_parts.txt) and the rest -- distances, rows, cut, reconstruction
-- 3 - 5 ms.  With the key the 64 dendrograms take 8 launches of 8; if eight jobs on eight L2s slow each other by 1.3 x, as 64 one-workgroup jobs did, that is
8 x 12 x 1.3 = 125 ms, plus about 20 ms for the distances of all jobs in one launch, 20 ms for forming the rows a second time and 64 x 4 ms for what is left of
each finalize: about 420 ms of finalizes, an update near 435 ms, 2.2 - 2.3 x the parent.  sd_linkage_many of 8 jobs against the loop: 8 / 1.3 = 6 x where the
merges dominate (8 000 rows), less at 1 500 rows where the loop pays 8 distance launches and 8 synchronisations that the call pays once.  If the dispatcher
does not deal every XCD its 32 workgroups, jobs time out (seconds each) and the figures below show it: linkage_xcd_timeouts is printed with every arm."""
ESTIMATE_ZERO = """estimate, written before the first run: every stream job of the 64-stream update at 10 min (986 ms, 982 on the parent: 64 finalizes of 15.3 ms) holds
duplicate rows and ties in front of its first merge; alone such a job takes three cooperative launches (k_linkage_rg to the tie, k_linkage_hx for the merges at
height 0, k_linkage_rg for the rest: 2 k_linkage_rg launches per job in profiles/linkage_xcd_times.txt) of about 10 - 12 ms together, and 3 - 5 ms of distances,
rows, cut and reconstruction.  With both keys the 64 jobs take 8 first launches that end at the tie (about 1 ms each), 8 zero launches (a few hundred merges at
height 0 per job, replayed by one thread per job at a few us each: 2 - 4 ms) and 8 continuation launches, which are the tie-free launch of 8 jobs of 1 500 - 2 000
rows measured before (9 - 12 ms): 8 x (1 + 3 + 12) = 130 ms, plus about 20 ms for the distances of all jobs in one launch, 20 ms for forming the rows a second
time and 64 x 4 ms for what is left of each finalize: an update near 430 ms, 2.2 - 2.3 x the parent -- the estimate of DESIGN 7.9, reached one pull request late.
sd_linkage_many of 8 jobs with 5 % duplicate rows against the parent's loop: the loop pays three launches and three synchronisations per job, the call three
per eight jobs, so somewhat above the 5.2 - 6.4 x of the tie-free case at 1 500 rows and about that at 8 000 rows, where the merges dominate; the new key at 0
redoes every job alone behind a wasted first launch: about 0.9 x.  If the streams tie above 0, or behind a merge, the new key cannot move them and the counters
printed with the parent's arm will show it: linkage_zero_phase_jobs + linkage_hx_jobs below linkage_tie_fallbacks means whole replays.  If the dispatcher does not
deal every XCD its 32 workgroups, jobs time out (seconds each) and the figures below show it: linkage_xcd_timeouts is printed with every arm."""
GIB48 = 48 << 30


def say(lines, text):
    lines.append(text)
    print(text, flush=True)


def inside(a, b):
    """each median inside the other side's min - max"""
    return b[0] <= a[len(a) // 2] <= b[-1] and a[0] <= b[len(b) // 2] <= a[-1]


def with_copies(X, rng):
    """5 % of the rows become copies of other rows"""
    n = len(X)
    dst = rng.choice(n, n // 20, replace=False)
    src = rng.choice(np.setdiff1d(np.arange(n), dst), n // 20)
    X[dst] = X[src]
    return X


def linkage_part(d, p, lines, flush, zero=False):
    rng = np.random.default_rng(64)
    names = ("linkage_rg_jobs", "linkage_xcd_jobs", "linkage_xcd_redone", "linkage_xcd_timeouts")
    if zero:
        names = names[:1] + ("linkage_hx_zero_jobs", "linkage_rg_cont_jobs", "linkage_xcd_jobs", "linkage_xcd_zero_jobs") + names[2:]
    for N in (1500, 2000, 4000, 8000):
        Xs = [rng.standard_normal((N, 192)) for _ in range(64)]
        Xs = [X / np.linalg.norm(X, axis=1, keepdims=True) for X in Xs]
        if zero:
            Xs = [with_copies(X, rng) for X in Xs]
        alone, ok = rounds([("one job alone", lambda: d.linkage_ex(Xs[0], "centroid").tobytes()), ("one job alone (parent)", lambda: p.linkage_ex(Xs[0], "centroid").tobytes())],
                           lambda got: got[0] == got[1])
        report(lines, "linkage, N = %d" % N, alone, ok)
        say(lines, "    each median inside the other side's range: %s" % inside(alone["one job alone"], alone["one job alone (parent)"]))
        for J in (8, 16, 64):
            def many(zkey=0):
                def f():
                    d.set_option("linkage_batch_xcd", 1)
                    d.set_option("linkage_batch_bytes", GIB48)
                    if zero:
                        d.set_option("linkage_batch_xcd_zero", zkey)
                    try:
                        return [z.tobytes() for z in d.linkage_many(Xs[:J], "centroid")[0]]
                    finally:
                        d.set_option("linkage_batch_xcd", 0)
                        d.set_option("linkage_batch_bytes", 2 << 30)
                        if zero:
                            d.set_option("linkage_batch_xcd_zero", 0)
                return f
            first = "sd_linkage_many, keys 1 / 1" if zero else "sd_linkage_many, key 1"
            arms = [(first, many(1))] + ([("sd_linkage_many, keys 1 / 0", many(0))] if zero else [])
            d.reset_stats()
            ms, ok = rounds(arms + [("loop of sd_linkage_ex (parent)", lambda: [p.linkage_ex(X, "centroid").tobytes() for X in Xs[:J]])],
                            lambda got: all(g == got[0] for g in got[1:]))
            report(lines, "linkage, %d jobs of N = %d%s" % (J, N, ", 5 % of the rows copies" if zero else ""), ms, ok)
            a, b = ms[first], ms["loop of sd_linkage_ex (parent)"]
            say(lines, "    ratio to the parent's minimum: %.2f x; all %d calls: %s" % (b[0] / a[len(a) // 2], 6 * len(arms), ", ".join("%s %d" % (k, d.kernel_stats(k)["launches"]) for k in names)))
            if J == 8:
                one = alone["one job alone"]
                say(lines, "    per-job slow-down of eight at once: %.2f x (the call of 8 against one job alone on this library, medians)" % (a[len(a) // 2] / one[len(one) // 2]))
            flush()


def streams_part(d, p, lines, flush, S, hour, zero=False):
    names = ("linkage_rg_jobs", "linkage_xcd_jobs", "linkage_xcd_redone", "linkage_xcd_timeouts", "linkage_rg_launches")
    if zero:
        names = names[:1] + ("linkage_hx_zero_jobs", "linkage_rg_cont_jobs", "linkage_xcd_jobs", "linkage_xcd_zero_jobs") + names[2:]
    pcm = synth.make_pcm((3600.0 if hour else 600.0) + 8.0 * S + 10.0, seed=1234)
    sn, so = [d.stream() for _ in range(S)], [p.stream() for _ in range(S)]
    PIECE = 960000

    def push(j):
        pieces = [pcm[128000 * i + (j - 1) * PIECE:128000 * i + j * PIECE] for i in range(S)]
        d.stream_push_many(sn, pieces)
        p.stream_push_many(so, pieces)

    def update(key, zkey=0):
        def f():
            d.set_option("linkage_batch", 1)
            d.set_option("linkage_batch_xcd", key)
            if zero:
                d.set_option("linkage_batch_xcd_zero", zkey)
            try:
                return d.stream_turns_many(sn)
            finally:
                d.set_option("linkage_batch", 0)
                d.set_option("linkage_batch_xcd", 0)
                if zero:
                    d.set_option("linkage_batch_xcd_zero", 0)
        return f

    def marks(label):
        d.reset_stats()
        p.reset_stats()
        first = "this library, keys 1 / 1" if zero else "this library, key 1"
        arms = ([(first, update(1, 1))] if zero else []) + [("this library, key 1", update(1)), ("this library, key 0", update(0)), ("parent", lambda: p.stream_turns_many(so))]
        ms, ok = rounds(arms, lambda got: all(g == got[0] for g in got[1:]) and all(isinstance(t, list) and len(t) >= 1 for t in got[0]))
        report(lines, "streams, %d, update at %s under linkage_batch 1" % (S, label), ms, ok)
        a, b = ms[first], ms["parent"]
        say(lines, "    ratio to the parent's minimum: %.2f x; this library, all %d calls: %s" % (b[0] / a[len(a) // 2], 6 * (len(arms) - 1), ", ".join("%s %d" % (k, d.kernel_stats(k)["launches"]) for k in names)))
        if zero:
            say(lines, "    acceptance (the median with all three keys below the parent's minimum): %s" % (a[len(a) // 2] < b[0]))
            say(lines, "    what the parent's jobs met, per update (6 updates): %s" % ", ".join(
                "%s %.1f" % (k, p.kernel_stats(k)["launches"] / 6.0) for k in ("linkage_tie_fallbacks", "linkage_zero_phase_jobs", "linkage_hx_jobs", "linkage_rg_launches")))
        one, ok1 = rounds([("this library", lambda: sn[0].turns()), ("parent", lambda: so[0].turns())], lambda got: got[0] == got[1] and len(got[0]) >= 1)
        report(lines, "one stream's own sd_stream_turns at %s" % label, one, ok1)
        say(lines, "    each median inside the other side's range: %s" % inside(one["this library"], one["parent"]))
        flush()

    for j in range(1, 11):
        push(j)
    marks("10 min")
    if hour:
        for s in sn + so:
            s.set_window(38)
        for j in range(11, 61):
            push(j)
        marks("1 h under a window of 38 blocks")
    for s in sn + so:
        s.close()


def finalize_part(d, p, lines, flush, zero=False):
    import torch
    if zero:
        rng = np.random.default_rng(65)
        X = rng.standard_normal((2000, 192))
        X = with_copies(X / np.linalg.norm(X, axis=1, keepdims=True), rng)
        ms, ok = rounds([("this library", lambda: d.linkage_ex(X, "centroid").tobytes()), ("parent", lambda: p.linkage_ex(X, "centroid").tobytes())], lambda got: got[0] == got[1])
        report(lines, "sd_linkage_ex of one job of 2 000 rows, 5 % of them copies, options unset", ms, ok)
        say(lines, "    each median inside the other side's range: %s" % inside(ms["this library"], ms["parent"]))
    seconds = 3600.0
    pcm = synth.make_pcm(seconds, seed=1234)
    n, nc = len(pcm), synth.num_chunks(len(pcm))
    sc, asg = synth.planted_scores(synth.with_duets(synth.schedule(seconds, 1234)), n, 0, nc)
    dev = torch.device("cuda", 0)
    d_pcm, d_sc, d_pe = torch.from_numpy(pcm).to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(synth.planted_embeddings(asg)).to(dev)
    d_seg = torch.zeros((nc, 293, 3), dtype=torch.float32, device=dev)
    d_emb = torch.zeros((nc * 3, 192), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    d.set_planted(d_sc.data_ptr(), d_pe.data_ptr(), 0, nc)
    d.shard_infer_dev(d_pcm.data_ptr(), 0, n, n, 0, nc, d_seg.data_ptr(), d_emb.data_ptr())
    d.set_planted(0, 0, 0, 0)
    ps, pe = d_seg.data_ptr(), d_emb.data_ptr()
    ms, ok = rounds([("this library", lambda: d.finalize_dev(ps, pe, nc, n)), ("parent", lambda: p.finalize_dev(ps, pe, nc, n))], lambda got: got[0] == got[1] and len(got[0]) >= 1)
    report(lines, "sd_finalize_dev of the planted hour (%d chunks), options unset" % nc, ms, ok)
    say(lines, "    each median inside the other side's range: %s" % inside(ms["this library"], ms["parent"]))
    flush()


def main():
    args = sys.argv[1:]
    out_path, S, hour, part, zero = None, 64, False, None, False
    while args[:1] and args[0].startswith("--"):
        if args[0] == "--out":
            out_path, args = args[1], args[2:]
        elif args[0] == "--streams":
            S, args = int(args[1]), args[2:]
        elif args[0] == "--part":
            part, args = args[1], args[2:]
        elif args[0] == "--hour":
            hour, args = True, args[1:]
        elif args[0] == "--zero":
            zero, args = True, args[1:]
        else:
            sys.exit(__doc__)
    if len(args) != 1 or part not in (None, "linkage", "streams", "finalize"):
        sys.exit(__doc__)
    out_path = out_path or os.path.join(ROOT, "profiles", "linkage_xcd_zero_times.txt" if zero else "linkage_xcd_times.txt")
    old = load_parent(args[0])
    tmp = tempfile.mkdtemp()
    seg, emb = tmp + "/s.sdw", tmp + "/e.sdw"
    nn.save_pack(seg, nn.synth_segmentation_weights(4321))
    nn.save_pack(emb, nn.synth_embedding_weights(4322))
    d, p = sdhip.Diarizer(seg, emb, 0), old.Diarizer(seg, emb, 0)
    lines = ["mid-size linkage jobs one per XCD against what they replace; one process, this library and the parent's in alternating rounds; ms, median of 5 (min - max)"]
    if part in (None, "linkage") or zero:
        lines += [ESTIMATE_ZERO if zero else ESTIMATE, ""]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    if part in (None, "linkage"):
        linkage_part(d, p, lines, flush, zero)
    if part in (None, "streams"):
        streams_part(d, p, lines, flush, S, hour, zero)
    if part in (None, "finalize"):
        finalize_part(d, p, lines, flush, zero)
    d.close()
    p.close()
    flush()
    print("wrote", out_path)


if __name__ == "__main__":
    main()
