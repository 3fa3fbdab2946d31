"""CPU tests of the group calls of the incremental path (sd_stream_push_many*, sd_stream_turns_many): the exported names, the refusals that need no
context, and the host planning of csrc/stream_book.h -- ranges to slots, the side of a range, growth before launch -- as a stand-alone program
under AddressSanitizer + UBSan (tools/sanitize/build_stream_group.sh), checked against the statement of the rules below.  Nothing loaded into python
runs under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sd_stream_push_many", "sd_stream_push_many_dev", "sd_stream_push_many_f32", "sd_stream_turns_many")
SD_ERR_ARG = 1
CHUNK, HOP, GAP, SKINNY = 80000, 8000, 9, 13
EDGES = (1, 100, 80001, 123457, 203000, 328000, 328001, 360000, 583999, 584000, 584001, 600000)


def test_the_four_entries_are_exported_and_declared_in_the_drop_in_header():
    L = sdhip.lib()
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    test_hdr = open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in sdhip.EXPORTS and name not in test_hdr
        assert len([l for l in hdr.splitlines() if l.startswith("int %s(" % name) and l.rstrip().endswith("*/")]) == 1, name      # each declaration on one line
    for m in ("stream_push_many", "stream_push_many_f32", "stream_push_many_dev", "stream_turns_many"):
        assert callable(getattr(sdhip.Diarizer, m))


def test_null_arguments_are_refused_without_a_context():
    L = sdhip.lib()
    one = (C.c_void_p * 1)(None)
    n = (C.c_int64 * 1)(0)
    for f in (L.sd_stream_push_many, L.sd_stream_push_many_dev, L.sd_stream_push_many_f32):
        assert f(None, one, n, 1) == SD_ERR_ARG            # no list
        assert f(one, one, n, 1) == SD_ERR_ARG             # a null stream
        assert f(one, one, n, 0) == SD_ERR_ARG and f(one, one, n, -1) == SD_ERR_ARG
    turns, nt, st = (C.c_void_p * 1)(), (C.c_int64 * 1)(7), (C.c_int32 * 1)(7)
    for hs, S in ((None, 1), (one, 1), (one, 0), (one, -1)):
        assert L.sd_stream_turns_many(hs, S, turns, nt, st) == SD_ERR_ARG
    assert list(nt) == [7] and list(st) == [7] and not any(turns)


# ---- the rules, stated again (sd.cpp:1419, 1457; include/sdhip.h)
def chunk_rule(n):
    i = cnt = 0
    if n > CHUNK:
        cnt = (n - CHUNK + HOP - 1) // HOP
        i = cnt * HOP
    last = 0
    if i + 1 < n:
        last = n - i
        cnt += 1
    return cnt, last


def sealed_of(n):
    full = 0 if n <= CHUNK else (n - CHUNK - 1) // HOP + 1      # chunks k with k * 8000 + 80000 < n
    return 32 * (full // 32)


def tile_of(lo, full, cb, pending):
    """full chunks of a range, from lo on, that the single-stream path computes in a batch of more than 13 chunks"""
    cb = max(cb, 1)
    if full <= 0:
        return 0
    if pending and full <= SKINNY:      # segment_pending: the whole path's batch starts at cb * (lo // cb) where cb keeps blocks whole
        whole = lo + full - cb * (lo // cb) if (cb >= 32 and cb % 32 == 0) else full
        if whole > SKINNY:
            return full
    sides = [min(cb, full - k) > SKINNY for k in range(0, full, cb)]      # run_segment: batches of cb from lo on
    assert all(sides[:-1]) or not any(sides)
    return sum(min(cb, full - k) for k, s in zip(range(0, full, cb), sides) if s)


def plan_of(cb, pending, states):
    out, base = [], 0
    for i, (n, sealed) in enumerate(states):
        if pending:
            n_eq = n - sealed * HOP
            chunks, last = chunk_rule(n_eq)
            if n < 2 or chunks <= 0:
                continue
            full = chunks - 1 if 0 < last < CHUNK else chunks
        else:
            chunks = sealed_of(n) - sealed
            if chunks <= 0:
                continue
            n_eq, full, last = (chunks + GAP) * HOP, chunks, CHUNK
        slot = -(-(chunks + GAP) // 32) * 32
        out.append((i, sealed, sealed + chunks, n_eq, full, last, tile_of(sealed, full, cb, pending), base, slot))
        base += slot
    return base, out


def cases():
    rng = np.random.default_rng(912)
    out = []
    for cb in (4096, 32, 64, 7, 13, 14, 20, 33):
        for pending in (0, 1):
            out.append((cb, pending, [(n, sealed_of(n) if pending else 0) for n in EDGES]))
            for _ in range(12):
                states = []
                for _ in range(int(rng.integers(1, 12))):
                    n = int(rng.choice(EDGES)) if rng.integers(0, 3) == 0 else int(rng.integers(0, 3000000))
                    if rng.integers(0, 4) == 0:      # at an edge of the sealing rule
                        n = (32 * int(rng.integers(1, 9)) - 1) * HOP + CHUNK + int(rng.integers(0, 3))
                    top = sealed_of(n)
                    states.append((n, top if pending else 32 * int(rng.integers(0, top // 32 + 1))))
                out.append((cb, pending, states))
    return out


def test_the_one_side_rule_under_address_and_ub_sanitizers(tmp_path):
    """seg_tile_chunks (csrc/many_plan.h), the one statement of the skinny / tile side rule that packs, groups and the single stream's pending batch
    read, against tile_of above, case by case; and the fact that lets a recording of sd_diarize_many be the pending range of a stream with nothing
    sealed: at lo = 0 the pending exception never fires"""
    exe = str(tmp_path / "stream_group_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_stream_group.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    cs = [(lo, full, cb, p) for cb in (1, 7, 13, 14, 20, 32, 33, 64, 4096) for full in range(81) for lo in (0, 32, 64, 4064, 4096, 8192) for p in (0, 1)]
    path = tmp_path / "tiles.txt"
    path.write_text("".join("%d %d %d %d\n" % c for c in cs))
    out = subprocess.run([exe, "tile", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (out.stdout[-300:], out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    padded = 0
    for line, (lo, full, cb, p) in zip(lines, cs):
        want = tile_of(lo, full, cb, bool(p))
        assert line == str(want), (lo, full, cb, p)
        padded += 0 < want <= SKINNY
        if lo == 0:
            assert tile_of(0, full, cb, True) == tile_of(0, full, cb, False), (full, cb)
    assert padded >= 1      # the batch padded to 14 occurs


def test_group_planning_under_address_and_ub_sanitizers(tmp_path):
    """ranges to slots and the side of a range against the statement above, over random stream states and n at the exact sealing boundaries; growth
    before launch, the appended tails, the scattered rows and the planned compactions on malloc'd memory of exactly the size asked for: two seeds,
    no report, every allocation released, no allocation behind the first kernel of a call"""
    exe = str(tmp_path / "stream_group_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_stream_group.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
    cs = cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join("%d %d %d %s\n" % (cb, p, len(st), " ".join("%d %d" % s for s in st)) for cb, p, st in cs))
    out = subprocess.run([exe, "plan", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (out.stdout[-300:], out.stderr[-2000:])
    lines = out.stdout.splitlines()
    pos = tiles = shorts = 0
    for cb, pending, states in cs:
        total, ranges = plan_of(cb, pending, states)
        assert lines[pos] == "case %d %d" % (total, len(ranges)), (cb, pending, states)
        for k, r in enumerate(ranges):
            assert lines[pos + 1 + k] == "r " + " ".join(str(v) for v in r), (cb, pending, states, k)
            tiles += 0 < r[6] <= SKINNY
            shorts += r[4] < r[2] - r[1]
        pos += 1 + len(ranges)
    assert pos == len(lines) and tiles >= 5 and shorts >= 20      # the padded tile-side range and the short last chunk both occur
    for seed in ("20240911", "7"):
        out = subprocess.run([exe, "run", seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("stream_group ok"), (out.stdout[-300:], out.stderr[-2000:])
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
