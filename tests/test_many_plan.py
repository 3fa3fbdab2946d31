"""CPU tests of the host side of sd_diarize_many* (csrc/many_plan.h, include/sdhip.h: sd_many_plan): the packed layout against a pure-Python
restatement of its rule, the argument checks that need no GPU, and the planner and the --many list reader as a stand-alone program under
AddressSanitizer / UBSan (tools/many_plan_check.cpp: nothing that is loaded into Python runs under a sanitizer)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, HOP = 80000, 8000
SD_ERR_ARG = 1


def chunks_of(n):
    """slide()'s chunk rule (sd.cpp:1419, 1457), restated"""
    i = cnt = 0
    if n > CHUNK:
        cnt = (n - CHUNK + HOP - 1) // HOP
        i = cnt * HOP
    return cnt + 1 if i + 1 < n else cnt


def plan_ref(lengths):
    """the rule: slot_r = roundup32(chunks_r + 9) chunks (none without a chunk) at the sum of the earlier slots"""
    bases, base = [], 0
    for n in lengths:
        c = chunks_of(n)
        bases.append(base)
        base += 0 if c <= 0 else (c + 9 + 31) // 32 * 32
    return bases, base


EDGES = [0, 1, 2, 100, 250, 251, 7999, 8000, 79999, 80000, 80001, 87999, 88000, 88001, 123457, 203000, 255999, 256000, 256001, 263999, 264000, 264001,
         360000, 511999, 512000, 512001, 960000, 1200000, 57600000, 10 ** 9 + 7]


@functools.lru_cache(maxsize=None)
def length_lists():
    rng = np.random.default_rng(20251)
    lists = [(n,) for n in EDGES] + [tuple(EDGES), tuple(reversed(EDGES))]
    for _ in range(300):
        R = int(rng.integers(1, 40))
        pick = rng.random(R)
        vals = np.where(pick < 0.3, rng.choice(EDGES, R), np.where(pick < 0.8, rng.integers(0, 2000000, R), HOP * rng.integers(0, 300, R) + rng.integers(-1, 2, R)))
        lists.append(tuple(int(max(v, 0)) for v in vals))
    return tuple(lists)


def test_plan_satisfies_the_four_conditions_and_equals_the_restated_rule():
    assert chunks_of(80000) == 1 and chunks_of(80001) == 2 and chunks_of(88000) == 2 and chunks_of(360000) == 36 and chunks_of(1) == 0 and chunks_of(100) == 1
    assert len(length_lists()) > 300
    for lengths in length_lists():
        base, total = sdhip.many_plan(lengths)
        want_base, want_total = plan_ref(lengths)
        assert list(base) == want_base and total == want_total, lengths
        end = 0
        for n, b in zip(lengths, base):
            c = chunks_of(n)
            assert c == sdhip.num_chunks(n)[0]
            slot = 0 if c <= 0 else (c + 9 + 31) // 32 * 32
            assert b % 32 == 0                                                     # aligned batches: 32 chunks = 96 items = 3 embedding batches
            assert b >= end                                                        # slots do not overlap
            if c > 0:
                assert HOP * (b + slot) >= HOP * b + max(n, HOP * (c - 1) + CHUNK)   # zero padding reaches the end of the last chunk's window
            end = b + slot
        assert total == end                                                        # the sum of the slots


def test_host_only_argument_checks_need_no_gpu():
    L = sdhip.lib()
    n = (C.c_int64 * 2)(80000, 90000)
    base = (C.c_int64 * 2)()
    total = C.c_int64(0)
    assert L.sd_many_plan(n, 2, base, C.addressof(total)) == 0 and list(base) == [0, 32] and total.value == 64
    assert L.sd_many_plan(None, 2, base, C.addressof(total)) == SD_ERR_ARG
    assert L.sd_many_plan(n, 2, None, C.addressof(total)) == SD_ERR_ARG
    assert L.sd_many_plan(n, 2, base, None) == SD_ERR_ARG
    assert L.sd_many_plan(n, 0, base, C.addressof(total)) == SD_ERR_ARG
    assert L.sd_many_plan(n, -1, base, C.addressof(total)) == SD_ERR_ARG
    huge = (C.c_int64 * 1)(2 ** 40 + 1)
    assert L.sd_many_plan(huge, 1, base, C.addressof(total)) == SD_ERR_ARG
    # without a context nothing is touched, whatever else is passed
    rows = (C.c_void_p * 1)(None)
    turns, nt, st = (C.c_void_p * 1)(), (C.c_int64 * 1)(7), (C.c_int32 * 1)(7)
    for f in (L.sd_diarize_many, L.sd_diarize_many_dev, L.sd_diarize_many_f32):
        assert f(None, rows, n, 1, turns, nt, st) == SD_ERR_ARG
        assert f(None, None, None, 0, None, None, None) == SD_ERR_ARG
    assert turns[0] is None and nt[0] == 7 and st[0] == 7
    assert L.sd_many_select(None, 0) == SD_ERR_ARG


def test_symbols_are_exported_declared_and_cited():
    L = sdhip.lib()
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    test_hdr = open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    for name in ("sd_many_plan", "sd_diarize_many", "sd_diarize_many_dev", "sd_diarize_many_f32", "sd_many_select"):
        assert hasattr(L, name) and name in sdhip.EXPORTS and name not in test_hdr
        m = re.search(r"^int %s\(.*$" % name, hdr, re.M)
        assert m and "sd.cpp:" in m.group(0), name
    assert "SD_MANY_MAX_CHUNKS 357199" in hdr and 357199 * 3 * 501 <= (2 ** 31 - 1) // 4 < 357200 * 3 * 501
    for name in ("diarize_many", "diarize_many_f32", "diarize_many_dev", "many_select"):
        assert callable(getattr(sdhip.Diarizer, name))


def test_planner_and_list_reader_under_the_sanitizers(tmp_path):
    exe = tmp_path / "many_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "many_plan_check.cpp"), "-o", str(exe)])
    lists = list(length_lists()) + [(2 ** 40 + 1,), (-5, 80000), ()]
    out = subprocess.run([str(exe), "plan"], input="".join(" ".join(map(str, l)) + "\n" for l in lists), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(lists)
    for l, line in zip(lists, lines):
        if not l or max(l) > 2 ** 40:
            assert line == "refused", l
            continue
        bases, total = plan_ref(l)
        assert line == "".join("%d " % b for b in bases) + "| %d" % total, l

    def read(data):
        p = tmp_path / "list.txt"
        p.write_bytes(data)
        r = subprocess.run([str(exe), "list", str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout.splitlines()

    assert read(b"a.wav\nb c.wav\r\n\n# note\n/x/y.wav") == ["ok 3", "a.wav", "b c.wav", "/x/y.wav"]
    assert read(b"a.wav\n")[0] == "ok 1"
    assert read(b"")[0].startswith("error:") and "no path" in read(b"\n\r\n# only a comment\n")[0]
    assert "NUL" in read(b"a.wav\nb\x00.wav\n")[0]
    assert "longer than 4096" in read(b"a.wav\n" + b"x" * 5000 + b"\n")[0]
    assert read(b"x" * 4096 + b"\n") == ["ok 1", "x" * 4096]
    r = subprocess.run([str(exe), "list", str(tmp_path / "absent.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr and r.stdout.startswith("error: cannot open")
