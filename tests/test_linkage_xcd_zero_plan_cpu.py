"""CPU tests of the planning behind option "linkage_batch_xcd_zero" (csrc/linkage_batch_plan.h: linkage_tie_plan, linkage_hx_form, linkage_job_xcd_zero,
linkage_xcd_zero_plan, linkage_xcd_zero_bytes), as a stand-alone program under AddressSanitizer / UBSan (tools/linkage_xcd_zero_plan_check.cpp:
nothing that is loaded into Python runs under a sanitizer) against a second implementation written here: which unfinished jobs of an XCD launch stay in the
batch, the first reason that sends any other home, zero launches of at most 8 consecutive jobs of one key, every job in exactly one launch or in none with a
reason, and the byte counts against the formula restated below."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_KEYS = ("on", "zero_phase", "tie_kernel", "onex", "wide", "cu")
JOB_KEYS = ("N", "G", "TH", "helper", "ran", "timeout", "tie", "bits", "untouched")
ON = dict(on=1, zero_phase=1, tie_kernel=1, onex=1, wide=0, cu=256)
IN, KEY_OFF, NOT_RUN, TIMEOUT, NO_TIE, TIE_ABOVE, AFTER_MERGE, PHASE_OFF, NO_ONEX_REPLAY, WIDE = range(10)
ONE = struct.unpack("<Q", struct.pack("<d", 1.0))[0]
MINUS_ZERO = 1 << 63


def ceil_div(a, b):
    return -(-a // b)


def hx_fits(N, workers):
    return 1 <= workers <= 128 and N >= 3 and ceil_div(N, workers) <= 4 * 256


def tie_ref(N, o):
    """-> (replay, hx_onex, workers): what run_linkage's plan says about the heap replay of a job with the square matrix (linkage.hip: linkage_plan)"""
    if o["tie_kernel"] == 0:
        return False, False, 0
    hx_onex = bool(o["onex"]) and o["cu"] >= 256 and hx_fits(N, 31)
    workers = 31 if hx_onex else (127 if N >= 60000 else 63)
    if o["tie_kernel"] > 1:
        workers = o["tie_kernel"]
        hx_onex = hx_onex and workers <= 31
    if workers + 1 > o["cu"]:
        workers = o["cu"] - 1
    return hx_fits(N, workers), hx_onex, workers


def form_ref(N, wide):
    """-> (s16, lc, dyn): k_linkage_hx's dynamic LDS (linkage_hx.hip: linkage_hx_run)"""
    budget = 130 * 1024
    s16 = N <= 65535 and not wide and 4 * N + 8192 <= budget
    kp = 4 * N if s16 else 0
    lc = min((budget - kp) // 8 if kp < budget else 0, 8191, N - 1)
    return s16, lc, (lc * 8 + kp + 15) // 16 * 16


def why_ref(j, o):
    if o["on"] != 1:
        return KEY_OFF
    if not j["ran"]:
        return NOT_RUN
    if j["timeout"]:
        return TIMEOUT
    if not j["tie"]:
        return NO_TIE
    if j["bits"] != 0:
        return TIE_ABOVE
    if not j["untouched"]:
        return AFTER_MERGE
    if o["zero_phase"] == 0:
        return PHASE_OFF
    replay, hx_onex, _ = tie_ref(j["N"], o)
    if not (replay and hx_onex):
        return NO_ONEX_REPLAY
    if not form_ref(j["N"], o["wide"])[0]:
        return WIDE
    return IN


def zero_bytes_ref(N, workers):
    """heap values (8 N), keys and positions (4 N each), the command record of 16 granules and 8 reply granules per worker, the two change lists of
    workers * cap entries (4 and 8 bytes), size and ty (4 N each); every int array padded to an even count"""
    cap = ceil_div(N, workers)
    even = lambda v: v + v % 2
    return 8 * N + 4 * even(N) * 2 + 8 * (16 + 8 * workers) + 4 * even(workers * cap) + 8 * workers * cap + 4 * even(N) * 2


def plan_ref(jobs, o):
    launches = []
    for k, j in enumerate(jobs):
        if why_ref(j, o) != IN:
            continue
        key = (j["G"], j["TH"], j["helper"], tie_ref(j["N"], o)[2])
        if launches and len(launches[-1][1]) < 8 and launches[-1][0] == key:
            launches[-1][1].append(k)
        else:
            launches.append((key, [k]))
    return [l for _, l in launches]


def dup(N, G=32, **kw):
    """a job that stopped at a tie at height 0 in front of its first merge"""
    return dict(dict(N=N, G=G, TH=256, helper=0, ran=1, timeout=0, tie=1, bits=0, untouched=1), **kw)


def cases():
    rng = np.random.default_rng(710)
    out = []
    for k in range(300):
        o = dict(ON)
        if rng.integers(0, 4) == 0:
            k2, vals = [("on", [0]), ("zero_phase", [0]), ("tie_kernel", [0, 2, 8, 31, 32, 63]), ("onex", [0]), ("wide", [1]), ("cu", [255, 304, 16])][int(rng.integers(0, 6))]
            o[k2] = int(rng.choice(vals))
        jobs = []
        for _ in range(int(rng.integers(0, 30))):
            j = dup(int(rng.choice([3, 4, 5, 33, 257, 1500, 4000, 15999, 31232, 31233, 31745, 40000, 2])), G=int(rng.choice([32, 32, 32, 2, 3])))
            r = int(rng.integers(0, 12))
            if r < 6:
                k2, v = [("ran", 0), ("timeout", 1), ("tie", 0), ("bits", ONE), ("bits", MINUS_ZERO), ("untouched", 0)][r]
                j[k2] = v
            if rng.integers(0, 10) == 0:
                j["helper"] = 1
            jobs.append(j)
        out.append((o, jobs))
    spelled = [
        (ON, []),                                                                    # empty set
        (ON, [dup(1500)]),                                                           # 1, 8, 9 and 17 jobs
        (ON, [dup(1500 + i) for i in range(8)]),
        (ON, [dup(1500 + i) for i in range(9)]),
        (ON, [dup(1500 + i) for i in range(17)]),
        (ON, [dup(40, 2), dup(41, 2), dup(42, 3), dup(43, 2), dup(44, 2, helper=1), dup(45, 2, helper=1)]),      # mixed keys: 2 + 1 + 1 + 2
        (ON, [dup(100), dup(101, tie=0, timeout=1), dup(102, bits=ONE), dup(103, untouched=0), dup(104, ran=0), dup(105, tie=0), dup(106)]),      # the zero set closes over the gaps
        (dict(ON, on=0), [dup(1500), dup(1600)]),
        (dict(ON, zero_phase=0), [dup(1500), dup(1600)]),
        (dict(ON, tie_kernel=0), [dup(1500), dup(1600)]),
        (dict(ON, wide=1), [dup(1500), dup(1600)]),
        (dict(ON, onex=0), [dup(1500), dup(1600)]),
        (dict(ON, cu=255), [dup(1500), dup(1600)]),
        (dict(ON, tie_kernel=32), [dup(1500), dup(1600)]),                           # 32 workers: the replay runs on all XCDs, not in the batch
        (dict(ON, tie_kernel=8), [dup(1500), dup(8192), dup(8193)]),                 # 8 workers hold 8 192 rows
        (ON, [dup(2), dup(3), dup(31232), dup(31233), dup(31744), dup(31745)]),      # N >= 3; the 16-bit form ends at 31 232 rows; 31 workers hold 31 744
    ]
    return out, spelled


def parse(line):
    l, info = line.split("|")
    launches = [[int(v) for v in part.split()] for part in l.split(";")] if l.strip() else []
    jobs = [[int(v) for v in j.split()] for j in info.split(",")] if info.strip() else []
    return launches, jobs


def test_zero_plan_under_the_sanitizers_against_a_second_implementation(tmp_path):
    exe = tmp_path / "linkage_xcd_zero_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "linkage_xcd_zero_plan_check.cpp"), "-o", str(exe)])
    rnd, spelled = cases()
    cs = rnd + spelled
    text = "".join("%s | %s\n" % (" ".join(str(o[k]) for k in OPT_KEYS), " , ".join(" ".join(str(j[k]) for k in JOB_KEYS) for j in jobs)) for o, jobs in cs)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    seen, multi = set(), 0
    for (o, jobs), line in zip(cs, lines):
        assert "BAD" not in line and "bad" not in line, line
        launches, info = parse(line)
        assert len(info) == len(jobs)
        flat = [k for l in launches for k in l]
        # every job in exactly one launch, or in none with a reason; launches in plan order
        assert flat == sorted(set(flat)) and flat == [k for k, i in enumerate(info) if i[0] == IN], line
        for j, (why, workers, replay, hx_onex, s16, lc, dyn, cap, nbytes) in zip(jobs, info):
            assert why == why_ref(j, o), (o, j)
            assert (bool(replay), bool(hx_onex), workers) == tie_ref(j["N"], o) or o["tie_kernel"] == 0
            assert (bool(s16), lc, dyn) == form_ref(j["N"], o["wide"])
            if why == IN:
                assert workers <= 31 and cap == ceil_div(j["N"], workers) and cap <= 1024 and nbytes == zero_bytes_ref(j["N"], workers)
                assert dyn <= 130 * 1024 and 4 * j["N"] + 8 * lc <= dyn
            else:
                assert cap == 0 and nbytes == 0
            seen.add(why)
        for l in launches:
            assert 1 <= len(l) <= 8 and len({(jobs[k]["G"], jobs[k]["TH"], jobs[k]["helper"], info[k][1]) for k in l}) == 1
        assert launches == plan_ref(jobs, o), (o, line)
        multi += len(launches) > 1
    assert seen == set(range(10)) and multi > 20
    res = [parse(l) for l in lines[len(rnd):]]
    assert res[0] == ([], [])
    assert [[len(l) for l in r[0]] for r in res[1:5]] == [[1], [8], [8, 1], [8, 8, 1]]
    assert res[5][0] == [[0, 1], [2], [3], [4, 5]]
    assert res[6][0] == [[0, 6]] and [i[0] for i in res[6][1]] == [IN, TIMEOUT, TIE_ABOVE, AFTER_MERGE, NOT_RUN, NO_TIE, IN]
    for r, why in zip(res[7:14], [KEY_OFF, PHASE_OFF, NO_ONEX_REPLAY, WIDE, NO_ONEX_REPLAY, NO_ONEX_REPLAY, NO_ONEX_REPLAY]):
        assert r[0] == [] and [i[0] for i in r[1]] == [why, why]
    assert res[14][0] == [[0, 1]] and [i[0] for i in res[14][1]] == [IN, IN, NO_ONEX_REPLAY] and res[14][1][1][7] == 1024
    assert res[15][0] == [[1, 2]] and [i[0] for i in res[15][1]] == [NO_ONEX_REPLAY, IN, IN, WIDE, WIDE, NO_ONEX_REPLAY]


def test_the_key_is_declared_and_the_planner_is_plain_cpp():
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    assert '"linkage_batch_xcd_zero"' in hdr and "height 0" in hdr
    plan = open(os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "csrc", "linkage_batch_plan.h")).read()
    assert "hip_runtime" not in plan and "__global__" not in plan and "common.h" not in plan
    assert "linkage_xcd_zero_plan" in plan and "linkage_xcd_zero_bytes" in plan and "linkage_tie_plan" in plan
