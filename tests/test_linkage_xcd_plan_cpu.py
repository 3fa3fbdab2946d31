"""CPU tests of the planner of the jobs sd_linkage_many runs one per XCD (csrc/linkage_batch_plan.h: linkage_geometry, linkage_job_xcd, linkage_xcd_plan;
option "linkage_batch_xcd"), as a stand-alone program under AddressSanitizer / UBSan (tools/linkage_xcd_plan_check.cpp: nothing that is loaded into Python runs
under a sanitizer) against a naive second implementation: the class boundaries, descending-stable order, launches of at most 8, groups within the budget,
every job in exactly one place."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAP_LDS = 2048
KEYS = ("on", "wgs", "onex", "threads", "square", "kernel", "prefetch", "cu", "method", "force", "budget")
AUTO = dict(on=1, wgs=-1, onex=1, threads=0, square=-1, kernel=-1, prefetch=0, cu=256, method=3, force=0, budget=2 ** 40)


def ceil_div(a, b):
    return -(-a // b)


def geom_ref(N, o):
    """the cooperative geometry run_linkage plans for N rows with the square matrix (linkage.hip: linkage_plan); None = the one-workgroup heap kernel"""
    auto_onex = o["wgs"] < 0 and o["onex"] and o["cu"] >= 256 and 1500 <= N < 70000
    if o["wgs"] >= 0:
        G = o["wgs"]
    elif N < 1500:
        G = 0
    elif auto_onex:
        G = 32
    else:
        G = 128 if N >= 90000 else 64 if N >= 8000 else 32
    G = min(G, o["cu"])
    TH = o["threads"]
    if TH <= 0:
        TH = (512 if N >= 16000 else 256) if auto_onex else (512 if N >= 8000 else 256)
    TH = 1024 if TH >= 1024 else 512 if TH >= 512 else 256 if TH >= 256 else 128
    if G <= 1:
        return None
    square = N * N * 8 <= 170e9 if o["square"] < 0 else o["square"] != 0
    if o["wgs"] < 0 and square and o["kernel"] != 0 and N >= 1500:
        G = min(32 if N < 16000 else 64 if N < 45000 else 128, o["cu"])
    if ceil_div(N, G) > 3400:
        G = ceil_div(N, 3400)
    onex = bool(o["onex"]) and G <= 32 and o["cu"] >= 256
    use_rg = square and o["kernel"] != 0
    fits = lambda t: 2 <= G <= 128 and ceil_div(N, G) <= (8 if t <= 512 else 4) * t and t <= 1024
    if use_rg and o["threads"] <= 0:
        TH = 256
    if use_rg and not fits(TH):
        t2 = TH
        while t2 < 1024 and not fits(t2):
            t2 *= 2
        if fits(t2) and (o["threads"] <= 0 or o["kernel"] > 0):
            TH = t2
        else:
            use_rg = False
    return dict(G=G, TH=TH, cap=ceil_div(N, G) + 1, use_rg=use_rg, onex=onex)


def xcd_bytes_ref(N, G):
    return 8 * N * N + 4 * 2 * (N + N % 2) + 2 * 8 * N + 32 * (N - 1) + 2 * G * 40 * 8 + 32 * 4


def job_ref(N, o):
    """-> (G, TH, helper) of a job of the class, else None"""
    if not o["on"] or o["force"] or not 0 <= o["method"] <= 6 or N < 2:
        return None
    g = geom_ref(N, o)
    if g is None or g["G"] < 2 or not g["use_rg"] or not g["onex"]:
        return None
    helper = 1 if o["prefetch"] and g["TH"] <= 448 and g["G"] <= 64 else 0
    if g["cap"] - 1 > 4 * g["TH"] or g["TH"] + 64 * helper > 256 or xcd_bytes_ref(N, g["G"]) > o["budget"]:
        return None
    return g["G"], g["TH"], helper


def heap_batched_ref(N, o):
    g = min(o["wgs"], o["cu"]) if o["wgs"] >= 0 else (0 if N < 1500 else 2)
    return 2 <= N <= HEAP_LDS + 1 and g <= 1


def plan_ref(N, o):
    cand = [j for j, n in enumerate(N) if not heap_batched_ref(n, o)]
    keys = {j: job_ref(N[j], o) for j in cand}
    picked = [j for j in cand if keys[j] is not None and sum(keys[i] == keys[j] for i in cand) >= 2]
    single = [j for j in cand if j not in set(picked)]
    order = sorted(picked, key=lambda j: -N[j])          # stable
    groups, cur, b = [], [], 0
    for j in order:
        bj = xcd_bytes_ref(N[j], keys[j][0])
        if cur and b + bj > o["budget"]:
            groups.append(cur)
            cur, b = [], 0
        cur.append(j)
        b += bj
    if cur:
        groups.append(cur)
    launches = []
    for grp in groups:
        ls = []
        for j in grp:
            if ls and len(ls[-1]) < 8 and keys[ls[-1][-1]] == keys[j]:
                ls[-1].append(j)
            else:
                ls.append([j])
        launches.append(ls)
    return single, launches


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for k in range(400):
        J = int(rng.integers(1, 40))
        N = rng.integers(0, 4000, J)
        if k % 3 == 0:
            N = rng.integers(1400, 17000, J)
        if k % 7 == 0:
            N[rng.integers(0, J)] = int(rng.choice([1499, 1500, 15999, 16000, 2, 1, 0, 1024 * 32, 1024 * 32 + 1]))
        # options under which the class exists, and in two cases of five one option that closes or changes it
        o = dict(on=1, wgs=int(rng.choice([-1, -1, -1, 2, 3, 32])), onex=1, threads=int(rng.choice([0, 0, 128, 256])), square=int(rng.choice([-1, 1])),
                 kernel=int(rng.choice([-1, 1])), prefetch=0, cu=int(rng.choice([256, 304])), method=int(rng.integers(0, 7)), force=0,
                 budget=int(rng.choice([10 ** 7, 10 ** 8, 2 ** 31, 2 ** 40])))
        if rng.integers(0, 5) < 2:
            k2, vals = [("on", [0]), ("wgs", [0, 1, 33]), ("onex", [0]), ("threads", [512, 1024]), ("square", [0]), ("kernel", [0]), ("prefetch", [1]),
                        ("cu", [255, 64]), ("method", [7, -1]), ("force", [1]), ("budget", [10 ** 5, 1])][int(rng.integers(0, 11))]
            o[k2] = int(rng.choice(vals))
        out.append((o, [int(v) for v in N]))
    spelled = [
        (AUTO, [1499, 1500, 15999, 16000, 1500, 7]),                       # the class boundaries under the automatic options
        (dict(AUTO, cu=255), [1500, 2000, 3000]),                          # fewer than 256 CUs: no one-XCD form
        (dict(AUTO, on=0), [1500, 2000, 3000]),                            # the key off
        (AUTO, [1500, 100, 16000]),                                        # fewer than two jobs of the class
        (AUTO, [1500, 2000, 16000, 20000]),                                # mixed G: 32 workgroups on one XCD, 64 on all
        (dict(AUTO, wgs=2, square=1), [2, 3, 5, 2, 9, 3, 1, 0, 5, 4, 6, 7, 8, 2, 3, 4, 5, 6, 7]),      # forced geometry: any N >= 2; 17 jobs = three launches
        (dict(AUTO, budget=3 * xcd_bytes_ref(1600, 32) + 100), [1600] * 7 + [1500] * 4),                  # groups of three
        (dict(AUTO, budget=xcd_bytes_ref(2000, 32)), [2001, 2000, 1999, 1500]),                            # a job over the budget is not of the class
        (dict(AUTO, force=1), [1500, 2000]), (dict(AUTO, method=7), [1500, 2000]), (dict(AUTO, kernel=0), [1500, 2000]), (dict(AUTO, square=0), [1500, 2000]),
        (dict(AUTO, onex=0), [1500, 2000]), (dict(AUTO, prefetch=1), [1500, 2000]),
    ]
    return out, spelled


def parse(line):
    heap, single, g, info = line.split("|")
    groups = [[[int(v) for v in l.split()] for l in grp.split(";")] for grp in g.split("/")] if g.strip() else []
    jobs = [[int(v) for v in j.split()] for j in info.split(",")] if info.strip() else []
    return [int(v) for v in heap.split()], [int(v) for v in single.split()], groups, jobs


def test_planner_under_the_sanitizers_against_a_naive_plan(tmp_path):
    exe = tmp_path / "linkage_xcd_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "linkage_xcd_plan_check.cpp"), "-o", str(exe)])
    rnd, spelled = cases()
    cs = rnd + spelled
    text = "".join("%s | %s\n" % (" ".join(str(o[k]) for k in KEYS), " ".join(map(str, N))) for o, N in cs)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    batched = multi_launch = multi_group = 0
    for (o, N), line in zip(cs, lines):
        assert "BAD" not in line and "bad" not in line, line
        heap, single, groups, jobs = parse(line)
        flat = [j for grp in groups for l in grp for j in l]
        # every job in exactly one place
        assert sorted(heap + single + flat) == list(range(len(N))), (N, line)
        assert single == sorted(single)
        # what the program says about each job alone
        for n, (ok, G, TH, helper, cap, nbytes) in zip(N, jobs):
            ref = job_ref(n, o)
            assert bool(ok) == (ref is not None), (o, n)
            if ref:
                assert (G, TH, helper) == ref and cap == ceil_div(n, G) + 1 and nbytes == xcd_bytes_ref(n, G)
        for grp in groups:
            members = [j for l in grp for j in l]
            assert sum(jobs[j][5] for j in members) <= o["budget"]
            for l in grp:
                assert 1 <= len(l) <= 8 and len({tuple(jobs[j][1:4]) for j in l}) == 1 and all(jobs[j][0] for j in l)
        assert all(N[a] > N[b] or (N[a] == N[b] and a < b) for a, b in zip(flat, flat[1:]))      # descending over the whole call, equal N in list order
        assert not flat or len(flat) >= 2
        assert (single, groups) == plan_ref(N, o), (o, N, line)
        batched += bool(flat)
        multi_launch += any(len(grp) > 1 for grp in groups)
        multi_group += len(groups) > 1
    assert batched > 40 and multi_launch > 10 and multi_group > 10
    # the boundaries, spelled out
    res = [parse(l) for l in lines[len(rnd):]]
    assert res[0][0] == [0, 5] and res[0][1] == [3] and res[0][2] == [[[2, 1, 4]]]       # 1499 goes to the one-workgroup batch, 1500 and 15 999 are of the class, 16 000 is not
    for r, (o, N) in zip(res[1:4], spelled[1:4]):
        assert r[2] == [] and sorted(r[0] + r[1]) == list(range(len(N)))
    assert res[1][1] == [0, 1, 2] and res[2][1] == [0, 1, 2] and res[3][0] == [1] and res[3][1] == [0, 2]
    assert res[4][1] == [2, 3] and res[4][2] == [[[1, 0]]]
    g17 = res[5][2]
    assert res[5][1] == [6, 7] and len(g17) == 1 and [len(l) for l in g17[0]] == [8, 8, 1] and g17[0][0][:3] == [4, 12, 11]      # 9, 8, 7 rows: longest first
    assert [[len(l) for l in grp] for grp in res[6][2]] == [[3], [3], [3], [2]]
    assert res[7][1] == [0] and res[7][2] == [[[1]], [[2]], [[3]]]                         # 2 001 rows exceed the budget alone; the others fit it one at a time
    for r in res[8:]:
        assert r[2] == [] and r[1] == [0, 1]


def test_the_key_is_declared_and_the_planner_is_plain_cpp():
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    assert '"linkage_batch_xcd"' in hdr and "eight to a launch" in hdr
    plan = open(os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "csrc", "linkage_batch_plan.h")).read()
    assert "hip_runtime" not in plan and "__global__" not in plan and "common.h" not in plan
    assert "linkage_xcd_plan" in plan and "linkage_geometry" in plan
