"""CPU tests of the host side of sd_linkage_many (csrc/linkage_batch_plan.h): which jobs of a call share a launch and in which groups, as a stand-alone
program under AddressSanitizer / UBSan (tools/linkage_batch_plan_check.cpp: nothing that is loaded into Python runs under a sanitizer) against a naive
second implementation, and the entry's place in the header, the library and the ctypes mirror."""
import os
import re
import subprocess

import numpy as np

import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAP_LDS = 2048


def wgs_ref(N, wgs, onex, cu):
    """the cooperative workgroups run_linkage plans for N rows (linkage.hip: linkage_plan); <= 1 = the one-workgroup heap kernel"""
    if wgs >= 0:
        G = wgs
    elif N < 1500:
        G = 0
    elif onex and cu >= 256 and N < 70000:
        G = 32
    else:
        G = 128 if N >= 90000 else 64 if N >= 8000 else 32
    return min(G, cu)


def bytes_ref(N):
    return 8 * (N * (N - 1) // 2) + 4 * 3 * (N + N % 2) + 8 * N + 32 * (N - 1)


def plan_ref(N, wgs, onex, cu, budget):
    batched = [j for j, n in enumerate(N) if 2 <= n and n - 1 <= HEAP_LDS and wgs_ref(n, wgs, onex, cu) <= 1]
    single = [j for j in range(len(N)) if j not in set(batched)]
    order = sorted(batched, key=lambda j: -N[j])          # stable
    groups, cur, b = [], [], 0
    for j in order:
        if cur and b + bytes_ref(N[j]) > budget:
            groups.append(cur)
            cur, b = [], 0
        cur.append(j)
        b += bytes_ref(N[j])
    if cur:
        groups.append(cur)
    return single, groups


def cases():
    rng = np.random.default_rng(77)
    out = []
    for k in range(300):
        J = int(rng.integers(1, 40))
        N = rng.integers(0, 3001, J)
        if k % 3 == 0:
            N = rng.integers(0, 300, J)
        if k % 7 == 0:
            N[rng.integers(0, J)] = int(rng.choice([1499, 1500, 1501, HEAP_LDS, HEAP_LDS + 1, HEAP_LDS + 2, 2, 1, 0]))
        wgs = int(rng.choice([-1, -1, -1, 0, 1, 2, 32]))
        onex = int(rng.integers(0, 2))
        cu = int(rng.choice([256, 256, 304, 64, 1]))
        budget = int(rng.choice([1, 10 ** 4, 10 ** 6, 2 * 10 ** 7, 2 ** 31]))
        out.append((wgs, onex, cu, budget, [int(v) for v in N]))
    # the route boundary under the automatic geometry and at the end of the LDS heap
    out.append((-1, 1, 256, 2 ** 31, [1498, 1499, 1500, 1501, 7]))
    out.append((0, 1, 256, 2 ** 31, [HEAP_LDS, HEAP_LDS + 1, HEAP_LDS + 2, 3000, 0, 1, 2]))
    out.append((-1, 1, 256, bytes_ref(64) * 2, [64, 64, 64, 64, 64, 63, 65]))
    return out


def test_planner_under_the_sanitizers_against_a_naive_plan(tmp_path):
    exe = tmp_path / "linkage_batch_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "linkage_batch_plan_check.cpp"), "-o", str(exe)])
    cs = cases()
    text = "".join("%d %d %d %d | %s\n" % (w, o, cu, b, " ".join(map(str, N))) for w, o, cu, b, N in cs)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    multi = 0
    for (wgs, onex, cu, budget, N), line in zip(cs, lines):
        s, g, b = line.split("|")
        single = [int(v) for v in s.split()]
        groups = [[int(v) for v in part.split()] for part in g.split("/")] if g.strip() else []
        nbytes = [int(v) for v in b.split()]
        assert nbytes == [bytes_ref(n) if n >= 2 else 0 for n in N]
        # every job in exactly one place
        assert sorted(single + [j for grp in groups for j in grp]) == list(range(len(N))), (N, line)
        for grp in groups:
            assert grp and (len(grp) == 1 or sum(bytes_ref(N[j]) for j in grp) <= budget), (budget, grp)
            assert all(N[a] >= N[b] for a, b in zip(grp, grp[1:]))
            assert all(2 <= N[j] <= HEAP_LDS + 1 and wgs_ref(N[j], wgs, onex, cu) <= 1 for j in grp)
        flat = [j for grp in groups for j in grp]
        assert all(N[a] > N[b] or (N[a] == N[b] and a < b) for a, b in zip(flat, flat[1:]))      # descending over the whole call, equal N in list order
        assert single == sorted(single)
        assert (single, groups) == plan_ref(N, wgs, onex, cu, budget), (wgs, onex, cu, budget, N)
        multi += len(groups) > 1
    assert multi > 20
    # the boundaries, spelled out
    s, g, _ = lines[-3].split("|")
    assert [int(v) for v in s.split()] == [2, 3] and [int(v) for v in g.split()] == [1, 0, 4]      # 1499 is batched, 1500 is not
    s, g, _ = lines[-2].split("|")
    assert [int(v) for v in s.split()] == [2, 3, 4, 5] and [int(v) for v in g.split()] == [1, 0, 6]      # N - 1 = HEAP_LDS is batched, one more is not; 0 and 1 are single
    assert lines[-1].split("|")[1].strip() == "6 / 0 1 / 2 3 / 4 5"


def test_entry_is_declared_exported_and_mirrored():
    L = sdhip.lib()
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    test_hdr = open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    assert hasattr(L, "sd_linkage_many") and "sd_linkage_many" in sdhip.EXPORTS and "sd_linkage_many" not in test_hdr
    m = re.search(r"^int sd_linkage_many\(.*$", hdr, re.M)
    assert m and "cl.cpp:" in m.group(0) and m.group(0).count(");") == 1 and "status" in m.group(0)      # one line, with its citation
    assert callable(sdhip.Diarizer.linkage_many)
    assert '"linkage_batch"' in hdr and '"linkage_batch_bytes"' in hdr
    plan = open(os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "csrc", "linkage_batch_plan.h")).read()
    assert "hip_runtime" not in plan and "__global__" not in plan and "common.h" not in plan          # the planner is plain C++
    assert "LINKAGE_HEAP_LDS = %d" % HEAP_LDS in plan
