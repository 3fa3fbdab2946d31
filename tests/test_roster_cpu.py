"""CPU tests of the speaker roster (sd_roster_*, sd_relabel_turns_map; the entries that need a stream or a context are in tests/test_roster.py): the library
against tests/roster_ref.py bit for bit on seeded random update sequences that are counted to contain every edge of the rule, known answers for a hand-made
split, merge and return, the refusals that need no stream (a roster of another d and closing an attached roster are refused in tests/test_roster.py, where
there is a stream to attach), the command line's usage errors, the rule on the planted recording with the oracle's labels and the reference's
centroids, and csrc/roster.cpp as a stand-alone program under AddressSanitizer + UBSan (tools/sanitize/build_roster.sh).  Nothing loaded into python
runs under a sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import roster_cases as rcs
import roster_ref
import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
NAMES = ("sd_roster_open", "sd_roster_close", "sd_roster_load", "sd_roster_info", "sd_roster_speakers", "sd_roster_update", "sd_roster_update_last",
         "sd_relabel_turns_map", "sd_stream_set_roster", "sd_last_roster_ids")
SD_ERR_ARG, SD_ERR_NUMERIC = 1, 5
D = 8


def table_bits(t):
    cen, n, seen = t[:3]
    return cen.tobytes(), n.tolist(), seen.tolist()


def lib_table(r):
    return table_bits(r.speakers()) + (r.info()[1],)


def ref_table(r):
    return table_bits(r.table()) + (r.updates,)


def test_exports_and_declarations():
    L = sdhip.lib()
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    test_hdr = open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    for name in NAMES:
        assert name in sdhip.EXPORTS and hasattr(L, name)
        line = re.search(r"^int %s\(.*$" % name, hdr, re.M)
        assert line and re.search(r"\);\s+/\* .*sd\.cpp:\d+-\d+.*\*/$", line.group(0)), name      # one line, with the citation the header's entries carry
        assert name not in test_hdr
    assert "typedef struct sd_roster sd_roster;" in hdr
    for method in ("update", "update_last", "speakers", "info", "load", "close"):
        assert callable(getattr(sdhip.Roster, method))
    assert callable(sdhip.Stream.set_roster) and callable(sdhip.Diarizer.last_roster_ids) and callable(sdhip.relabel_turns_map)
    src = open(os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "csrc", "roster.cpp")).read()
    assert "hip/" not in src and "common.h" not in src                     # the rule is host-only code


def random_sequences():
    """500 seeded sequences of at most 8 updates: K <= 6, P <= 12, M <= 60, d = 8.  Centroids come from a small integer grid (exact ties, exact
    distances) in the even sequences and from noisy copies of a few directions in the odd ones"""
    for seed in range(500):
        rng = np.random.default_rng(seed)
        grid = seed % 2 == 0
        base = rng.standard_normal((8, D))

        def vec():
            if grid:
                v = rng.integers(-2, 3, D).astype(np.float64)
                if not v.any():
                    v[0] = 1.0
                return v
            return base[rng.integers(0, 8)] + 0.25 * rng.standard_normal(D)
        yield seed, rng, vec


def test_random_update_sequences_equal_the_reference_bit_for_bit():
    seen = dict(equal_cnt=0, equal_distance=0, distance_is_t=0, nan_row=0, no_common_row=0, rows_absent=0, prev_absent=0, count_tie=0, loaded=0,
                zero_norm=0, updates=0)
    for seed, rng, vec in random_sequences():
        ref = roster_ref.Roster(D)
        with sdhip.Roster(D) as lib:
            if seed % 5 == 0:                                              # a loaded roster
                P0 = int(rng.integers(1, 5))
                cen, cnt = np.stack([vec() for _ in range(P0)]), rng.integers(0, 20, P0)
                ref.load(cen, cnt)
                lib.load(cen, cnt)
                seen["loaded"] += 1
                assert lib_table(lib) == ref_table(ref), seed
            kept = None
            for step in range(8):
                K, M, P = int(rng.integers(0, 7)), int(rng.integers(0, 61)), ref.P
                if P + K > 12:
                    break
                C_ = np.stack([vec() for _ in range(K)]) if K else np.zeros((0, D))
                m = rng.integers(0, 30, K)
                dup = False
                for k in range(K):
                    how = int(rng.integers(0, 12))
                    if how == 0:
                        C_[k, 0] = np.nan
                        seen["nan_row"] += 1
                    elif how == 1 and P > 0:                                # an entry's own centroid and count: distance 0, and m[k] == n_p
                        p = int(rng.integers(0, P))
                        C_[k], m[k] = ref.cen[p], ref.n[p]
                    elif how == 2 and k > 0:                                # duplicated rows: two columns at exactly equal distance from every entry
                        C_[k] = C_[k - 1]
                        dup = True
                    elif how == 3 and int(rng.integers(0, 8)) == 0:
                        C_[k] = 0.0                                         # a zero norm
                live_p = [p for p in range(P) if not np.isnan(ref.cen[p, 0]) and ref.cen[p].any()]
                live_k = [k for k in range(K) if not np.isnan(C_[k, 0]) and C_[k].any()]
                seen["equal_distance"] += bool(dup and live_p)
                rows = np.where(rng.random(M) < 0.8, rng.integers(0, max(K, 1), M), -1).astype(np.int32) if K else np.full(M, -1, np.int32)
                use_rows, use_prev = rng.random() < 0.8, kept is not None and rng.random() < 0.85
                shift = 0 if rng.random() < 0.6 or kept is None else int(rng.integers(0, len(kept) + 4))
                t = [None, 0.0, 2.0, float(rng.random() * 1.2)][int(rng.integers(0, 4))]
                if live_p and live_k and rng.random() < 0.3:                # a threshold that IS a distance of this update: the pair is taken (inclusive)
                    t = roster_ref.cosine_distance(C_[live_k[int(rng.integers(0, len(live_k)))]], ref.cen[live_p[int(rng.integers(0, len(live_p)))]])
                    if 0.0 <= t <= 2.0:
                        seen["distance_is_t"] += 1
                    else:
                        t = 2.0                                             # (rounding may leave a distance a hair outside [0, 2])
                a_rows, a_prev = rows if use_rows else None, kept if use_prev else None
                seen["rows_absent"] += not use_rows
                seen["prev_absent"] += not use_prev
                if use_rows and use_prev:
                    seen["no_common_row"] += shift >= len(kept)
                    cnt = {}
                    for i in range(min(M, max(0, len(kept) - shift))):
                        if rows[i] >= 0 and kept[i + shift] >= 0:
                            cnt[(int(rows[i]), int(kept[i + shift]))] = cnt.get((int(rows[i]), int(kept[i + shift])), 0) + 1
                    seen["equal_cnt"] += len(set(cnt.values())) < len(cnt)
                before, n_before = ref_table(ref), ref.n.copy()
                try:
                    want = ref.update(C_, m, a_rows, a_prev, shift, roster_ref.T_DEFAULT if t is None else t)
                except roster_ref.ZeroNorm:
                    with pytest.raises(sdhip.SdError) as e:
                        lib.update(C_, m, a_rows, a_prev, shift, t)
                    assert e.value.code == SD_ERR_NUMERIC and lib_table(lib) == before == ref_table(ref), (seed, step)
                    seen["zero_norm"] += 1
                    continue
                got = lib.update(C_, m, a_rows, a_prev, shift, t)
                assert got.dtype == np.int32 and got.tolist() == want.tolist(), (seed, step, got, want)
                assert lib_table(lib) == ref_table(ref), (seed, step)
                assert len(set(got.tolist())) == K                          # two columns never share an id
                seen["count_tie"] += any(want[k] < P and not np.isnan(C_[k, 0]) and m[k] == n_before[want[k]] for k in range(K))
                seen["updates"] += 1
                if use_rows:
                    kept = roster_ref.kept_rows(rows, want)
    print(seen)
    assert seen["updates"] >= 1500 and seen["zero_norm"] >= 3
    for case in ("equal_cnt", "equal_distance", "distance_is_t", "nan_row", "no_common_row", "rows_absent", "prev_absent", "count_tie", "loaded"):
        assert seen[case] >= 20, (case, seen)


def unit(*idx, scale=1.0):
    v = np.zeros(D)
    for i in idx:
        v[i] = scale
    return v


def test_known_answers_split_merge_renumbering_and_return():
    with sdhip.Roster(D) as r:
        A, B, Cc = unit(0), unit(1), unit(2)
        rows = np.zeros(10, np.int32)
        assert r.update([A], [10], rows).tolist() == [0]                     # one speaker
        kept = np.zeros(10, np.int32)
        # split: rows 0..5 stay with column 0, rows 6..9 go to a new column whose centroid is far from everybody's
        rows = np.array([0] * 6 + [1] * 4, np.int32)
        ids = r.update([A, B], [6, 4], rows, kept)
        assert ids.tolist() == [0, 1] and r.info()[:2] == (2, 2)
        kept = ids[rows]
        # the clustering renumbers its columns: the ids follow the rows, not the numbers
        rows = np.array([1] * 6 + [0] * 4, np.int32)
        ids = r.update([B, A], [4, 6], rows, kept)
        assert ids.tolist() == [1, 0]
        kept = ids[rows]
        # merge: one column again; it keeps the id most of its rows had, the other entry stays in the roster, untouched
        rows = np.zeros(10, np.int32)
        ids = r.update([unit(0, 1)], [10], rows, kept)
        assert ids.tolist() == [0] and r.info()[:2] == (2, 4)
        cen, cnt, seen = r.speakers()
        assert cnt.tolist() == [10, 4] and seen.tolist() == [3, 2] and np.array_equal(cen[0], unit(0, 1)) and np.array_equal(cen[1], B)
        # a tie of the row counts goes to the smaller column, then the smaller id: 5 rows each way
        kept = np.array([0] * 5 + [1] * 5, np.int32)
        rows = np.array([1] * 5 + [0] * 5, np.int32)
        assert r.update([A, B], [1, 1], rows, kept).tolist() == [1, 0]
        # return: no row in common with the previous table (the window moved past it); the voice near entry 1 gets id 1 back, a stranger id 2
        near_b = unit(1) + 0.05 * unit(3)
        ids = r.update([Cc, near_b], [3, 3], np.array([0, 1, 1], np.int32), kept, shift=40)
        assert ids.tolist() == [2, 1]
        # refresh: fewer rows than the entry was made from leave its centroid alone, as many or more replace it
        cen, cnt, _ = r.speakers()
        assert np.array_equal(cen[1], B) and cnt[1] == 4                     # 3 < 4
        r.update([near_b], [4], threshold=0.5)
        cen, cnt, seen = r.speakers()
        assert np.array_equal(cen[1], near_b) and cnt.tolist() == [10, 4, 3] and seen.tolist() == [4, 6, 5]
        # a threshold of 0 takes a distance of exactly 0 and nothing else (for a unit axis the three sums give exactly 0; for most vectors
        # sqrt(m) * sqrt(m) is a rounding off m); NaN columns get ids of their own and entries without a centroid
        ids = r.update([Cc, Cc + 1e-3 * unit(5), np.full(D, np.nan)], [1, 1, 7], threshold=0.0)
        assert ids.tolist() == [2, 3, 4]
        cen, cnt, _ = r.speakers()
        assert np.isnan(cen[4]).all() and cnt[4] == 0
    assert sdhip.relabel_turns_map([(0.0, 1.0, 1), (0.5, 2.0, 0), (3.0, 4.0, 1)], [7, 3]) == [(0.0, 1.0, 3), (0.5, 2.0, 7), (3.0, 4.0, 3)]


def test_refusals_leave_the_roster_unchanged():
    L = sdhip.lib()
    i64p, dp, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert L.sd_roster_open(0, C.byref(C.c_void_p())) == SD_ERR_ARG and L.sd_roster_open(D, None) == SD_ERR_ARG
    assert L.sd_roster_close(None) == 0
    assert L.sd_roster_info(None, None, None, None) == SD_ERR_ARG and L.sd_roster_speakers(None, None, None, None, 0, None) == SD_ERR_ARG
    assert L.sd_roster_load(None, None, None, 0) == SD_ERR_ARG and L.sd_roster_update(None, None, None, 0, None, 0, None, 0, 0, 0.5, None) == SD_ERR_ARG
    assert L.sd_roster_update_last(None, None, None, 0, None) == SD_ERR_ARG and L.sd_last_roster_ids(None, None, 0, None) == SD_ERR_ARG
    assert L.sd_stream_set_roster(None, None) == SD_ERR_ARG and L.sd_relabel_turns_map(None, 1, None, 1) == SD_ERR_ARG
    with sdhip.Roster(D) as r:
        r.load([unit(0), unit(1)], [3, 4])
        r.update([unit(0)], [5], np.zeros(4, np.int32))
        before = lib_table(r)
        h = r._handle()
        cen, cnt, ids = np.stack([unit(0), unit(2)]), np.array([1, 2], np.int64), np.zeros(2, np.int32)
        rows, prev = np.array([0, 1, 2], np.int32), np.array([0, 3], np.int32)
        p = sdhip._ptr
        bad = [
            (h, None, p(cnt), 2, None, 0, None, 0, 0, 0.5, p(ids)), (h, p(cen), None, 2, None, 0, None, 0, 0, 0.5, p(ids)), (h, p(cen), p(cnt), 2, None, 0, None, 0, 0, 0.5, None),
            (h, p(cen), p(cnt), -1, None, 0, None, 0, 0, 0.5, p(ids)), (h, p(cen), p(cnt), 2, None, -1, None, 0, 0, 0.5, p(ids)), (h, p(cen), p(cnt), 2, None, 0, None, -1, 0, 0.5, p(ids)),
            (h, p(cen), p(cnt), 2, None, 0, None, 0, -1, 0.5, p(ids)), (h, p(cen), p(cnt), 2, None, 0, None, 0, 0, 2.5, p(ids)), (h, p(cen), p(cnt), 2, None, 0, None, 0, 0, -0.1, p(ids)),
            (h, p(cen), p(cnt), 2, p(rows), 3, None, 0, 0, 0.5, p(ids)),                                  # a row label of K
            (h, p(cen), p(cnt), 2, None, 0, p(prev), 2, 0, 0.5, p(ids)),                                  # a previous id of P
        ]
        for args in bad:
            assert L.sd_roster_update(*args) == SD_ERR_ARG, args[3:]
        cnt[1] = -2
        assert L.sd_roster_update(h, p(cen), p(cnt), 2, None, 0, None, 0, 0, 0.5, p(ids)) == SD_ERR_ARG   # a negative count
        with pytest.raises(sdhip.SdError) as e:
            r.load([unit(3)], [1])                                           # load into a roster that is not empty
        assert e.value.code == SD_ERR_ARG
        with pytest.raises(sdhip.SdError) as e:
            r.update([np.zeros(D)], [1])                                     # a zero norm that step B has to read
        assert e.value.code == SD_ERR_NUMERIC
        assert L.sd_roster_speakers(h, None, None, None, -1, None) == SD_ERR_ARG
        assert lib_table(r) == before
        with pytest.raises(sdhip.SdError) as e:
            sdhip.relabel_turns_map([(0.0, 1.0, 0), (1.0, 2.0, 2)], [5, 6])  # label 2 outside a map of 2
        assert e.value.code == SD_ERR_ARG
        turns = (sdhip.Turn * 2)(sdhip.Turn(0.0, 1.0, 0, 0), sdhip.Turn(1.0, 2.0, -1, 0))
        assert L.sd_relabel_turns_map(turns, 2, p(ids), 2) == SD_ERR_ARG and (turns[0].label, turns[1].label) == (0, -1)      # nothing is written
        # at most cap entries are written
        out = np.full((3, D), 7.0)
        P = C.c_int64(0)
        assert L.sd_roster_speakers(h, p(out), None, None, 1, C.byref(P)) == 0 and P.value == 2 and (out[1:] == 7.0).all() and np.array_equal(out[0], unit(0))
    with sdhip.Roster(D) as empty:
        empty.load(np.zeros((0, D)), [])                                     # nothing into an empty roster: still empty, still loadable
        assert empty.info() == (0, 0, D)
        assert empty.update(np.zeros((0, D)), []).tolist() == [] and empty.info() == (0, 1, D)


def test_command_line_usage_errors():
    base = [EXE, "seg.sdw", "emb.sdw", "a.wav"]
    for args in (["--stream-roster"], ["--stream-roster", "--stream-updates"], ["--stream-roster", "--stream-window", "60"],      # only with --stream
                 ["--stream", "10", "--stream-roster", "--relabel"], ["--stream", "10", "--stream-roster", "--speakers", "v.txt"]):
        out = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and out.stderr.startswith("usage: "), (args, out.returncode, out.stderr)
    for args in (["--stream", "10", "--stream-roster"], ["--stream", "10", "--stream-roster", "--stream-window", "32", "--stream-updates"]):
        out = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and not out.stderr.startswith("usage: "), (args, out.stderr)      # the argument check passes; no model file (or no GPU) ends the run


@pytest.mark.parametrize("window", [None, 1])
def test_planted_recording_one_id_per_talker_with_exact_centroids(window):
    """the rule alone, before any GPU run: hard labels of the oracle, centroids of tests/speakers_ref.py, pieces of 10 s"""
    run = rcs.planted_run(window)
    fixed = rcs.majority_map(run)
    assert sorted(fixed) == [0, 1, 2, 3] and sorted(fixed.values()) == [0, 1, 2, 3], fixed      # four ids for four talkers, one each
    assert run[-1][4][0].shape == (4, 192)
    maps = [step[2].tolist() for step in run]
    assert any(a != b and len(a) == len(b) for a, b in zip(maps, maps[1:])) or len({tuple(m) for m in maps}) > 2      # the raw labels really do permute
    if window == 1:
        origins = [step[1] for step in run]
        assert origins == [0, 0, 0, 256000, 256000, 512000, 768000]
        who = {t: i for i, t in fixed.items()}
        assert who[0] not in run[5][2].tolist() and who[0] in run[6][2].tolist()              # talker 0 is out of the window at 60 s and back, under his id, at 70 s
        # ... by centroid: none of his rows in the last table had an id in the table before
        n, origin, ids, hard, _ = run[6]
        prev = roster_ref.kept_rows(run[5][3], run[5][2])
        shift = 3 * (origin - run[5][1]) // 8000
        k = ids.tolist().index(who[0])
        assert not any(hard[i] == k and i + shift < len(prev) and prev[i + shift] >= 0 for i in range(len(hard)))


def test_roster_under_address_and_ub_sanitizers(tmp_path):
    """csrc/roster.cpp itself with a stand-alone main: random update sequences against a naive implementation, every allocation failing in turn, every
    error leaving the roster unchanged; two seeds, no report"""
    exe = str(tmp_path / "roster_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_roster.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    src = open(os.path.join(ROOT, "tools", "sanitize", "roster_main.cpp")).read()
    assert "int main(" in src and "malloc(" in src and "hip/" not in src
    for seed in ("20241019", "7"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (out.stdout[-300:], out.stderr[-2000:])
        m = re.match(r"roster ok: (\d+) updates, (\d+) failed allocations, (\d+) refusals, (\d+) zero norms, (\d+) returns", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) >= 1000 and int(m.group(2)) >= 1000 and int(m.group(4)) >= 5, out.stdout[-300:]
