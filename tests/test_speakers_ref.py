"""CPU tests of the known-speaker references (tests/speakers_ref.py) and of the host-only entries: the centroid reference is pinned to the oracle
through the soft table it must reproduce bit for bit, the span-mask rule to the frame map of the front end, the greedy matching to its tie rules,
and the voiceprint file / named RTTM writers to their formats."""
import os
import re

import numpy as np
import pytest

import sdhip
from oracle import orc

import speakers_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")


# ------------------------------------------------------------------ centroids: pinned to the oracle's soft table
def _soft_from(emb, cen):
    """2 - sequential cosine distance of every row to every centroid; rows without an embedding excluded"""
    flat = emb.reshape(-1, emb.shape[-1])
    ok = ~np.isnan(flat[:, 0])
    return ok, 2.0 - sr.cosine_distances(cen, flat[ok]).T


@pytest.mark.parametrize("case", ["plain", "num_clusters=2", "small cluster"])
def test_centroid_reference_reproduces_the_oracle_soft_table(case):
    kw = {}
    emb = sr.planted_embeddings(small=5 if case == "small cluster" else 0)
    if case == "num_clusters=2":
        kw["num_clusters"] = 2
    hard, K, train = orc.clustering(emb, **kw)
    N = int((~np.isnan(emb.reshape(-1, sr.DIM)[:, 0])).sum())
    assert 80 <= N <= 100 and len(train) == N
    assert K == (2 if case == "num_clusters=2" else 3)
    if case == "small cluster":
        # the five rows are a cluster of their own for the linkage (K = 4 when nothing is too small) and too small for the default: remapped
        assert orc.clustering(emb, min_cluster_size=1)[1] == 4 and min(15, max(1, round(0.1 * N))) > 5
    cen, cnt = sr.centroids(emb, train)
    assert cen.shape == (K, sr.DIM) and cnt.sum() == N and (cnt > 0).all()
    _, K2, soft = orc.clustering_full(emb, **kw)
    assert K2 == K
    ok, ref = _soft_from(emb, cen)
    assert np.array_equal(soft.reshape(-1, K)[ok], ref)
    assert np.array_equal(np.argmax(ref, 1), hard.reshape(-1)[ok])


def test_centroid_reference_without_train_rows():
    cen, cnt = sr.centroids(np.full((4, 3, 8), np.nan), np.zeros(0, np.int32))
    assert cen.shape == (1, 8) and np.isnan(cen).all() and list(cnt) == [0]


# ------------------------------------------------------------------ span masks
def test_mask_frames_partition_the_chunk_as_the_front_end_does():
    per_frame = np.diff(sr.frame_start(np.arange(sr.FRAMES + 1)))
    assert per_frame.sum() == sr.CHUNK and sr.frame_start(0) == 0 and sr.frame_start(sr.FRAMES) == sr.CHUNK
    assert np.array_equal(per_frame, np.bincount((np.arange(sr.CHUNK, dtype=np.int64) * sr.FRAMES) // sr.CHUNK, minlength=sr.FRAMES))
    # ... and both device files state that map in the same words
    expr = r"\(int\)\(\(\(int64_t\)SD_CHUNK \* f \+ \(SD_FRAMES - 1\)\) / SD_FRAMES\)"
    for f, name in (("frontend.hip", "frame_start"), ("speakers.hip", "span_frame_start")):
        src = open(os.path.join(PKG, "csrc", f)).read()
        assert re.search(r"int %s\(int f\) \{ return %s; \}" % (name, expr), src), f


def test_span_rounding_merging_and_labels():
    n = 100000
    spans = [(1.0, 2.0, 0), (1.5, 2.5, 0), (0.00390625, 0.5, 1), (6.0, 9.0, 0), (7.0, 8.0, 0), (3.0, 3.0, 0)]
    assert sr.span_samples(spans, 0, n) == [(16000, 40000), (96000, n)]
    assert sr.span_samples(spans, 1, n) == [(62, 8000)]                      # 62.5 samples rounds to even
    assert sr.span_samples([(0.01171875, 0.5, 1)], 1, n) == [(188, 8000)]    # 187.5 too
    assert sr.span_samples(spans, -1, n) == [(62, 8000), (16000, 40000), (96000, n)]
    assert sr.span_samples(None, 3, n) == [(0, n)] and sr.span_samples([], -1, n) == [(0, n)] and sr.span_samples([], 0, n) == []
    m = sr.span_masks(n, spans, 0)
    assert m.shape == (sr.num_chunks(n) * 3, sr.FRAMES) and not m[1::3].any() and not m[2::3].any()
    fs = sr.frame_start(np.arange(sr.FRAMES))
    assert np.array_equal(m[0] > 0, (fs >= 16000) & (fs < 40000))
    assert np.array_equal(m[3 * 2] > 0, ((2 * sr.HOP + fs >= 16000) & (2 * sr.HOP + fs < 40000)) | ((2 * sr.HOP + fs >= 96000) & (2 * sr.HOP + fs < n)))


# ------------------------------------------------------------------ matching
def test_greedy_matching_rules():
    inf = 9.0
    # a tie on distance goes to the lower k, then the lower m
    d = np.array([[0.2, 0.2], [0.2, 0.2]])
    assert list(sr.greedy_match(d, 0.5)[0]) == [0, 1]
    d = np.array([[inf, 0.2], [0.2, 0.2]])
    assert list(sr.greedy_match(d, 0.5)[0]) == [1, 0]                        # (0.2, 0, 1) first, then (0.2, 1, 0)
    # dist == threshold matches, the next float above does not
    d = np.array([[0.25]])
    assert list(sr.greedy_match(d, 0.25)[0]) == [0] and list(sr.greedy_match(d, np.nextafter(0.25, 0.0))[0]) == [-1]
    # greedy, not optimal: cluster 1's only candidate under the threshold is taken by cluster 0
    d = np.array([[0.1, 0.3], [0.2, inf]])
    match, best = sr.greedy_match(d, 0.5)
    assert list(match) == [0, -1] and best[0] == 0.1 and np.isnan(best[1])
    # NaN rows (skipped centroids) match nobody
    d = np.array([[np.nan, np.nan], [0.1, 0.05]])
    assert list(sr.greedy_match(d, 0.5)[0]) == [-1, 1]


def test_default_threshold_is_half_the_squared_clustering_threshold():
    t = float(np.float32(0.7153814381597874))
    assert sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT == t * t / 2 and abs(t * t / 2 - 0.2558853) < 1e-6


# ------------------------------------------------------------------ voiceprint files and named RTTM (host-only: no GPU)
def test_voiceprint_file_round_trip_is_bit_exact(tmp_path):
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((3, sr.DIM)) * np.exp(8.0 * rng.standard_normal((3, sr.DIM)))
    emb[0, :4] = [0.1, 1.0 / 3.0, 5e-324, -1.7976931348623157e308]
    names = ["alice", "bob_2", "Zoë"]
    a, b = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    sdhip.write_voiceprints(a, names, emb)
    n1, e1 = sdhip.read_voiceprints(a)
    assert n1 == names and e1.dtype == np.float64 and np.array_equal(e1.view(np.uint64), emb.view(np.uint64))
    sdhip.write_voiceprints(b, n1, e1)
    assert open(a, "rb").read() == open(b, "rb").read()
    n2, e2 = sdhip.read_voiceprints(b)
    assert n2 == names and np.array_equal(e2.view(np.uint64), emb.view(np.uint64))
    lines = open(a).read().splitlines()
    assert len(lines) == 3 and lines[0].split()[0] == "alice" and lines[0].split()[1] == "%.17g" % 0.1 and len(lines[1].split()) == sr.DIM + 1
    # comments and blank lines
    with open(a, "w") as f:
        f.write("# gallery\n\n" + lines[1] + "   # the second one\n   \n" + lines[0] + "\n")
    n3, e3 = sdhip.read_voiceprints(a)
    assert n3 == ["bob_2", "alice"] and np.array_equal(e3, emb[[1, 0]])
    sdhip.write_voiceprints(a, [], np.zeros((0, sr.DIM)))
    assert sdhip.read_voiceprints(a) [0] == []


def test_voiceprint_file_of_integer_valued_vectors(tmp_path):
    p = str(tmp_path / "int.txt")
    v = np.arange(sr.DIM) - 7
    with open(p, "w") as f:
        f.write("counting\t" + " ".join(str(int(x)) for x in v) + "\nmixed " + " ".join(["16", "1e2", "-0"] + ["3"] * (sr.DIM - 3)) + "\n")
    names, emb = sdhip.read_voiceprints(p)
    assert names == ["counting", "mixed"] and np.array_equal(emb[0], v.astype(np.float64))
    assert list(emb[1, :4]) == [16.0, 100.0, 0.0, 3.0] and np.signbit(emb[1, 2])


def test_malformed_voiceprint_files_name_the_line(tmp_path):
    good = "a " + " ".join(["1"] * sr.DIM)
    cases = {"short": "b " + " ".join(["1"] * (sr.DIM - 1)), "long": "b " + " ".join(["1"] * (sr.DIM + 1)), "word": "b " + " ".join(["1"] * (sr.DIM - 1) + ["x1"]),
             "nan": "b " + " ".join(["1"] * (sr.DIM - 1) + ["nan"]), "inf": "b " + " ".join(["inf"] + ["1"] * (sr.DIM - 1)), "twice": good, "name only": "b"}
    for what, line in cases.items():
        p = str(tmp_path / "bad.txt")
        with open(p, "w") as f:
            f.write("# header\n" + good + "\n\n" + line + "\n")
        with pytest.raises(sdhip.SdError) as e:
            sdhip.read_voiceprints(p)
        assert e.value.code == 1 and "line 4" in str(e.value), (what, str(e.value))
    with pytest.raises(sdhip.SdError) as e:
        sdhip.read_voiceprints(str(tmp_path / "absent.txt"))
    assert e.value.code == 1 and "cannot open" in str(e.value)
    for names in (["two words"], [""], ["a#b"], ["tab\tbed"], ["a", "a"]):
        with pytest.raises(sdhip.SdError) as e:
            sdhip.write_voiceprints(str(tmp_path / "w.txt"), names, np.ones((len(names), sr.DIM)))
        assert e.value.code == 1
    with pytest.raises(sdhip.SdError):
        sdhip.write_voiceprints(str(tmp_path / "w.txt"), ["a"], np.full((1, sr.DIM), np.nan))


def test_named_rttm(tmp_path):
    turns = [(0.5, 2.25, 1), (2.5, 3.0, 0), (3.0, 4.0, 2), (4.0, 5.0, 12)]
    p = str(tmp_path / "x.rttm")
    sdhip.write_rttm_named(p, "rec", turns, ["ann", None, "carl"], conf=[1.5, float("nan"), 0.25, 2.0])
    assert open(p).read().splitlines() == ["SPEAKER rec 1 0.500 1.750 <NA> <NA> SPEAKER_01 <NA> 1.5000", "SPEAKER rec 1 2.500 0.500 <NA> <NA> ann <NA> <NA>",
                                           "SPEAKER rec 1 3.000 1.000 <NA> <NA> carl <NA> 0.2500", "SPEAKER rec 1 4.000 1.000 <NA> <NA> SPEAKER_12 <NA> 2.0000"]
    q = str(tmp_path / "y.rttm")
    sdhip.write_rttm_named(p, "rec", turns, [])
    sdhip.write_rttm(q, "rec", turns)
    assert open(p).read() == open(q).read()                                   # no names: sd_write_rttm's file
    with pytest.raises(sdhip.SdError):
        sdhip.write_rttm_named(p, "rec", turns, ["two words"])


# ------------------------------------------------------------------ command line: bad values are usage errors before anything touches the GPU
@pytest.mark.parametrize("flags", [
    ["--speakers"], ["--speakers", ""], ["--speakers", "f.txt", "--speakers-threshold", "2.5"], ["--speakers", "f.txt", "--speakers-threshold", "-0.1"],
    ["--speakers", "f.txt", "--speakers-threshold", "nan"], ["--speakers", "f.txt", "--speakers-threshold", "0.2x"], ["--speakers-threshold", "0.2"],
    ["--enroll", "A"], ["--enroll", "two words", "--speakers", "f.txt"], ["--enroll", "", "--speakers", "f.txt"], ["--enroll", "a#b", "--speakers", "f.txt"],
    ["--enroll", "A", "--speakers", "f.txt", "--enroll-span", "5"], ["--enroll", "A", "--speakers", "f.txt", "--enroll-span", "5", "2"],
    ["--enroll", "A", "--speakers", "f.txt", "--enroll-span", "-1", "2"], ["--enroll", "A", "--speakers", "f.txt", "--enroll-span", "0", "nan"],
    ["--enroll", "A", "--speakers", "f.txt", "--enroll-span", "0", "1s"], ["--speakers", "f.txt", "--enroll-span", "0", "1"],
    ["--enroll", "A", "--speakers", "f.txt", "--speakers-threshold", "0.2"], ["--enroll", "A", "--speakers", "f.txt", "--stream", "5"],
    ["--speakers", "f.txt", "--activity", "speech"], ["--speakers", "f.txt", "--gpus", "2"], ["--enroll", "A", "--speakers", "f.txt", "--gpus", "2"]])
def test_cli_refuses_bad_speaker_flags_before_touching_the_gpu(flags, tmp_path):
    import subprocess
    exe = os.path.join(PKG, "speakerDiarizer")
    out = subprocess.run([exe, "no_seg.sdw", "no_emb.sdw", "no.wav"] + flags, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "usage" in out.stderr and "sd_create" not in out.stderr and "failed" not in out.stderr
    assert "Speaker_" not in out.stdout and "enrolled" not in out.stdout and not os.listdir(str(tmp_path))
