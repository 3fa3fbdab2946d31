"""CPU tests of the scoring entries (csrc/der.cpp; include/sdhip.h: sd_der, sd_read_rttm, sd_score_error) and of the command line's --score / --tune
refusals: sd_der against the exact rational reference tests/der_ref.py, which tests/test_der_ref.py pins.

Tolerance.  sd_der takes every interval length as one f64 subtraction (an error of at most 2^-53 of the length) and adds the lengths up in sums that
carry their rounding errors; der_ref does the same in exact fractions.  With n scored elementary intervals of summed length `extent`, one rounding per
interval length plus the additions of the sum stay below n * 2^-52 * extent for every component: the bound asserted, derived and not measured."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sdhip
import der_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
SD_ERR_ARG = 1


def _check(ref, hyp, opt, tag):
    want = dr.der(ref, hyp, **opt)
    got = sdhip.der(ref, hyp, **opt)
    bound = want["n"] * Fraction(1, 2 ** 52) * want["extent"]
    for k in dr.COMPONENTS:
        assert abs(Fraction(got[k]) - want[k]) <= bound, (tag, k, got[k], float(want[k]), float(bound))
    if want["der"] is None:
        assert np.isnan(got["der"]), tag
    else:
        assert got["der"] == (got["missed"] + got["false_alarm"] + got["confusion"]) / got["total"], tag
    # the mapping handed out is one-to-one, pairs labels that exist, and is optimal: its exact `correct` is the optimum's
    m = got["map"]
    assert len(set(m.values())) == len(m) and set(m) <= {t[2] for t in hyp} and set(m.values()) <= {t[2] for t in ref}, tag
    assert abs(dr.correct_of(ref, hyp, m, **opt) - want["correct"]) <= bound, (tag, m, want["map"])
    return got, want


@pytest.mark.parametrize("name", sorted(dr.hand_cases()))
def test_hand_computed_cases(name):
    ref, hyp, opt, expect = dr.hand_cases()[name]
    got, _ = _check(ref, hyp, opt, name)
    for k in dr.COMPONENTS:
        assert got[k] == expect[k], (name, k)             # times that are exact in binary: exact results


def test_random_cases_against_the_exact_reference():
    seen = dict(uem=0, collar=0, skip_overlap=0, empty=0, six=0)
    for seed in range(500):
        ref, hyp, opt = dr.random_case(seed)
        _check(ref, hyp, opt, seed)
        for k in opt:
            seen[k] += 1
        seen["empty"] += not ref or not hyp
        seen["six"] += len({t[2] for t in ref}) == 6 or len({t[2] for t in hyp}) == 6
    assert all(v >= 5 for v in seen.values()), seen


def test_more_labels_than_a_brute_force_can_try():
    """12 speakers a side, hypothesis = reference under a label permutation plus a little noise: the solver must find the permutation"""
    rng = np.random.default_rng(3)
    perm = rng.permutation(12)
    ref = [(float(i), float(i) + 1.5, int(i % 12)) for i in range(60)]
    hyp = [(a + 0.125, b, int(perm[k]) + 100) for a, b, k in ref]
    got = sdhip.der(ref, hyp)
    assert got["map"] == {int(perm[k]) + 100: k for k in range(12)}
    assert got["confusion"] == 0 and got["missed"] > 0 and got["false_alarm"] == 0 and got["total"] == 90.0


@pytest.mark.parametrize("ref,hyp,kw", [
    ([(0.0, 1.0, -1)], [], {}),
    ([(0.0, 1.0, 0)], [(0.0, 1.0, -3)], {}),
    ([(2.0, 1.0, 0)], [], {}),
    ([(0.0, 1.0, 0)], [(3.0, 2.5, 0)], {}),
    ([(float("nan"), 1.0, 0)], [], {}),
    ([(0.0, float("nan"), 0)], [], {}),
    ([(-0.5, 1.0, 0)], [], {}),
    ([(0.0, 1.0, 0)], [], dict(uem=[(2.0, 1.0)])),
    ([(0.0, 1.0, 0)], [], dict(collar=-0.1)),
    ([(0.0, 1.0, 0)], [], dict(collar=float("nan"))),
])
def test_refusals(ref, hyp, kw):
    with pytest.raises(sdhip.SdError) as e:
        sdhip.der(ref, hyp, **kw)
    assert e.value.code == SD_ERR_ARG and "sd_der" in str(e.value)


# ------------------------------------------------------------------ sd_read_rttm
def test_rttm_round_trip_of_the_library_writer(tmp_path):
    turns = [(0.5, 2.25, 2), (2.25, 3.0, 0), (3.5, 7.125, 2), (8.0, 8.5, 5)]
    path = str(tmp_path / "a.rttm")
    sdhip.write_rttm_named(path, "rec", turns, ["anna", None, "bob"])
    got, names = sdhip.read_rttm(path)
    assert names == ["bob", "anna", "SPEAKER_05"]                # order of first appearance
    assert got == [(0.5, 2.25, 0), (2.25, 3.0, 1), (3.5, 7.125, 0), (8.0, 8.5, 2)]
    assert sdhip.der(turns, got)["der"] == 0.0
    sdhip.write_rttm(path, "rec", turns, conf=[0.5, float("nan"), 1.0, 1.5])
    got, names = sdhip.read_rttm(path, uri="rec")
    assert names == ["SPEAKER_02", "SPEAKER_00", "SPEAKER_05"] and len(got) == 4
    assert sdhip.read_rttm(path, uri="other") == ([], [])


def test_rttm_as_pyannote_writes_it_and_the_uri_filter(tmp_path):
    path = tmp_path / "p.rttm"
    path.write_text(";; a comment\n"
                    "SPEAKER fileA 1 0.031 1.520 <NA> <NA> SPEAKER_01 <NA> <NA>\n"
                    "\n"
                    "SPKR-INFO fileA 1 <NA> <NA> <NA> unknown SPEAKER_01 <NA>\n"
                    "SPEAKER\tfileB  1   4.000   2.500 <NA> <NA> spk_b <NA> <NA>\n"
                    "SPEAKER fileA 1 1.551 0.25 <NA> <NA> SPEAKER_00 <NA> 0.9\n")
    turns, names = sdhip.read_rttm(str(path))
    assert names == ["SPEAKER_01", "spk_b", "SPEAKER_00"]
    assert turns == [(0.031, 0.031 + 1.520, 0), (4.0, 6.5, 1), (1.551, 1.551 + 0.25, 2)]
    turns, names = sdhip.read_rttm(str(path), uri="fileA")
    assert names == ["SPEAKER_01", "SPEAKER_00"] and [t[2] for t in turns] == [0, 1]


@pytest.mark.parametrize("line,why", [
    ("SPEAKER fileA 1 0.5 abc <NA> <NA> s <NA> <NA>", "abc"),
    ("SPEAKER fileA 1 -0.5 1.0 <NA> <NA> s <NA> <NA>", "-0.5"),
    ("SPEAKER fileA 1 0.5 nan <NA> <NA> s <NA> <NA>", "nan"),
    ("SPEAKER fileA 1 0.5 1.0 <NA>", "8 fields"),
])
def test_a_malformed_rttm_line_is_named(tmp_path, line, why):
    path = tmp_path / "bad.rttm"
    path.write_text("SPEAKER fileA 1 0.0 1.0 <NA> <NA> s <NA> <NA>\n\n" + line + "\n")
    with pytest.raises(sdhip.SdError) as e:
        sdhip.read_rttm(str(path))
    assert e.value.code == SD_ERR_ARG and "line 3" in str(e.value) and why in str(e.value) and "bad.rttm" in str(e.value)
    with pytest.raises(sdhip.SdError) as e:
        sdhip.read_rttm(str(tmp_path / "absent.rttm"))
    assert "cannot open" in str(e.value)


# ------------------------------------------------------------------ the command line refuses before it touches the GPU
def _good_rttm(tmp_path):
    p = tmp_path / "ref.rttm"
    p.write_text("SPEAKER a 1 0.0 1.0 <NA> <NA> s <NA> <NA>\n")
    return str(p)


@pytest.mark.parametrize("flags", [
    ["--score", "@absent"], ["--score", "@bad"], ["--score"], ["--score", "@good", "--collar", "-1"], ["--score", "@good", "--collar", "x"],
    ["--score", "@good", "--tune", "@good", "--thresholds", "0.3:1.2:4"], ["--score", "@good", "--stream", "5"], ["--score", "@good", "--activity", "speech"],
    ["--tune", "@good"], ["--tune", "@absent", "--thresholds", "0.3:1.2:4"], ["--tune", "@bad", "--thresholds", "0.3:1.2:4"],
    ["--tune", "@good", "--thresholds", "0.3:1.2"], ["--tune", "@good", "--thresholds", "1.2:0.3:4"], ["--tune", "@good", "--thresholds", "0.3:2.5:4"],
    ["--tune", "@good", "--thresholds", "0.3:1.2:0"], ["--tune", "@good", "--thresholds", "a:b:c"], ["--tune", "@good", "--thresholds", "0.3:1.2:4x"],
    ["--tune", "@good", "--thresholds", "0.3:1.2:4", "--min-cluster-sizes", "5,0"], ["--tune", "@good", "--thresholds", "0.3:1.2:4", "--min-cluster-sizes", "5,,7"],
    ["--tune", "@good", "--thresholds", "0.3:1.2:4", "--min-cluster-sizes", "five"], ["--tune", "@good", "--thresholds", "0.3:1.2:4", "--gpus", "2"],
    ["--tune", "@good", "--thresholds", "0.3:1.2:4", "--dump-steps", "/tmp"], ["--thresholds", "0.3:1.2:4"], ["--collar", "0.25"], ["--skip-overlap"],
])
def test_cli_refuses_a_bad_score_or_tune_request_before_touching_the_gpu(flags, tmp_path):
    """the model and wav paths do not exist: a command line that got as far as opening a model or a device would say so instead of `usage`"""
    bad = tmp_path / "bad.rttm"
    bad.write_text("SPEAKER a 1 zero 1.0 <NA> <NA> s <NA> <NA>\n")
    sub = {"@good": _good_rttm(tmp_path), "@bad": str(bad), "@absent": str(tmp_path / "absent.rttm")}
    out = subprocess.run([EXE, str(tmp_path / "no_seg.sdw"), str(tmp_path / "no_emb.sdw"), str(tmp_path / "no.wav")] + [sub.get(f, f) for f in flags],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2
    assert "usage" in out.stderr and "sd_create" not in out.stderr and "failed" not in out.stderr
    assert "Speaker_" not in out.stdout and "DER" not in out.stdout + out.stderr
