"""CPU tests of streams at another sample rate (include/sdhip.h, "streams at any sample rate"; csrc/resample_book.h): the rule F(n) -- the outputs of
n inputs that no later input can change -- against its definition and against the float64 oracle of the resample leg, the library's
sd_resample_final_len against it, the host bookkeeping under sanitizers, and the command line's usage errors."""
import os
import subprocess

import numpy as np
import pytest

import resample_stream_ref as rr
import sdhip
from oracle import resample_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")


def lengths():
    """n = 0 .. 3000, values around 2^24 and 2^30, 20 000 random n < 2^33 (most far above 2^24, a quarter below it): ascending"""
    rng = np.random.default_rng(1611)
    ns = set(range(0, 3001))
    for c in (2 ** 24, 2 ** 30):
        ns.update(range(c - 40, c + 41))
    ns.update(int(v) for v in rng.integers(0, 2 ** 33, 15000))
    ns.update(int(v) for v in rng.integers(0, 2 ** 24, 5000))
    return sorted(ns)


@pytest.mark.parametrize("sr", rr.RATES)
def test_final_len_is_the_count_of_outputs_whose_reads_lie_in_front_of_n(sr):
    for n in list(range(0, 700)) + [1000, 2999, 8000, 16000]:
        assert rr.final_len(n, sr) == rr.final_len_brute(n, sr), (sr, n)
    L, M, J = rr.plan(sr)
    one_second = {8000: 15864, 11025: 15902}.get(sr, 15933 if sr != 12345 else None)
    if one_second is not None:
        assert rr.final_len(sr, sr) == one_second


@pytest.mark.parametrize("sr", rr.RATES)
def test_final_outputs_of_a_prefix_are_those_of_the_whole_and_the_next_one_is_not(sr):
    """oracle.resample_oracle in float64 on noise: resample(x[:n])[:F(n)] == resample(x)[:F(n)] exactly, and wherever F(n) < len(n) output F(n)
    differs -- its reads reach behind the prefix.  One case cannot differ and is held to the opposite: F goes by the kernel's reads, and the outermost
    tap, h(m M - k L) at k = i0 + J, lies outside the window's support for some phases (at 8 kHz for both: |u| = 136 or 135 > half = 134.7), so where
    output F(n) misses exactly the inputs under such taps it is a sum of the same numbers and must be EQUAL.  At 8 kHz that is every n (output
    F(n) = 2 (n - J) reads up to input n itself, through the tap that is zero); there the first output behind F(n) that misses an input under a
    non-zero tap must differ instead."""
    L, M, fc, half, J = ro.plan(sr, 16000)
    rng = np.random.default_rng(sr)
    N = 2 * J + 12 * max(1, M // L) + 400
    x = rng.standard_normal(N)
    whole = ro.resample(x, sr)

    def misses_something(m, n):
        """output m of the prefix of n inputs lacks an input of the whole recording whose tap is not zero"""
        i0 = (m * M) // L
        k = np.arange(n, min(i0 + J, N - 1) + 1)
        return len(k) > 0 and bool(np.any(ro.h(m * M - k * L, L, fc, half) != 0.0))

    differ = equal = 0
    for n in sorted({1, J, J + 1, J + 2, 2 * J + 5, N // 2, N - 3, N - 1} | {int(v) for v in rng.integers(1, N, 6)}):
        f = rr.final_len(n, sr)
        part = ro.resample(x[:n], sr)
        assert len(part) == rr.out_len(n, sr) and f <= len(part)
        assert np.array_equal(part[:f], whole[:f]), (sr, n)
        if f < len(part):
            assert (f * M) // L + J >= n                          # it does read behind the prefix
            if misses_something(f, n):
                assert part[f] != whole[f], (sr, n)
                differ += 1
            else:
                assert part[f] == whole[f], (sr, n)
                later = [m for m in range(f, len(part)) if misses_something(m, n)]
                assert not later or (later[0] <= f + 2 and part[later[0]] != whole[later[0]]), (sr, n)
                equal += 1
    print("%d Hz: output F(n) differs at %d lengths, misses only zero taps at %d" % (sr, differ, equal))
    assert differ + equal >= 5 and (differ >= 1 or sr == 8000)      # (the up-sampling rates meet zero outer taps at most phases, the others at none)


def test_prefix_equality_at_8_khz_at_the_lengths_around_the_wing():
    rng = np.random.default_rng(8)
    x = rng.standard_normal(2400)
    whole = ro.resample(x, 8000)
    for n in (1, 68, 69, 70, 137, 500, 2001):
        f = rr.final_len(n, 8000)
        assert np.array_equal(ro.resample(x[:n], 8000)[:f], whole[:f]), n
    assert [rr.final_len(n, 8000) for n in (68, 69, 70)] == [0, 2, 4]


@pytest.mark.parametrize("sr", rr.RATES)
def test_library_final_len_equals_the_rule_and_both_lengths_never_shrink(sr):
    prev_f = prev_len = 0
    worst = 0
    for n in lengths():
        f, ln = rr.final_len(n, sr), rr.out_len(n, sr)
        assert sdhip.resample_final_len(n, sr) == f, (sr, n)
        assert sdhip.lib().sd_resample_len(n, sr, 16000) == ln
        assert prev_f <= f <= ln and prev_len <= ln, (sr, n)
        prev_f, prev_len = f, ln
        if n < 2 ** 24:
            worst = max(worst, ln - f)
    assert worst <= (136 if sr == 8000 else 100), (sr, worst)      # the lag of the stream behind its audio: 8.5 ms at 8 kHz
    assert sdhip.resample_final_len(-1, sr) == -1 and sdhip.resample_final_len(10, 0) == -1 and sdhip.resample_final_len(10, sr, 0) == -1
    assert sdhip.resample_final_len(5000, 16000) == 5000 - 68      # (the rule as such; a stream at 16 000 has no resampler)


def test_symbols_are_exported_declared_and_cited():
    import re
    L = sdhip.lib()
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    for name in ("sd_stream_set_input_rate", "sd_stream_end_input", "sd_stream_input_info", "sd_resample_final_len"):
        assert hasattr(L, name) and name in sdhip.EXPORTS
        line = re.search(r"^[a-z0-9_]+ " + name + r"\(.*$", hdr, re.M)
        assert line and re.search(r"\);\s+/\* .*resampler\.cc:\d+-\d+.*\*/$", line.group(0)), name      # one line, with the citation the header's entries carry
    assert "F(n) = min(len(n)" in hdr
    hook = open(os.path.join(ROOT, "include", "sdhip_stream_test.h")).read()
    assert "sd_test_stream_tail" in hook and hasattr(L, "sd_test_stream_tail") and sdhip.STREAM_TEST_EXPORTS == ["sd_test_stream_tail"]


def test_rate_bookkeeping_under_address_and_ub_sanitizers(tmp_path):
    """the host bookkeeping of a stream with an input rate (csrc/resample_book.h) as a stand-alone CPU program with the device calls stubbed by
    malloc'd memory of exactly the size asked for and the kernel body restated in float (tools/sanitize/build_resample_book.sh): random piece
    sequences at seven rates, pieces of one sample included, give the one-shot outputs; every allocation fails in turn and leaves the book as it
    was; two seeds, no report, every allocation released"""
    exe = str(tmp_path / "resample_book_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_resample_book.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
    for seed in ("20240611", "7"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("resample_book ok"), (out.stdout[-300:], out.stderr[-2000:])
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr


@pytest.mark.parametrize("args,word", [
    (["missing.wav", "--stream-rate", "8000"], "--stream-rate"),                             # without --stream
    (["missing.wav", "--stream", "2", "--stream-rate", "8000"], "--stream-rate"),            # with a wav path instead of -
    (["-", "--stream", "2", "--stream-rate", "0"], "--stream-rate"), (["-", "--stream", "2", "--stream-rate", "-8000"], "--stream-rate"),
    (["-", "--stream", "2", "--stream-rate", "8000.5"], "--stream-rate"), (["-", "--stream", "2", "--stream-rate", "abc"], "--stream-rate"),
    (["-", "--stream", "2", "--stream-rate"], "--stream-rate"),
])
def test_cli_usage_errors_of_stream_rate_exit_2_before_anything_touches_the_gpu(args, word):
    """the model files do not exist: a run that got as far as sd_create would say so and exit 1"""
    out = subprocess.run([EXE, "missing_seg.sdw", "missing_emb.sdw"] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "usage" in out.stderr and word in out.stderr and "sd_create" not in out.stderr and out.stdout == ""
