"""CPU tests of the incremental path (sd_stream_*): the sealing rule, the command line's usage errors, and that the planted 75 s case the GPU
tests compare on is not degenerate at any prefix they use."""
import os
import subprocess

import numpy as np
import pytest

import sdhip
import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")


def test_sealed_chunks_against_the_definition():
    """sealed(n) = 32 * (full(n) / 32), full(n) = chunks k with k * 8000 + 80000 < n (strict: the chunk that ends at n is the reference's last chunk)"""
    edges = {0: 0, 1: 0, 80000: 0, 80001: 0, 327999: 0, 328000: 0, 328001: 32, 583999: 32, 584000: 32, 584001: 64}
    for n, want in edges.items():
        assert sdhip.sealed_chunks(n) == want == sc.sealed(n), n
    rng = np.random.default_rng(75)
    for n in rng.integers(0, 2 ** 31, 10000):
        n = int(n)
        f = sc.full(n)
        assert f >= 0 and (f == 0 or (f - 1) * 8000 + 80000 < n) and not f * 8000 + 80000 < n, n      # chunk f - 1 is full, chunk f is not
        got = sdhip.sealed_chunks(n)
        assert got == 32 * (f // 32), n
        assert got <= sdhip.num_chunks(n)[0] and sdhip.num_chunks(n)[0] - got <= 32


@pytest.mark.parametrize("args,word", [
    (["--stream", "0"], "--stream"), (["--stream", "-3"], "--stream"), (["--stream", "abc"], "--stream"), (["--stream", "1e-9"], "--stream"),
    (["--stream", "nan"], "--stream"), (["--stream"], "--stream"),
    (["--stream", "10", "--gpus", "2"], "--gpus"), (["--stream", "10", "--activity", "speech"], "--activity"),
    (["--stream", "10", "--dump-steps", "/tmp"], "--dump-steps"), (["--stream-updates"], "--stream-updates"), (["-"], "--stream"),
])
def test_cli_usage_errors_exit_2_before_anything_touches_the_gpu(args, word):
    """the model files do not exist: a run that got as far as sd_create would say so and exit 1"""
    wav = [] if args == ["-"] else ["missing.wav"]
    order = ["missing_seg.sdw", "missing_emb.sdw"] + wav + args
    out = subprocess.run([EXE] + order, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "usage" in out.stderr and word in out.stderr and "sd_create" not in out.stderr
    assert out.stdout == ""


def test_planted_75s_case_is_not_degenerate_at_any_prefix():
    """the equalities of the GPU tests are not equalities of empty lists: from the first seal on every prefix has at least two clusters and four
    turns, the whole recording four speakers"""
    scores, emb = sc.planted75()
    assert scores.shape == (141, 293, 3) and emb.shape == (423, 192)
    for n in sc.PLANTED_PREFIXES:
        turns, K = sc.planted_oracle(n)
        print("prefix %d: %d turns, K = %d" % (n, len(turns), K))
        assert K >= 2 and len(turns) >= 4, (n, K, len(turns))
    turns, K = sc.planted_oracle(sc.N)
    assert K == 4 and len({t[2] for t in turns}) == 4


def test_stream_bookkeeping_under_address_and_ub_sanitizers(tmp_path):
    """the host bookkeeping of a stream (csrc/stream_book.h: sealing rule, tail offsets through appends and compactions, growth of the two caches) as
    a stand-alone CPU program with the device calls stubbed by malloc'd memory of exactly the size asked for, built with AddressSanitizer + UBSan
    (tools/sanitize/build_stream_book.sh): two seeds, no report, every allocation released"""
    exe = str(tmp_path / "stream_book_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_stream_book.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
    for seed in ("20240607", "7"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("stream_book ok"), (out.stdout[-300:], out.stderr[-2000:])
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
