"""CPU tests of the sliding window of sd_stream (sd_stream_forget, sd_stream_set_window, sd_stream_origin): the exported names and declarations, the
command line's usage errors, and the book-keeping of csrc/stream_book.h (book_forget next to reserve, push, seal and the group steps) as a stand-alone
program under AddressSanitizer + UBSan (tools/sanitize/build_stream_window.sh).  Nothing loaded into python runs under a sanitizer."""
import os
import re
import subprocess

import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
NAMES = ("sd_stream_forget", "sd_stream_set_window", "sd_stream_origin")


def test_exports_and_declarations():
    L = sdhip.lib()
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    for name in NAMES:
        assert name in sdhip.EXPORTS and hasattr(L, name)
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
    assert re.search(r"^int sd_stream_forget\(sd_stream\*, int64_t keep_blocks\);", hdr, re.M)
    assert re.search(r"^int sd_stream_origin\(const sd_stream\*, int64_t\* first_sample\);", hdr, re.M)
    for method in ("forget", "set_window", "origin"):
        assert callable(getattr(sdhip.Stream, method))
    # a null stream is refused before anything is dereferenced
    assert L.sd_stream_forget(None, 1) == 1 and L.sd_stream_set_window(None, 1) == 1 and L.sd_stream_origin(None, None) == 1


def test_command_line_usage_errors():
    base = [EXE, "seg.sdw", "emb.sdw", "a.wav"]
    for args in (["--stream-window", "60"],                               # only with --stream
                 ["--stream", "10", "--stream-window"], ["--stream", "10", "--stream-window", "0"], ["--stream", "10", "--stream-window", "-5"],
                 ["--stream", "10", "--stream-window", "abc"], ["--stream", "10", "--stream-window", "nan"], ["--stream", "10", "--stream-window", "10s"]):
        out = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and out.stderr.startswith("usage: "), (args, out.returncode, out.stderr)
    out = subprocess.run(base + ["--stream", "10", "--stream-window", "600"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and not out.stderr.startswith("usage: ")     # a good value passes the argument check; no model file (or no GPU) ends the run


def test_book_keeping_of_the_window_under_address_and_ub_sanitizers(tmp_path):
    """random sequences of reserve, push, seal, forget, the window's policy and the group variants on malloc'd memory of exactly the size asked for: after
    every step the book's samples and rows are those of a fresh book fed the kept samples; a failed allocation leaves the book unchanged; two seeds,
    no report, every allocation released"""
    exe = str(tmp_path / "stream_window_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_stream_window.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
    src = open(os.path.join(ROOT, "tools", "sanitize", "stream_window_main.cpp")).read()
    assert "int main(" in src and "malloc(" in src and "hip/" not in src
    for seed in ("20241019", "7"):
        out = subprocess.run([exe, seed], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, (out.stdout[-300:], out.stderr[-2000:])
        m = re.match(r"stream_window ok: (\d+) allocations, (\d+) forgets, (\d+) failed allocations", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(2)) >= 20 and int(m.group(3)) >= 20, out.stdout[-300:]
