"""CPU test of csrc/wav_file.h -- the wav reader and the rule that turns a file and the SD_WAV_* flags into the samples the pipeline diarizes -- as a
stand-alone program under AddressSanitizer + UBSan (tools/sanitize/wav_file_main.cpp, built by tools/sanitize/build_wav_file.sh): well-formed files,
stream headers and odd sizes, refused and hostile files, each under every flag set.  What the program prints is compared, as bytes, with the library's
own readers (host calls, no GPU), with the oracle's reader on the well-formed files, and with the loading rule restated here in numpy."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import sdhip
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLE, DOWNMIX, ASSUME_16K = 1, 2, 4
FLAG_SETS = (0, RESAMPLE, DOWNMIX, ASSUME_16K, DOWNMIX | ASSUME_16K)
PCM16, F32, F32_OFF_RATE, UNREADABLE, OFF_RATE, NO_SAMPLES = range(6)


def wav(samples, bits=16, channels=1, sr=16000, fmt_size=16, before=b"", after=b"", announce=None):
    data = np.asarray(samples).astype({8: np.int8, 16: "<i2", 24: "<i4", 32: "<i4"}[bits]).tobytes()
    if bits == 24:
        data = data[:len(data) // 4 * 3]
    fmt = struct.pack("<HHIIHH", 1, channels, sr, sr * channels * bits // 8, channels * bits // 8 & 0xFFFF, bits) + b"\0" * (fmt_size - 16 if 16 < fmt_size < 100 else 0)
    body = before + b"data" + struct.pack("<I", len(data) if announce is None else announce) + data + after
    return b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<I", fmt_size) + fmt + body


S = np.array([0, 1, -1, 300, -300, 32767, -32768, 12345, -2, 77, 1000, -1000], np.int64)
LIST = b"LIST" + struct.pack("<I", 6) + b"abcdef"
LIST_ODD = b"LIST" + struct.pack("<I", 11) + b"INFOabcdefg" + b"\0" + b"id3 " + struct.pack("<I", 4) + b"wxyz"
# name -> (bytes, samples the readers deliver (n), or None where both refuse the file)
WELL_FORMED = {
    "mono16": (wav(S), 12), "stereo16": (wav(S, channels=2), 6), "mono8": (wav(S % 128 - 64, bits=8), 12), "mono32": (wav(S * 65536 + 5, bits=32), 12),
    "fmt18": (wav(S, fmt_size=18), 12), "fmt40": (wav(S * 3 % 999, bits=32, fmt_size=40), 12), "list_front": (wav(S, before=LIST), 12),
    "empty_then_list": (wav([], after=LIST_ODD), 0), "mono44k": (wav(S, sr=44100), 12),
}
STREAMED = {
    "stream_ff": (wav(S, announce=0xFFFFFFFF), 12), "stream_0": (wav(S, announce=0), 12), "cut": (wav(S, announce=4000), 12),
    "odd_bytes": (wav(S)[:-1], 11),          # the header still announces 24 bytes: 23 are there, 11 whole samples
}
REFUSED = {
    "bits24": (wav(S, bits=24), None), "len0": (b"", None), "len10": (wav(S)[:10], None), "len43": (wav(S)[:43], None), "len44": (wav(S)[:44], 0),
    "fmt8": (wav(S, fmt_size=8), None), "fmt_huge": (wav(S, fmt_size=0x7FFFFFF0), None),
    "chunk_past_end": (wav(S, before=b"LIST" + struct.pack("<I", 0x7FFFFF00) + b"abcdef"), None),
    "no_data": (wav(S).replace(b"data", b"dat_"), None), "ch0": (wav(S, channels=0), 12), "ch65535": (wav(S[:4], channels=65535), 0),
    "empty44k": (wav([], sr=44100), 0),
}
FILES = {**WELL_FORMED, **STREAMED, **REFUSED}


def lib_read(path, f32):
    """the library's reader through the C ABI: (ALL n * max(ch, 1) interleaved samples, n, sr, ch) or None -- sdhip.read_wav* keep the first n only"""
    L = sdhip.lib()
    p = (C.POINTER(C.c_float) if f32 else C.POINTER(C.c_int16))()
    n, sr, ch, bits = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if f32:
        rc = L.sd_read_wav_f32(path.encode(), C.byref(p), C.byref(n), C.byref(sr), C.byref(ch), C.byref(bits))
    else:
        rc = L.sd_read_wav(path.encode(), C.byref(p), C.byref(n), C.byref(sr), C.byref(ch))
    if rc:
        return None
    total = n.value * max(ch.value, 1)
    arr = np.ctypeslib.as_array(p, shape=(max(total, 1),))[:total].copy()
    (L.sd_free_wav if f32 else L.sd_free_pcm)(p)
    return arr, n.value, sr.value, ch.value


def rule(path, flags):
    """the loading rule over the library's two readers: (kind, n, sr, bytes of the samples delivered)"""
    r = lib_read(path, False)
    if r is not None:
        pcm, n, sr, ch = r
        if (sr == 16000 or flags & ASSUME_16K) and not (ch > 1 and flags & DOWNMIX):
            return PCM16, n, sr, pcm[:n].tobytes()
    r = lib_read(path, True)
    if r is None:
        return UNREADABLE, None, None, None
    w, n, sr, ch = r
    if ch > 1 and flags & DOWNMIX:
        s = np.zeros(n, np.float32)
        for q in range(ch):                      # s += wav[i * ch + q] in float, channel after channel; then s / ch
            s = s + w.reshape(n, ch)[:, q]
        w = s / np.float32(ch)
    if sr == 16000 or flags & ASSUME_16K:
        return F32, n, sr, w[:n].tobytes()
    if not flags & RESAMPLE:
        return OFF_RATE, None, sr, None
    if n <= 0:
        return NO_SAMPLES, None, sr, None
    return F32_OFF_RATE, n, sr, w[:n].tobytes()


def test_reader_and_loading_rule_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "wav_file_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_wav_file.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
    paths = {}
    for name, (data, _) in FILES.items():
        paths[name] = str(tmp_path / (name + ".wav"))
        with open(paths[name], "wb") as f:
            f.write(data)
    out = subprocess.run([exe] + list(paths.values()) + [str(tmp_path / "absent.wav")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.endswith("wav_file ok\n"), (out.stdout[-300:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    got = {}
    for line in out.stdout.splitlines()[:-1]:
        path, what, rest = line.split(" ", 2)
        fields = dict(kv.split("=") for kv in rest.split(" ") if "=" in kv and not kv.startswith("--"))
        key = (path, what) if what != "load" else (path, what, int(fields["flags"]))
        got[key] = (fields, rest)
    assert len(got) == (len(FILES) + 1) * (2 + len(FLAG_SETS))
    tail = lambda rest: b"" if rest.split(" ")[-1] == "-" else bytes.fromhex(rest.split(" ")[-1])
    for name, (_, n_want) in FILES.items():
        p = paths[name]
        # the two readers: what the library's entries give, and the counts the file was written for
        for what, f32 in (("pcm16", False), ("f32", True)):
            fields, rest = got[(p, what)]
            r = lib_read(p, f32)
            print(name, what, rest[:60])
            if r is None:
                assert int(fields["rc"]) != 0, (name, what)
                continue
            arr, n, sr, ch = r
            assert (int(fields["rc"]), int(fields["n"]), int(fields["sr"]), int(fields["ch"])) == (0, n, sr, ch), (name, what)
            assert tail(rest) == arr.tobytes(), (name, what)
            assert n == n_want, (name, what)
            assert np.array_equal((sdhip.read_wav_f32(p) if f32 else sdhip.read_wav(p))[0], arr[:n]), (name, what)
        if n_want is None:
            assert lib_read(p, True) is None and lib_read(p, False) is None, name
        if name in WELL_FORMED:
            w_ref, sr_ref, ch_ref, bits_ref = orc.read_wav(p)              # the oracle's restatement of wav.h:62-126, as test_next_rows.py compares
            fields, rest = got[(p, "f32")]
            assert (int(fields["n"]), int(fields["sr"]), int(fields["ch"]), int(fields["bits"])) == (len(w_ref), sr_ref, ch_ref, bits_ref), name
            assert tail(rest)[:4 * len(w_ref)] == w_ref.tobytes(), name
        # the loader under every flag set: the rule over the library's readers
        for flags in FLAG_SETS:
            fields, rest = got[(p, "load", flags)]
            kind, n, sr, data = rule(p, flags)
            assert int(fields["kind"]) == kind, (name, flags, rest[:80])
            if data is not None:
                assert (int(fields["n"]), int(fields["sr"])) == (n, sr) and tail(rest) == data, (name, flags)
            if kind == OFF_RATE:
                assert all(w in rest for w in (str(sr), "16000", "--resample", "SD_WAV_RESAMPLE", "--assume-16k", "SD_WAV_ASSUME_16K")), rest
    # what the rule means for the files it was written for
    kinds = lambda name: [int(got[(paths[name], "load", f)][0]["kind"]) for f in FLAG_SETS]
    assert kinds("mono16") == [PCM16] * 5 and kinds("mono8") == [F32] * 5 and kinds("mono32") == [F32] * 5
    assert kinds("stereo16") == [PCM16, PCM16, F32, PCM16, F32]
    assert kinds("mono44k") == [OFF_RATE, F32_OFF_RATE, OFF_RATE, PCM16, PCM16]
    assert kinds("empty44k") == [OFF_RATE, NO_SAMPLES, OFF_RATE, PCM16, PCM16]
    for name in ("bits24", "len0", "len10", "len43", "fmt8", "fmt_huge", "chunk_past_end", "no_data"):
        assert kinds(name) == [UNREADABLE] * 5, name
    assert all(int(got[(str(tmp_path / "absent.wav"), "load", f)][0]["kind"]) == UNREADABLE for f in FLAG_SETS)
    st = np.frombuffer(tail(got[(paths["stereo16"], "load", DOWNMIX)][1]), np.float32)
    assert np.array_equal(st, ((S[0::2] + S[1::2]) / 65536.0).astype(np.float32))      # sums of two 16-bit samples / 32768 and their halves are exact in float
