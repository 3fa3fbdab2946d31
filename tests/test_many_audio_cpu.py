"""CPU tests of the host side of sd_diarize_many_audio*: sd_read_wav_audio (csrc/wav_file.h: wav_read_audio) on files written here -- it returns the
file's own bytes and a descriptor as written, or refuses -- and the planner (csrc/ingest_plan.h) and the reader as a stand-alone program under
AddressSanitizer + UBSan (tools/sanitize/ingest_main.cpp, built by tools/sanitize/build_ingest.sh) on random descriptor lists, the size limits, and
truncated and corrupted headers.  Nothing is loaded into python under a sanitizer."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ingest_ref as G
import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD_ERR_ARG = 1


def wav_bytes(tag, bits, channels, sr, data, fmt_extra=b"", chunks_before_data=b"", announced=None):
    data = bytes(data)
    fmt = struct.pack("<HHIIHH", tag, channels, sr, sr * channels * bits // 8, channels * bits // 8, bits) + fmt_extra
    body = b"WAVEfmt " + struct.pack("<I", len(fmt)) + fmt + chunks_before_data + b"data" + struct.pack("<I", len(data) if announced is None else announced) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def payload(enc, n, channels, seed):
    rng = np.random.default_rng(seed)
    if enc == G.ENC_S16:
        return rng.integers(-32768, 32768, n * channels).astype(np.int16)
    return rng.integers(0, 256, n * channels).astype(np.uint8)


FORMS = {G.ENC_S16: (1, 16), G.ENC_MULAW: (7, 8), G.ENC_ALAW: (6, 8)}
LIST = b"LIST" + struct.pack("<I", 10) + b"INFOabcdef"


def files(tmp_path):
    """name -> (path, expected (elements, sr, enc, channels) or None for a refusal)"""
    out, k = {}, 0

    def add(name, blob, want):
        nonlocal k
        p = tmp_path / (name + ".wav")
        p.write_bytes(blob)
        out[name] = (str(p), want)
        k += 1

    for enc, (tag, bits) in FORMS.items():
        for channels, sr, n in ((1, 8000, 1001), (2, 8000, 640), (3, 11025, 333), (5, 48000, 77), (1, 16000, 0)):
            el = payload(enc, n, channels, k)
            add("tag%d_c%d_%d" % (tag, channels, sr), wav_bytes(tag, bits, channels, sr, el.tobytes()), (el, sr, enc, channels))
        el = payload(enc, 500, 2, 100 + k)
        add("tag%d_long_fmt" % tag, wav_bytes(tag, bits, 2, 8000, el.tobytes(), fmt_extra=b"\x00\x00"), (el, 8000, enc, 2))      # the 18-byte fmt chunk G.711 writers leave
        add("tag%d_list" % tag, wav_bytes(tag, bits, 2, 8000, el.tobytes(), chunks_before_data=LIST), (el, 8000, enc, 2))
        add("tag%d_long_fmt_list" % tag, wav_bytes(tag, bits, 2, 8000, el.tobytes(), fmt_extra=b"\x00\x00", chunks_before_data=LIST), (el, 8000, enc, 2))
        add("tag%d_streamed" % tag, wav_bytes(tag, bits, 2, 8000, el.tobytes(), announced=0xFFFFFFFF), (el, 8000, enc, 2))
        odd = el.tobytes()[:-1]                                                                                               # a torn last frame: whole frames only
        keep = len(odd) // (2 * bits // 8) * 2
        add("tag%d_torn" % tag, wav_bytes(tag, bits, 2, 8000, odd), (el[:keep], 8000, enc, 2))
        add("tag%d_announced_beyond" % tag, wav_bytes(tag, bits, 2, 8000, el.tobytes(), announced=len(el.tobytes()) + 4000), (el, 8000, enc, 2))
    f = np.linspace(-1, 1, 100).astype(np.float32)
    add("tag3_float", wav_bytes(3, 32, 1, 16000, f.tobytes()), None)
    add("tag1_8bit", wav_bytes(1, 8, 1, 16000, bytes(range(200))), None)
    add("tag1_32bit", wav_bytes(1, 32, 1, 16000, f.tobytes()), None)
    add("tag7_16bit", wav_bytes(7, 16, 1, 8000, bytes(200)), None)
    add("tag6_channels0", wav_bytes(6, 8, 0, 8000, bytes(200)), None)
    add("tag7_rate0", wav_bytes(7, 8, 1, 0, bytes(200)), None)
    add("extensible", wav_bytes(0xFFFE, 16, 2, 48000, bytes(400), fmt_extra=bytes(24)), None)
    good = wav_bytes(7, 8, 1, 8000, bytes(300), chunks_before_data=LIST)
    for cut in (0, 3, 12, 21, 22, 30, 43, 44, 50, 61):
        # cut inside the RIFF / fmt header, inside LIST, inside the data chunk's header; 62 bytes are the headers of this file
        add("cut%d" % cut, good[:cut], None)
    bad = bytearray(good)
    bad[16:20] = struct.pack("<I", 8)
    add("fmt_size_8", bytes(bad), None)
    bad = bytearray(good)
    bad[16:20] = struct.pack("<I", 0x7FFFFFF0)
    add("fmt_size_huge", bytes(bad), None)
    bad = bytearray(good)
    bad[40:44] = struct.pack("<I", 0x7FFFFF00)                                                                                # the LIST chunk claims two gigabytes
    add("list_size_huge", bytes(bad), None)
    return out


def test_read_wav_audio_returns_bytes_and_descriptor_as_written_or_refuses(tmp_path):
    fs = files(tmp_path)
    assert sum(1 for _, w in fs.values() if w is None) >= 20
    for name, (path, want) in fs.items():
        if want is None:
            with pytest.raises(sdhip.SdError) as e:
                sdhip.read_wav_audio(path)
            assert e.value.code == SD_ERR_ARG, name
            continue
        el, sr, enc, channels = want
        a = sdhip.read_wav_audio(path)
        assert (a.sample_rate, a.encoding, a.channels, a.channel, a.n) == (sr, enc, channels, 0, len(el) // channels), name
        assert a.data.dtype == el.dtype and a.data.tobytes() == el.tobytes(), name
        assert sdhip.audio_len16(a) == G.len16(a.n, sr), name
    with pytest.raises(sdhip.SdError):
        sdhip.read_wav_audio(str(tmp_path / "absent.wav"))


def test_existing_readers_still_read_g711_files_as_before(tmp_path):
    """out of scope and unchanged: sd_read_wav_f32 never looked at the format tag and reads a tag-7 file's bytes as signed chars"""
    fs = files(tmp_path)
    path, (el, sr, enc, channels) = fs["tag7_c1_8000"]
    w, sr2, ch2, bits = sdhip.read_wav_f32(path)
    assert (sr2, ch2, bits) == (8000, 1, 8) and np.array_equal(w, el.view(np.int8).astype(np.float32) / np.float32(32768.0))


def test_planner_and_reader_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "ingest_asan")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_ingest.sh"), exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
    fs = files(tmp_path)
    names = list(fs)
    out = subprocess.run([exe] + [fs[k][0] for k in names] + [str(tmp_path / "absent.wav")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.endswith("ingest ok\n"), (out.stdout[-600:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr and "BAD" not in out.stdout, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    # the reader: the program's lines against what was written
    for k, line in zip(names, lines):
        path, want = fs[k]
        assert line.startswith(path + " audio rc="), line[:200]
        if want is None:
            assert line == path + " audio rc=1 n=0 sr=0 enc=0 ch=0 channel=0 -", k
        else:
            el, sr, enc, channels = want
            assert line == "%s audio rc=0 n=%d sr=%d enc=%d ch=%d channel=0 %s" % (path, len(el) // channels, sr, enc, channels, el.tobytes().hex() or "-"), k
    # the planner: 200 random rounds, accepted and refused ones among them, and the limits
    rounds = [l for l in lines if l.startswith("round ")]
    assert len(rounds) == 200 and sum("refusal" in l for l in rounds) >= 20 and sum("recordings," in l for l in rounds) >= 100
    limits = dict(l[6:].rsplit(" -> ", 1) for l in lines if l.startswith("limit "))
    ok, bad_desc, null_data, rate_table, byte_limit, pack = "0 bad=-1", "1 bad=0", "2 bad=1", "3 bad=0", "5 bad=0", "6 bad=-1"
    assert limits == {"null list": pack, "R = 0": pack, "R = 2^20 + 1": pack, "n = 2^40 at 16 kHz": pack, "n = 2^40 + 1": bad_desc,
                      "n = 2^40 at 1 Hz": "6 bad=0", "n = 2^40 at 2^31 - 1 Hz": rate_table, "n = 2^40 of 2^31 - 1 float channels": byte_limit,
                      "n = 2^40 int16 stereo": pack, "null data": null_data, "null data, n = 0": ok, "SD_MANY_MAX_CHUNKS": ok,
                      "SD_MANY_MAX_CHUNKS + 1 slot": pack, "2^20 recordings of 2^40 samples": pack}


def test_the_hook_has_a_header_of_its_own_and_the_interface_is_mirrored():
    """include/sdhip_ingest_test.h declares the one hook (tests/test_abi.py pins sdhip_test.h's list name by name); the five public entries are in EXPORTS"""
    import re
    L = sdhip.lib()
    hook = set(re.findall(r"^int (sd_[a-z0-9_]+)\(", open(os.path.join(ROOT, "include", "sdhip_ingest_test.h")).read(), re.M))
    assert hook == set(sdhip.INGEST_TEST_EXPORTS) == {"sd_test_many_ingest"} and hasattr(L, "sd_test_many_ingest")
    assert "sd_test_many_ingest" not in open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    for name in ("sd_audio_len16", "sd_g711_decode", "sd_read_wav_audio", "sd_diarize_many_audio", "sd_diarize_many_audio_dev"):
        assert name in sdhip.EXPORTS and hasattr(L, name)
    assert (sdhip.ENC_S16, sdhip.ENC_F32, sdhip.ENC_MULAW, sdhip.ENC_ALAW) == (0, 1, 2, 3)
    assert C.sizeof(sdhip.AudioDesc) == 32
