"""CPU tests of the rule of sd_diarize_many_audio* (include/sdhip.h): the library's host-only entries against tests/ingest_ref.py, the reference
against wav_load's own downmix loop, and the proof that the reference is sharp -- every planted mistake of ingest_ref.MISTAKES changes a byte of the
case ingest_cases.SHOWN_BY names for it."""
import struct

import numpy as np
import pytest

import ingest_cases as IC
import ingest_ref as G
import sdhip
from oracle import resample_oracle as ro


@pytest.mark.parametrize("enc", [G.ENC_MULAW, G.ENC_ALAW])
def test_g711_decode_is_the_reference_table_over_all_codes(enc):
    got = sdhip.g711_decode(enc, np.arange(256, dtype=np.uint8))
    ref = G.mulaw_table() if enc == G.ENC_MULAW else G.alaw_table()
    assert got.dtype == np.int16 and np.array_equal(got.astype(np.int32), ref)
    assert len(sdhip.g711_decode(enc, np.zeros(0, np.uint8))) == 0


def test_g711_decode_pinned_itu_values_and_refusals():
    mu = sdhip.g711_decode(G.ENC_MULAW, [0xFF, 0x80, 0x00, 0x7F])
    assert list(mu) == [0, 32124, -32124, 0]
    al = sdhip.g711_decode(G.ENC_ALAW, [0xD5, 0x55, 0xAA, 0x2A])
    assert list(al) == [8, -8, 32256, -32256]
    for enc in (G.ENC_S16, G.ENC_F32, 4, -1):
        with pytest.raises(sdhip.SdError):
            sdhip.g711_decode(enc, [0])


def test_both_laws_are_odd_symmetric_but_for_mulaws_two_zeros():
    mu, al = G.mulaw_table(), G.alaw_table()
    c = np.arange(128)
    assert np.array_equal(mu[c], -mu[c | 0x80])                       # bit 7 is the sign; 0x7F and 0xFF are -0 and +0
    assert mu[0x7F] == 0 and mu[0xFF] == 0 and (mu[np.arange(256) & 0x7F != 0x7F] != 0).all()
    assert np.array_equal(al[c | 0x80], -al[c]) and (al != 0).all()
    assert np.abs(mu).max() == 32124 and np.abs(al).max() == 32256 and np.abs(al).min() == 8
    assert abs(int(mu[G.GUARD_CODE[G.ENC_MULAW]])) == 32124 and abs(int(al[G.GUARD_CODE[G.ENC_ALAW]])) == 32256
    assert len(set(np.abs(mu))) == 128 and len(set(np.abs(al))) == 128


def test_audio_len16_against_sd_resample_len():
    L = sdhip.lib()
    for sr in (8000, 11025, 16000, 22050, 32000, 44100, 48000, 16001, 1):
        for n in (0, 1, 2, 7999, 8000, 80001, 12345678):
            a = sdhip.Audio(0, sr, G.ENC_MULAW, 2, 1, n=n)
            want = n if sr == 16000 else L.sd_resample_len(n, sr, 16000)
            assert sdhip.audio_len16(a) == want == G.len16(n, sr), (sr, n)
    ok = dict(sample_rate=8000, encoding=G.ENC_S16, channels=2, channel=-1, n=10)
    assert sdhip.audio_len16(sdhip.Audio(0, **ok)) == ro.out_len(10, 8000, 16000)
    for bad in (dict(n=-1), dict(sample_rate=0), dict(sample_rate=-8000), dict(encoding=4), dict(encoding=-1), dict(channels=0), dict(channel=2), dict(channel=-2),
                dict(n=(1 << 40) + 1)):
        assert sdhip.audio_len16(sdhip.Audio(0, **dict(ok, **bad))) == -1, bad


def write_pcm16(path, pcm, sr, channels):
    data = np.ascontiguousarray(pcm, np.int16).tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, sr, sr * 2 * channels, 2 * channels, 16)
    open(path, "wb").write(hdr + b"data" + struct.pack("<I", len(data)) + data)


@pytest.mark.parametrize("channels", [2, 3])
def test_downmix_reference_is_wav_loads_own_loop(tmp_path, channels):
    """wav_load's downmix loop (csrc/wav_file.h), restated here on the floats sd_read_wav_f32 returns, equals the reference's channel rule on the int16
    elements: the 16-bit decode of the reader equals pcm_to_float exactly"""
    rng = np.random.default_rng(channels)
    n = 4001
    pcm = rng.integers(-32768, 32768, n * channels).astype(np.int16)
    pcm[:channels] = (-32768, 32767, 1)[:channels]
    p = str(tmp_path / "c.wav")
    write_pcm16(p, pcm, 16000, channels)
    w, sr, ch, bits = sdhip.read_wav_f32(p)
    assert (sr, ch, bits, len(w)) == (16000, channels, 16, n)
    # read_wav_f32 hands back the reference's "first n interleaved samples"; wav_load sums over the whole buffer, so the same samples are read again
    # as a mono file: these floats are the reader's own 16-bit decode
    write_pcm16(p, pcm, 16000, 1)
    full = sdhip.read_wav_f32(p)[0]
    assert len(full) == n * channels and np.array_equal(full[:n], w)
    assert full.tobytes() == G.decode(pcm, G.ENC_S16).tobytes()
    s = np.zeros(n, np.float32)
    for q in range(channels):
        s = (s + full[q::channels]).astype(np.float32)
    loop = (s / np.float32(channels)).astype(np.float32)
    assert G.frames(pcm, G.ENC_S16, channels, -1, n).tobytes() == loop.tobytes()
    for c in range(channels):
        assert G.frames(pcm, G.ENC_S16, channels, c, n).tobytes() == full[c::channels].tobytes()


@pytest.mark.parametrize("name", IC.CASES)
def test_cases_are_well_formed_and_accepted_by_the_no_subnormal_guard(name):
    """every case computes on the CPU table (input_ref's guard asserts inside), leaves its canaries, and holds no NaN"""
    rows, src, dst_len = IC.case(name)
    exp = IC.expected(name)
    assert len(exp) == dst_len + IC.SLACK and not np.isnan(exp).any()
    assert (exp[dst_len:] == IC.FCANARY).all() and (exp[:3] == IC.FCANARY).all()
    assert (rows[:, 7] >= 1).all() and all(G.len16(int(r[4]), int(r[3])) <= r[7] for r in rows)      # what the hook asks of a row
    iv = sorted((int(r[6]), int(r[6] + r[7])) for r in rows)
    assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:])) and iv[-1][1] <= dst_len


def test_the_named_shapes_are_among_the_cases():
    rows = IC.case("mixed9")[0]
    assert len(rows) == 10 and (rows[:, 4] == 0).sum() == 2 and rows[-1][7] == 512            # nine rows and the pad row; a row with n = 0
    extra = [int(r[7]) - G.len16(int(r[4]), int(r[3])) for r in rows[:9]]
    assert min(extra) == 1 and max(extra) == 80000
    assert any(r[6] % 4 != 0 and G.len16(int(r[4]), int(r[3])) >= 512 for r in rows[:9])      # a full tile on an unaligned base
    for e in (G.ENC_MULAW, G.ENC_ALAW):
        rows, src, _ = IC.case("direct_%s" % IC.ENC_NAMES[e])
        assert np.array_equal(src[rows[0][5]:rows[0][5] + 256], np.arange(256, dtype=np.uint8))
    for name in IC.DIRECT:
        rows = IC.case(name)[0]
        assert {int(r[6]) % 4 for r in rows} == {0, 1, 2, 3} and {1, 255, 256, 257, 773} <= {int(r[4]) for r in rows}
        assert {(int(r[1]), int(r[2])) for r in rows} == set(IC.CHANNEL_FORMS)
    for sr in IC.OFF_RATES:
        rows = IC.case("rate_%d" % sr)[0]
        J = IC.R.plan(sr)[2]
        # a whole recording has sd_resample_len outputs: above 16 kHz every count is some recording's, below it the nearest one at or above it
        # (at 8 000 Hz the length is 2 n: 2, 256, 258 and 774 stand for the odd counts)
        want = {1, 255, 256, 257, 773} if sr > 16000 else {G.len16(IC.K.n_for(sr, no), sr) for no in (1, 255, 256, 257, 773)}
        assert want <= {G.len16(int(r[4]), sr) for r in rows} and 256 in want and {1, 2, J, J + 1} <= {int(r[4]) for r in rows}
        assert {int(r[0]) for r in rows} == set(IC.ENCS)


@pytest.mark.parametrize("mistake", G.MISTAKES)
def test_every_planted_mistake_changes_a_byte_of_its_case(mistake):
    name = IC.SHOWN_BY[mistake]
    good, bad = IC.expected(name), IC.expected(name, mistake=mistake)
    assert good.tobytes() != bad.tobytes(), (mistake, name)
    assert set(IC.SHOWN_BY) == set(G.MISTAKES)
