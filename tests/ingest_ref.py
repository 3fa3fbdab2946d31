"""Plain numpy reference of the rule of sd_diarize_many_audio* (include/sdhip.h, "recordings in their own rate and encoding") and of k_many_ingest
(csrc/ingest.hip), for tests/test_ingest_ref.py (CPU), tests/test_ingest_kernel.py and tests/test_many_audio.py (GPU).

  decode        the G.711 tables from ITU-T's formulas as the header states them, int16 * 2^-15, float as it is
  channel rule  one channel, or the mean: s = +0.0f, s += x_q in channel order in float32, s / float32(channels) -- numpy's float32 division is
                correctly rounded
  rate          at 16 kHz the frames; else tests/input_ref.py's resample_exact (imported, not copied) on a tap table it is given
  the pack      dst[base, base + len16) = y, zeros up to base + len, nothing else touched

`mistake` (default None) plants ONE of MISTAKES: tests/test_ingest_ref.py shows that each changes a byte of a named case of tests/ingest_cases.py."""
import numpy as np

import input_ref as R
from oracle import resample_oracle as ro

SLACK = R.SLACK
ENC_S16, ENC_F32, ENC_MULAW, ENC_ALAW = 0, 1, 2, 3
DTYPES = {ENC_S16: np.int16, ENC_F32: np.float32, ENC_MULAW: np.uint8, ENC_ALAW: np.uint8}
GUARD_CODE = {ENC_MULAW: 0x80, ENC_ALAW: 0xAA}      # the code of each law's largest magnitude: what the hook puts behind a G.711 source

MISTAKES = ("mulaw_bias_forgotten", "alaw_e0_branch", "sign_flipped", "channel_stride", "mean_f64", "reciprocal_multiply", "zeros_missing", "last_input_readable")


def mulaw_table(mistake=None):
    """int32 [256]: with u = ~code, t = (((u & 15) << 3) + 132) << ((u >> 4) & 7), s = t - 132, negative when u & 0x80"""
    u = ~np.arange(256, dtype=np.int64) & 0xFF
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    s = t if mistake == "mulaw_bias_forgotten" else t - 132
    neg = (u & 0x80) != 0
    if mistake == "sign_flipped":
        neg = ~neg
    return np.where(neg, -s, s).astype(np.int32)


def alaw_table(mistake=None):
    """int32 [256]: with a = code ^ 0x55, e = (a >> 4) & 7, m = a & 15, s = e ? ((m << 4) + 264) << (e - 1) : (m << 4) + 8, positive when a & 0x80"""
    a = np.arange(256, dtype=np.int64) ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    big = ((m << 4) + 264) << np.maximum(e - 1, 0)
    small = (m << 4) + 8
    s = np.where(e > 0, big, ((m << 4) + 264) >> 1 if mistake == "alaw_e0_branch" else small)
    pos = (a & 0x80) != 0
    if mistake == "sign_flipped":
        pos = ~pos
    return np.where(pos, s, -s).astype(np.int32)


def decode(elems, enc, mistake=None):
    """step 1: the elements of a source -> float32"""
    if enc == ENC_F32:
        return np.asarray(elems, np.float32)
    if enc == ENC_S16:
        v = np.asarray(elems, np.int16).astype(np.int32)
    else:
        v = (mulaw_table(mistake) if enc == ENC_MULAW else alaw_table(mistake))[np.asarray(elems, np.uint8)]
    return (v.astype(np.float64) * 2.0 ** -15).astype(np.float32)      # exact


def frames(elems, enc, channels, channel, n, mistake=None):
    """steps 1 and 2: n frames of `channels` interleaved elements -> float32 [n]"""
    x = decode(elems, enc, mistake)
    if mistake == "channel_stride":
        idx = np.arange(n, dtype=np.int64) * max(channels - 1, 1)      # a stride of channels - 1
    else:
        idx = np.arange(n, dtype=np.int64) * channels
    if channel >= 0:
        return x[np.minimum(idx + channel, len(x) - 1)] if n else np.zeros(0, np.float32)
    if mistake == "mean_f64":
        return np.stack([x[np.minimum(idx + q, len(x) - 1)] for q in range(channels)]).astype(np.float64).mean(0).astype(np.float32)
    s = np.zeros(n, np.float32)
    for q in range(channels):
        s = (s + x[np.minimum(idx + q, len(x) - 1)]).astype(np.float32)
    if mistake == "reciprocal_multiply":
        return (s * (np.float32(1.0) / np.float32(channels))).astype(np.float32)
    return (s / np.float32(channels)).astype(np.float32)


def len16(n, sr):
    return n if sr == 16000 else ro.out_len(n, sr, 16000)


def samples16(elems, enc, channels, channel, sr, n, taps=None, mistake=None):
    """the whole rule: y [len16] float32.  taps: the table of sr -> 16 000 Hz (unused at 16 kHz)"""
    x = frames(elems, enc, channels, channel, n, mistake)
    if sr == 16000:
        return x
    L, M, J = R.plan(sr)
    no = len16(n, sr)
    if mistake == "last_input_readable":
        # the element behind the last frame is the hook's guard: NaN for floats, 0x7fff for int16, the law's largest for G.711
        g = {ENC_S16: np.float32(32767.0 / 32768.0), ENC_F32: np.float32(np.nan)}.get(enc)
        if g is None:
            g = decode(np.array([GUARD_CODE[enc]], np.uint8), enc)[0]
        return R.resample_exact(np.concatenate([x, [g]]).astype(np.float32), 0, n + 1, 0, no, taps, L, M, J)
    return R.resample_exact(x, 0, n, 0, no, taps, L, M, J)


def ingest_ref(rows, src, tables, dst_len, canary, mistake=None):
    """k_many_ingest on rows as Diarizer.many_ingest_case takes them -- (encoding, channels, channel, sample_rate, n, src_off in bytes or -1, base, len) --
    and the bytes of all sources; tables: sample_rate -> the tap table -> [dst_len + SLACK] float32"""
    src = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
    out = np.full(dst_len + SLACK, canary, np.float32)
    for enc, channels, channel, sr, n, so, base, ln in np.asarray(rows, np.int64).reshape(-1, 8):
        enc, channels, channel, sr, n = int(enc), int(channels), int(channel), int(sr), int(n)
        es = np.dtype(DTYPES[enc]).itemsize
        elems = src[so:so + n * channels * es].view(DTYPES[enc]) if n > 0 else np.zeros(0, DTYPES[enc])
        y = samples16(elems, enc, channels, channel, sr, n, tables.get(sr), mistake)
        assert len(y) <= ln
        out[base:base + len(y)] = y
        if mistake != "zeros_missing":
            out[base + len(y):base + ln] = 0.0
    return out
