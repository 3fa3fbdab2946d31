"""Reference of the "streams at any sample rate" rule (include/sdhip.h; csrc/resample_book.h) in plain Python integers, shared by
tests/test_stream_rate_cpu.py and tests/test_stream_rate.py.  The plan of a rate pair and the float length rule are oracle/resample_oracle.py's."""
import numpy as np

from oracle import resample_oracle as ro

RATES = (8000, 11025, 22050, 32000, 44100, 48000, 12345)


def plan(in_sr, out_sr=16000):
    """(L, M, J) of the rate pair"""
    L, M, _, _, J = ro.plan(in_sr, out_sr)
    return L, M, J


def out_len(n, in_sr, out_sr=16000):
    return ro.out_len(n, in_sr, out_sr)


def final_len(n, in_sr, out_sr=16000):
    """F(n) = min(len(n), n - 1 - J < 0 ? 0 : ((n - J) L - 1) / M + 1): the outputs of n inputs that no later input can change"""
    L, M, J = plan(in_sr, out_sr)
    by_reads = 0 if n - 1 - J < 0 else ((n - J) * L - 1) // M + 1
    return min(out_len(n, in_sr, out_sr), by_reads)


def final_len_brute(n, in_sr, out_sr=16000):
    """the definition: count the outputs m of len(n) whose last read, input floor(m M / L) + J, lies in front of n (the reads rise with m)"""
    L, M, J = plan(in_sr, out_sr)
    m = 0
    while m < out_len(n, in_sr, out_sr) and (m * M) // L + J <= n - 1:
        m += 1
    return m


def noise(n, seed):
    """n float32 samples of uniform noise in [-0.5, 0.5) that are also exact int16 / 32768 values (read-only)"""
    pcm = np.random.default_rng(seed).integers(-16384, 16384, n).astype(np.int16)
    x = pcm.astype(np.float32) / np.float32(32768.0)
    pcm.setflags(write=False)
    x.setflags(write=False)
    return pcm, x
