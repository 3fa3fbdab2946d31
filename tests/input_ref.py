"""Plain numpy references of the kernels IN FRONT of the two networks -- the resampler (csrc/resample.hip), the copy kernels of the streams
(csrc/stream.hip), the pack and gap-mask kernels (csrc/many.hip) and the fp16 weight forms (csrc/weights_gpu.hip) -- one function per kernel, for
tests/test_input_kernels.py (GPU) and tests/test_input_ref.py (CPU).

The resampler has three references, from strict to independent:
  resample_exact   restates resample_point's arithmetic on a tap table it is GIVEN (the GPU test hands it the table the context built): j from -J to J
                   alternating between two float32 accumulators with fmaf, then acc0 + acc1.  numpy has no fmaf: fma32 below is one, pinned to the C
                   library's on the CPU.  Its results are the kernel's bytes.
  tap_table_ref    oracle/resample_oracle.h in float64: the table must be its float32 rounding to half an ulp, and zero outside the window.
  oracle_bound     resample_oracle.resample in float64 with a derived bound: a mistake that kernel and restatement share still has to pass it.
The copy, pack and mask references are slicing; the weight forms are numpy's round-to-nearest-even conversions and the layout formula of k_w16x.

`mistake` (default None) plants ONE of MISTAKES in a function: tests/test_input_ref.py shows that each of them changes a byte of a case of
tests/input_cases.py, makes a result non-finite, or touches a canary.  Two notes on what a planted mistake can mean.  "last_tap_dropped": row j = +J of
the product's table is zero BY CONSTRUCTION (J = floor(half / L) + 1, so J L > half), and dropping a tap that is +0.0 is no change of the function at
all; the case that shows this mistake runs the reference on a table of random numbers.  "src_cut": a kernel that cut its groups of four at the 16-byte
boundaries of the SOURCE would store 16 bytes at places that are not 16-byte aligned; the reference models such a store as landing on the aligned
address below it."""
import ctypes
import ctypes.util

import numpy as np

from oracle import resample_oracle as ro

SLACK = 256
TAIL_PAD = 512                                   # SD_TAIL_PAD
FRAMES, SPEAKERS = 293, 3
TINY = 2.0 ** -126                               # the smallest normal float32

MISTAKES = ("first_tap_dropped", "last_tap_dropped", "one_accumulator", "rounded_product", "phase_off_by_one", "i0_rounded_up", "n_limit_ignored",
            "rs_pad_short",
            "pad_short", "room_ignored", "src_cut", "div_32767", "len_unclamped", "gap_unclamped",
            "truncated", "residue_unscaled", "pad_in_max", "exponent_off_by_one")


# ---------------------------------------------------------------- fmaf
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma32(a, b, c, naive=False):
    """float32(a * b + c) with ONE rounding, elementwise on float32 arrays.  The product of two float32 is exact in float64; its sum with c is not
    always, and rounding that float64 sum to float32 rounds twice.  The two roundings differ from one exactly where the float64 sum sits on the midpoint
    of two neighbouring float32 and the part the first rounding dropped (TwoSum's error term) is not zero: then the neighbour on the error's side is
    the answer, not the even one.  naive = True skips the correction ("compute in float64, then round").  No float32 subnormals: callers see to that."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        s, e = two_sum(p, c.astype(np.float64))
        r = s.astype(np.float32)
        if naive:
            return r
        d = s - r.astype(np.float64)
        toward = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.isfinite(s) & (d != 0) & (e != 0) & (toward.astype(np.float64) - s == d)
        return np.where(tie & (np.sign(e) == np.sign(d)), toward, r).astype(np.float32)


_libm = None


def c_fmaf(a, b, c):
    """fmaf of the C library, element by element"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fmaf.restype = ctypes.c_float
        _libm.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)


# ---------------------------------------------------------------- resample.hip
def plan(in_sr, out_sr=16000):
    """(L, M, J) of a rate pair (resample_book.h: make_plan)"""
    L, M, fc, half, J = ro.plan(in_sr, out_sr)
    return L, M, J


def tap_table_ref(in_sr, out_sr=16000):
    """-> (h64 [2J + 1][L] float64 of oracle/resample_oracle.h, inside [2J + 1][L] bool: |u| <= half)"""
    L, M, fc, half, J = ro.plan(in_sr, out_sr)
    u = np.arange(L, dtype=np.float64)[None, :] + (np.arange(2 * J + 1, dtype=np.float64)[:, None] - J) * L
    return ro.h(u, L, fc, half), np.abs(u) <= half


def _no_subnormal(what, v):
    v = np.abs(np.asarray(v, np.float64))
    assert not ((v != 0) & (v < TINY)).any(), "%s: a non-zero value below 2^-126: flush-to-zero would be what the test measures" % what


def resample_exact(x, first, n_limit, m_first, count, taps, L, M, J, mistake=None):
    """resample_point for outputs [m_first, m_first + count): x[0] is input `first`, inputs in front of 0 and from n_limit on are zero -> float32 [count].
    Asserts that no product and no partial sum is a non-zero number below 2^-126."""
    x = np.asarray(x, np.float32)
    taps = np.asarray(taps, np.float32).reshape(2 * J + 1, L)
    m = m_first + np.arange(count, dtype=np.int64)
    t = m * M
    i0 = -((-t) // L) if mistake == "i0_rounded_up" else t // L
    ph = t - (t // L) * L
    if mistake == "phase_off_by_one":
        ph = (ph + 1) % L
    acc = [np.zeros(count, np.float32), np.zeros(count, np.float32)]
    held = len(x)
    for j in range(-J, J + 1):
        if (mistake == "first_tap_dropped" and j == -J) or (mistake == "last_tap_dropped" and j == J):
            continue
        g = i0 - j
        live = (g >= max(first, 0)) & (g < (first + held if mistake == "n_limit_ignored" else n_limit))
        assert first == 0 or (g >= first).all(), "a summed input in front of the inputs held"
        xv = np.where(live, x[np.clip(g - first, 0, max(held - 1, 0))] if held else np.float32(0), np.float32(0)).astype(np.float32)
        tp = taps[j + J, ph]
        k = 0 if mistake == "one_accumulator" else (j + J) & 1
        _no_subnormal("product", tp.astype(np.float64) * xv.astype(np.float64))
        if mistake == "rounded_product":
            acc[k] = ((tp * xv).astype(np.float32) + acc[k]).astype(np.float32)
        else:
            acc[k] = fma32(tp, xv, acc[k])
        _no_subnormal("partial sum", acc[k])
    y = fma32(acc[0], np.ones(count, np.float32), acc[1])
    _no_subnormal("sum", y)
    return y


def resample_ref(x, in_sr, n_out, taps, canary, mistake=None, out_sr=16000):
    """k_resample: outputs [0, n_out) of the whole recording x -> [n_out + SLACK] float32"""
    L, M, J = plan(in_sr, out_sr)
    x = np.asarray(x, np.float32)
    xs = np.concatenate([x, np.full(SLACK, np.nan, np.float32)]) if mistake == "n_limit_ignored" else x
    return np.concatenate([resample_exact(xs, 0, len(x), 0, n_out, taps, L, M, J, mistake), np.full(SLACK, canary, np.float32)])


def resample_jobs_ref(rows, x, tables, arena, canary, mistake=None):
    """rows as Diarizer.resample_jobs_case takes them; tables: in_sr -> the tap table -> the arena [arena + SLACK] float32"""
    out = np.full(arena + SLACK, canary, np.float32)
    for in_sr, pad, first, held, n_limit, m_first, count, x_off, dst_off in rows:
        L, M, J = plan(in_sr)
        xs = np.asarray(x[x_off:x_off + held], np.float32)
        if mistake == "n_limit_ignored":
            xs = np.concatenate([xs, np.full(SLACK, np.nan, np.float32)])      # what lies behind the inputs held
        y = resample_exact(xs, first, n_limit, m_first, count, tables[in_sr], L, M, J, mistake)
        out[dst_off:dst_off + count] = y
        p = pad - 1 if mistake == "rs_pad_short" and pad > 0 else pad
        out[dst_off + count:dst_off + count + p] = 0.0
    return out


def oracle_bound(x, in_sr, out_sr=16000):
    """-> (y64 of resample_oracle.resample, the bound (J + 4) 2^-24 sum_j |h_j x_j| per output).  The terms: the table's rounding (2^-24 per product), a
    chain of at most J + 1 fmaf per accumulator (2^-24 of a partial sum that the sum of magnitudes bounds, each), the last add, and the oracle's own
    64-bit roundings, which one more 2^-24 covers many times over."""
    x = np.asarray(x, np.float64)
    L, M, fc, half, J = ro.plan(in_sr, out_sr)
    y64 = ro.resample(x, in_sr, out_sr)
    no = len(y64)
    t = np.arange(no, dtype=np.int64) * M
    i0 = t // L
    ph = (t - i0 * L).astype(np.float64)
    xp = np.concatenate([np.zeros(J + 1), np.abs(x), np.zeros(J + 2 + max(0, int(i0.max(initial=0)) + 1 - len(x)))])
    mag = np.zeros(no)
    for j in range(-J, J + 1):
        mag += np.abs(ro.h(ph + j * L, L, fc, half)) * xp[i0 - j + J + 1]
    return y64, (J + 4) * 2.0 ** -24 * mag


def impulse_expected(n, in_sr, impulses, taps, n_out):
    """x = sum of amp * delta(k) over impulses (k, amp), amp a power of two, every two at least 2J + 2 apart: output m is amp * table[i0 - k + J][ph] of
    the one impulse with |i0 - k| <= J, or zero.  Leans on neither fma32 nor the oracle."""
    L, M, J = plan(in_sr)
    ks = sorted(k for k, _ in impulses)
    assert all(b - a >= 2 * J + 2 for a, b in zip(ks, ks[1:])) and 0 <= ks[0] and ks[-1] < n
    t = np.arange(n_out, dtype=np.int64) * M
    i0 = t // L
    ph = t - i0 * L
    y = np.zeros(n_out, np.float32)
    for k, amp in impulses:
        j = i0 - k
        hit = np.abs(j) <= J
        y[hit] = np.float32(amp) * np.asarray(taps, np.float32)[j[hit] + J, ph[hit]]
    return y


# ---------------------------------------------------------------- stream.hip
def to_f32(v, mistake=None):
    """the samples as the kernels hand them on: float32 copied, int16 / 32768 (exact)"""
    v = np.asarray(v)
    if v.dtype == np.float32:
        return v
    return (v.astype(np.float64) / (32767.0 if mistake == "div_32767" else 32768.0)).astype(np.float32)


def group_copy_ref(which, src, rows, dst_len, canary, mistake=None, dst_align=0):
    """k_group_append (0), k_group_scatter (1), k_group_tail_move (2), k_tail_move (3): dst[0, len) = src[0, len), `pad` zeros behind, nothing at or behind
    dst[room] (k_tail_move has no room) -> [dst_len + SLACK] float32.  dst_align / the source's element offsets matter to "src_cut" alone."""
    pad = 0 if which == 1 else TAIL_PAD
    if mistake == "pad_short" and pad:
        pad -= 1
    out = np.full(dst_len + SLACK, canary, np.float32)
    for so, do, ln, room in np.asarray(rows, np.int64).reshape(-1, 4):
        end = ln + pad if which == 3 or mistake == "room_ignored" else min(ln + pad, room)
        n = min(ln, end)
        vals = np.concatenate([to_f32(src[so:so + n], mistake), np.zeros(end - n, np.float32)])
        if mistake == "src_cut" and which != 3:
            head = min((-so) % 4, end)                      # groups of four from the source's boundary on, each stored at the aligned address below
            for i in range(head, end - 3, 4):
                at = do + i - (do + i + dst_align) % 4
                out[at:at + 4] = vals[i:i + 4]
            tail = head + (end - head) // 4 * 4
            out[do:do + head] = vals[:head]
            out[do + tail:do + end] = vals[tail:]
        else:
            hi = min(do + end, len(out))
            out[do:hi] = vals[:hi - do]
    return out


# ---------------------------------------------------------------- many.hip
def many_pack_ref(src, rows, dst_len, canary, mistake=None):
    """k_many_pack: dst[base, base + n) = src[0, n), zeros up to base + len, nothing at or behind dst_len -> [dst_len + SLACK] float32"""
    out = np.full(dst_len + SLACK, canary, np.float32)
    lim = len(out) if mistake == "len_unclamped" else dst_len
    for so, n, base, ln in np.asarray(rows, np.int64).reshape(-1, 4):
        end = max(min(base + ln, lim), base)
        k = min(n, end - base)
        if k > 0:
            out[base:base + k] = to_f32(src[so:so + k], mistake)
        out[base + max(k, 0):end] = 0.0
    return out


def gap_masks_ref(gaps, total_chunks, canary, mistake=None):
    """k_many_gap_masks: zero mask rows for chunks [first, first + count), nothing from total_chunks on -> [(total_chunks + SLACK) * 3][293] float32"""
    out = np.full((total_chunks + SLACK, SPEAKERS * FRAMES), canary, np.float32)
    lim = total_chunks + SLACK if mistake == "gap_unclamped" else total_chunks
    for first, cnt in np.asarray(gaps, np.int64).reshape(-1, 2):
        out[min(first, lim):min(first + cnt, lim)] = 0.0
    return out.reshape(-1, FRAMES)


# ---------------------------------------------------------------- weights_gpu.hip
def to_half(v, mistake=None):
    """float32 -> float16, round to nearest even ("truncated": toward zero)"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16)
        if mistake == "truncated":
            over = np.abs(h.astype(np.float32)) > np.abs(v)
            h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h


def w16_planes_ref(w, cin, canary, mistake=None):
    """k_w16_planes: [2][K][Cout][roundup64(cin)] fp16 bit patterns, the plane of float16(w) and the plane of float16(w - float32(hi)); pad channels zero"""
    w = np.asarray(w, np.float32)
    K, Cout, _ = w.shape
    pad16 = (cin + 63) // 64 * 64
    out = np.zeros((2, K, Cout, pad16), np.float16)
    v = w[:, :, :cin]
    hi = to_half(v, mistake)
    with np.errstate(over="ignore", invalid="ignore"):
        out[0, :, :, :cin] = hi
        out[1, :, :, :cin] = to_half(v - hi.astype(np.float32), mistake)
    return np.concatenate([out.reshape(-1).view(np.uint16), np.full(SLACK, canary, np.uint16)])


def w16x_ref(w, cin, canary, mistake=None):
    """k_w_absmax + k_w16x, restated: 2^e puts the largest finite |w| of the real channels into [2^13, 2^14); per 32-channel chunk of a row
    [hi 0..7 | lo 0..7 | hi 8..15 | ...] of float16(w 2^e) and float16(w 2^e - float32(hi)) -> (bit patterns + SLACK canaries, float32 2^-e)"""
    w = np.asarray(w, np.float32)
    K, Cout, CinPad = w.shape
    v = w if mistake == "pad_in_max" else w[:, :, :cin]
    fin = np.abs(v[np.isfinite(v)])
    wmax = np.float32(fin.max()) if fin.size else np.float32(0)
    e = 0
    if wmax > 0:
        e = 14 - int(np.frexp(wmax)[1]) + (1 if mistake == "exponent_off_by_one" else 0)
    sc = np.float32(np.ldexp(1.0, e))
    with np.errstate(over="ignore", invalid="ignore"):
        s = (w[:, :, :cin] * sc).astype(np.float32)
        hi = to_half(s, mistake)
        lo = to_half((w[:, :, :cin] if mistake == "residue_unscaled" else s) - hi.astype(np.float32), mistake)
    out = np.zeros((K * Cout, 2 * CinPad), np.float16)
    i = np.arange(cin)
    at = (i // 32) * 64 + ((i % 32) // 8) * 16 + i % 8
    out[:, at] = hi.reshape(K * Cout, cin)
    out[:, at + 8] = lo.reshape(K * Cout, cin)
    return np.concatenate([out.reshape(-1).view(np.uint16), np.full(SLACK, canary, np.uint16)]), np.float32(np.ldexp(1.0, -e))
