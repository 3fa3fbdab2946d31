"""Float64 reference of the conv / linear operation libsdhip's conv_gemm kernels compute, written from the contract in the ConvArgs
comments of csrc/common.h (not from the kernels' device code) in plain numpy.

Row spaces.  Item i stores n_in[i] input frames and n_out[i] output frames, item after item (the compact spaces of the embedding
network); the dense mapping is the special case n_in[i] = tp_in, n_out[i] = tp_out with `valid_out` = t output frames defined.
For output frame t of item i, tap kk reads input frame

    pad_mode 0 ("same"):  q = t + (kk - (kt - 1) // 2) * dil, reflected about 0 and about tin - 1, then clamped to [0, n_in[i] - 1]
    pad_mode 1 ("valid"): q = t + kk * dil

    acc = sum_kk  (x[q] (+ x2[q])) . w[kk]  + bias + item_bias[i]
    y   = act2(act1(acc) * scale + shift)          act1: 0 none, 1 relu, 2 leaky relu (0.01); act2: 0 none, 1 tanh, 2 sigmoid

conv_ref also returns S = sum |x| |w| + |bias| + |item_bias| per output, the magnitude a rounding-error bound scales with, and acc.
The operands are taken as the kernel sees them (the caller rounds them to fp16 first for the fp16 kernels)."""
import numpy as np


def src_frames(t, kk, kt, dil, tin, n_in_i, pad_mode):
    """input frame(s) that tap kk of output frame(s) t reads"""
    t = np.asarray(t, np.int64)
    if pad_mode == 1:
        return t + kk * dil
    q = t + (kk - (kt - 1) // 2) * dil
    q = np.where(q < 0, -q, q)
    q = np.where(q > tin - 1, 2 * (tin - 1) - q, q)
    return np.clip(q, 0, n_in_i - 1)


def conv_ref(x, w, n_in, n_out, tin, dil=1, pad_mode=0, x2=None, bias=None, scale=None, shift=None, item_bias=None, act1=0, act2=0):
    """x [sum n_in][cin], w [kt][cout][cin] -> (y, S, acc), each [sum n_out][cout] float64"""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    kt, cout, cin = w.shape
    n_in, n_out = np.asarray(n_in, np.int64), np.asarray(n_out, np.int64)
    assert x.shape == (n_in.sum(), cin)
    xs = x if x2 is None else x + np.asarray(x2, np.float64)      # the kernels add X2 to X before the contraction (exact in f64 for the tests' operands)
    xa = np.abs(x) if x2 is None else np.abs(x) + np.abs(np.asarray(x2, np.float64))
    i0 = np.concatenate([[0], np.cumsum(n_in)])
    o0 = np.concatenate([[0], np.cumsum(n_out)])
    M = int(o0[-1])
    acc = np.zeros((M, cout))
    S = np.zeros((M, cout))
    wa = np.abs(w)
    for i in range(len(n_in)):
        t = np.arange(n_out[i])
        for kk in range(kt):
            q = src_frames(t, kk, kt, dil, tin, n_in[i], pad_mode)
            assert q.min() >= 0 and q.max() < n_in[i], "tap outside the stored rows"
            acc[o0[i]:o0[i + 1]] += xs[i0[i] + q] @ w[kk].T
            S[o0[i]:o0[i + 1]] += xa[i0[i] + q] @ wa[kk].T
        if item_bias is not None:
            acc[o0[i]:o0[i + 1]] += np.asarray(item_bias, np.float64)[i]
            S[o0[i]:o0[i + 1]] += np.abs(np.asarray(item_bias, np.float64)[i])
    if bias is not None:
        acc += np.asarray(bias, np.float64)
        S += np.abs(np.asarray(bias, np.float64))
    v = acc
    if act1 == 1:
        v = np.maximum(v, 0.0)
    elif act1 == 2:
        v = np.where(v > 0, v, 0.01 * v)
    if scale is not None:
        v = v * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if act2 == 1:
        v = np.tanh(v)
    elif act2 == 2:
        v = 1.0 / (1.0 + np.exp(-v))
    return v, S, acc
