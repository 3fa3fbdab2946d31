"""Pins tests/conv_ref.py -- the float64 reference tests/test_conv_kernels.py compares the conv kernels with -- on the CPU, before
anything is compared with it: against torch's conv1d, against the ECAPA oracle's TDNN block, and against hand-computed frames."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_ref import conv_ref, src_frames


@pytest.mark.parametrize("dil", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_reference_equals_torch_conv1d_on_reflect_padded_full_items(k, dil):
    rng = np.random.default_rng(100 * k + dil)
    items, T, cin, cout = 3, 37, 7, 5
    x = rng.standard_normal((items, T, cin))
    w = rng.standard_normal((k, cout, cin))
    b = rng.standard_normal(cout)
    y, S, acc = conv_ref(x.reshape(-1, cin), w, [T] * items, [T] * items, T, dil=dil, bias=b)
    xt = torch.from_numpy(x).transpose(1, 2)                        # [items][cin][T]
    pad = dil * (k - 1) // 2
    if pad:
        xt = F.pad(xt, (pad, pad), mode="reflect")
    ref = F.conv1d(xt, torch.from_numpy(w).permute(1, 2, 0).contiguous(), torch.from_numpy(b), dilation=dil).transpose(1, 2).reshape(-1, cout).numpy()
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(y, acc) and (S >= np.abs(acc) - 1e-12 * S).all()


def test_reference_equals_ecapa_oracle_tdnn_block():
    from oracle import nn_oracle as nn
    we = nn.synth_embedding_weights()
    p, dil = "blocks.1.res2net.0", 2
    W = np.asarray(we[p + ".conv.weight"], np.float64)              # [cout][cin][k]
    g, bb = np.asarray(we[p + ".norm.weight"], np.float64), np.asarray(we[p + ".norm.bias"], np.float64)
    mu, var = np.asarray(we[p + ".norm.running_mean"], np.float64), np.asarray(we[p + ".norm.running_var"], np.float64)
    scale = g / np.sqrt(var + 1e-5)
    shift = bb - mu * scale
    rng = np.random.default_rng(5)
    items, T = 2, 41
    x = rng.standard_normal((items, T, W.shape[1]))
    ref = nn.EcapaOracle(we, torch.float64)._tdnn(torch.from_numpy(x).transpose(1, 2), p, dil).transpose(1, 2).reshape(-1, W.shape[0]).numpy()
    y, _, _ = conv_ref(x.reshape(-1, W.shape[1]), W.transpose(2, 0, 1), [T] * items, [T] * items, T, dil=dil,
                       bias=np.asarray(we[p + ".conv.bias"], np.float64), scale=scale, shift=shift, act1=1)
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


def test_clamp_and_reflection_by_hand():
    """k = 3, dilation 2, one channel, w = (1, 10, 100): y[t] = x[q0] + 10 x[q1] + 100 x[q2].  An item of three frames x = (1, 2, 3):
    - as a FULL item (tin = 3) the right edge reflects about frame 2:  t = 2 reads q = (0, 2, 4 -> 0)
    - as the three stored frames of a longer item (tin = 5) nothing reflects at the right edge, the taps beyond the last stored frame read it:
      t = 2 reads q = (0, 2, 4 -> 2);  t = 1 reads q = (-1 -> 1, 1, 3 -> 2);  t = 0 reads q = (-2 -> 2, 0, 2)"""
    w = np.array([1.0, 10.0, 100.0]).reshape(3, 1, 1)
    x = np.array([[1.0], [2.0], [3.0]])
    full, _, _ = conv_ref(x, w, [3], [3], 3, dil=2)
    assert full[:, 0].tolist() == [3 + 10 + 300, 2 + 20 + 200, 1 + 30 + 100]
    short, S, _ = conv_ref(x, w, [3], [3], 5, dil=2)
    assert short[:, 0].tolist() == [3 + 10 + 300, 2 + 20 + 300, 1 + 30 + 300]
    assert S[:, 0].tolist() == short[:, 0].tolist()
    # two items in one buffer: the second item's frames never read the first's
    two, _, _ = conv_ref(np.concatenate([x, 10 * x]), w, [3, 3], [3, 2], 5, dil=2)
    assert two[:, 0].tolist() == [313, 322, 331, 3130, 3220]
    # "valid": no mapping at all
    v, _, _ = conv_ref(np.arange(1.0, 8.0).reshape(7, 1), w, [7], [3], 7, dil=2, pad_mode=1)
    assert v[:, 0].tolist() == [1 + 30 + 500, 2 + 40 + 600, 3 + 50 + 700]
    assert src_frames([0, 1, 2], 0, 3, 2, 5, 3, 0).tolist() == [2, 1, 0]


def test_epilogue_order_and_second_input():
    """y = act2(act1(acc) * scale + shift); X2 is added to X; the per-item bias joins the accumulator before act1"""
    w = np.array([[[2.0]]])
    x, x2 = np.array([[1.0], [-3.0]]), np.array([[0.5], [0.5]])
    y, S, acc = conv_ref(x, w, [1, 1], [1, 1], 1, x2=x2, bias=[1.0], item_bias=[[0.0], [2.0]], scale=[0.5], shift=[-1.0], act1=2, act2=1)
    assert acc[:, 0].tolist() == [4.0, -2.0] and S[:, 0].tolist() == [4.0, 10.0]
    assert np.allclose(y[:, 0], np.tanh([4.0 * 0.5 - 1.0, -0.02 * 0.5 - 1.0]), rtol=1e-15, atol=0)
    y, _, _ = conv_ref(x, w, [1, 1], [1, 1], 1, act1=1, act2=2)
    assert np.allclose(y[:, 0], [1 / (1 + np.exp(-2.0)), 0.5], rtol=1e-15, atol=0)
