"""Pins tests/_conv_ref.py, the float64 reference of tests/test_gpu_conv_generic.py and tests/test_gpu_linear_rows.py, against
torch.nn.functional.conv1d / conv_transpose1d / linear in float64 on the CPU: every (Kw, stride, pad, dil) class the GPU files use, in_shift as a
nearest-neighbour repeat of the input, Kw < stride, ragged lengths as a run on the truncated item, the epilogue's order.  Agreement 1e-12 of the
tensor's largest value."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R

# (Kw, stride, pad, dil) of the GPU file's conv cases, and (Kw, stride, pad, output_padding) of its transposed cases
CONV_TAPS = [(3, 1, 1, 1), (1, 1, 0, 1), (7, 1, 9, 3), (11, 1, 25, 5), (3, 2, 1, 1), (12, 6, 3, 1), (4, 2, 0, 1), (7, 1, 6, 1)]
CONVT_TAPS = [(20, 10, 5, 0), (12, 6, 3, 0), (3, 2, 1, 0), (4, 2, 1, 0), (2, 4, 0, 0), (16, 8, 4, 3)]


def _close(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def _t(a):
    return torch.tensor(np.asarray(a, np.float64))


def torch_conv(x, w, bias, stride, pad, dil):
    return F.conv1d(_t(x).transpose(1, 2), _t(w).permute(0, 2, 1), None if bias is None else _t(bias), stride, pad, dil).transpose(1, 2).numpy()


def torch_convT(x, w, bias, stride, pad, opad):
    # torch's transposed weight is [Cin][Cout][Kw]; ours [Cout][Kw][Cin]
    return F.conv_transpose1d(_t(x).transpose(1, 2), _t(w).permute(2, 0, 1), None if bias is None else _t(bias), stride, pad, opad).transpose(1, 2).numpy()


@pytest.mark.parametrize("taps", CONV_TAPS, ids=str)
@pytest.mark.parametrize("L", [1, 37, 141])
def test_conv1d_against_torch(taps, L):
    Kw, s, p, d = taps
    rng = np.random.default_rng(Kw * 1000 + L)
    B, Cin, Cout = 2, 5, 4
    x, w, bias = rng.standard_normal((B, L, Cin)), rng.standard_normal((Cout, Kw, Cin)), rng.standard_normal(Cout)
    # rows past the input's end read as zero, so torch on the input followed by zero rows states the same op for any number of output rows
    # (and accepts an input shorter than the kernel)
    rows = max((L + 2 * p - d * (Kw - 1) - 1) // s + 1, 0) + 3
    xp = np.concatenate([x, np.zeros((B, 3 * s + d * Kw, Cin))], 1)
    got, S = R.conv1d(x, w, bias, stride=s, pad=p, dil=d, rows=rows)
    _close(got, torch_conv(xp, w, bias, s, p, d)[:, :rows])
    _close(S, torch_conv(np.abs(xp), np.abs(w), None, s, p, d)[:, :rows])


def test_conv1d_short_input_all_padding():
    """L = 1 under (11, 1, 25, 5): torch computes it too (the padded input is long enough); every tap but the centre reads padding."""
    rng = np.random.default_rng(5)
    x, w = rng.standard_normal((1, 1, 3)), rng.standard_normal((2, 11, 3))
    got, _ = R.conv1d(x, w, None, pad=25, dil=5, rows=1)
    _close(got, np.einsum("blc,oc->blo", x, w[:, 5, :]))


@pytest.mark.parametrize("Kw", [1, 3])
@pytest.mark.parametrize("shift", [1, 2])
def test_in_shift_is_a_nearest_neighbour_repeat(Kw, shift):
    rng = np.random.default_rng(Kw + shift)
    B, L, Cin, Cout, p = 2, 41, 6, 5, Kw // 2
    x, w, bias = rng.standard_normal((B, L, Cin)), rng.standard_normal((Cout, Kw, Cin)), rng.standard_normal(Cout)
    xu = np.repeat(x, 1 << shift, axis=1)
    got, S = R.conv1d(x, w, bias, pad=p, in_shift=shift, rows=xu.shape[1])
    _close(got, torch_conv(xu, w, bias, 1, p, 1))
    _close(S, torch_conv(np.abs(xu), np.abs(w), None, 1, p, 1))


@pytest.mark.parametrize("taps", CONVT_TAPS, ids=str)
@pytest.mark.parametrize("L", [1, 33, 129])
def test_conv_transpose1d_against_torch(taps, L):
    Kw, s, p, opad = taps
    rng = np.random.default_rng(Kw * 1000 + L)
    B, Cin, Cout = 2, 5, 4
    Lout = (L - 1) * s - 2 * p + Kw + opad
    x, w, bias = rng.standard_normal((B, L, Cin)), rng.standard_normal((Cout, Kw, Cin)), rng.standard_normal(Cout)
    ref = torch_convT(x, w, bias, s, p, opad)
    assert ref.shape[1] == Lout
    got, S = R.conv_transpose1d(x, w, bias, stride=s, pad=p, rows=Lout)
    _close(got, ref)
    _close(S, torch_convT(np.abs(x), np.abs(w), None, s, p, opad))
    if Kw < s:  # phases no tap reaches hold the bias alone
        r = (np.arange(Lout) + p) % s
        assert np.array_equal(got[:, r >= Kw], np.broadcast_to(bias, got[:, r >= Kw].shape)) and np.all(S[:, r >= Kw] == 0)


def test_ragged_items_are_truncated_items():
    """lin / lout: item b computes what the item cut to lin[b] rows computes, and rows from lout[b] on are zero (also under bias, res, accumulate)."""
    rng = np.random.default_rng(7)
    B, L, Cin, Cout, Kw = 3, 30, 5, 4, 7
    lens = [30, 11, 0]
    x, w, bias = rng.standard_normal((B, L, Cin)), rng.standard_normal((Cout, Kw, Cin)), rng.standard_normal(Cout)
    res, old = rng.standard_normal((B, L, Cout)), rng.standard_normal((B, L, Cout))
    got, _ = R.conv1d(x, w, bias, pad=9, dil=3, res=res, accumulate_into=old, lin=lens, lout=lens, rows=L)
    for b, n in enumerate(lens):
        assert np.all(got[b, n:] == 0)
        if n:
            _close(got[b, :n], torch_conv(x[b : b + 1, :n], w, bias, 1, 9, 3)[0] + res[b, :n] + old[b, :n])
    s, p = 2, 1
    louts = [2 * n for n in lens]
    gt, _ = R.conv_transpose1d(x, w[:, :4], bias, stride=s, pad=p, lin=lens, lout=louts, rows=2 * L)
    for b, n in enumerate(lens):
        assert np.all(gt[b, 2 * n :] == 0)
        if n:
            _close(gt[b, : 2 * n], torch_convT(x[b : b + 1, :n], w[:, :4], bias, s, p, 0)[0])


def test_epilogue_order_and_activations():
    rng = np.random.default_rng(8)
    B, L, Cin, Cout = 2, 19, 6, 5
    x, w, bias = rng.standard_normal((B, L, Cin)), rng.standard_normal((Cout, 3, Cin)), rng.standard_normal(Cout)
    res, old = rng.standard_normal((B, L, Cout)), rng.standard_normal((B, L, Cout))
    base = _t(torch_conv(np.where(x > 0, x, 0.1 * x), w, bias, 1, 1, 1))
    for act, fn in ((R.ACT_NONE, lambda v: v), (R.ACT_LRELU, lambda v: F.leaky_relu(v, 0.2)), (R.ACT_GELU, F.gelu),
                    (R.ACT_GELU_TANH, lambda v: F.gelu(v, approximate="tanh"))):
        got, _, pre = R.conv1d(x, w, bias, pad=1, in_slope=0.1, act=act, act_slope=0.2, res=res, scale=0.25, accumulate_into=old, rows=L, parts=True)
        _close(got, ((fn(base) + _t(res)) * 0.25 + _t(old)).numpy())
        _close(pre, base.numpy())
    elu, _ = R.conv1d(x, w, bias, pad=1, elu=True, rows=L)
    _close(elu, torch_conv(F.elu(_t(x)).numpy(), w, bias, 1, 1, 1))
    relu, _ = R.conv1d(x, w, bias, pad=1, in_slope=0.0, rows=L)
    _close(relu, torch_conv(np.maximum(x, 0), w, bias, 1, 1, 1))


def test_linear_rows_against_torch():
    rng = np.random.default_rng(9)
    B, rows, K, N = 3, 7, 32, 6
    lens = [7, 3, 0]
    x, w, bias = rng.standard_normal((B, rows, K)), rng.standard_normal((N, K)), rng.standard_normal(N)
    for act, fn in ((R.ACT_NONE, lambda v: v), (R.ACT_GELU, F.gelu)):
        got, S = R.linear_rows(x, w, bias, act, lens)
        ref = fn(F.linear(_t(x), _t(w), _t(bias))).numpy()
        for b, n in enumerate(lens):
            ref[b, n:] = 0
        _close(got, ref)
        _close(S, F.linear(_t(np.abs(x)), _t(np.abs(w))).numpy())


def test_bf16_round_and_pack():
    v = np.array([1.00390625, 1.01171875, -0.0, 3.0e38, 1e-3], np.float32)
    assert np.array_equal(R.bf16_round(v).view(np.uint32), torch.tensor(v).bfloat16().float().numpy().view(np.uint32))
    w = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)
    p, ldw = R.pack_w(w)
    assert ldw == 64 and p.shape == (3, 5, 64) and p[1, 4, 1] == w[1, 1, 4] and np.all(p[:, :, 2:] == 0)
