"""The float64 numpy references of tests/_norm_ref.py against torch's own float64 operators (no GPU): the GPU tests of the
normalisation kernels (tests/test_gpu_norm_kernels.py) are only as good as these."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _norm_ref as R

TOL = 1e-12


def _close(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(got - ref).max(initial=0.0) <= TOL * max(1.0, np.abs(ref).max(initial=0.0))


def _t(a):
    return torch.tensor(np.asarray(a, np.float64))


def _inorm(x_nc):
    """F.instance_norm of one item given as [n][C] -> [1][C][n]; torch refuses a single frame, whose normalised value is x - x = 0."""
    t = _t(np.asarray(x_nc).T)[None]
    return F.instance_norm(t, eps=1e-5) if t.shape[-1] > 1 else torch.zeros_like(t)


@pytest.mark.parametrize("n", [1, 2, 37, 60])
def test_instnorm_stats_matches_instance_norm(n):
    rng = np.random.default_rng(n)
    L, C = 60, 13
    x = rng.standard_normal((L, C)) * 2 + 3
    mean, rstd = R.instnorm_stats(x, n)
    ref = _inorm(x[:n])[0].T.numpy()  # [n][C]
    _close((x[:n] - mean) * rstd, ref)
    _close(mean, x[:n].mean(0))
    _close(rstd, 1.0 / np.sqrt(x[:n].var(0) + 1e-5))


def test_instnorm_stats_of_an_empty_item_are_zero():
    mean, rstd = R.instnorm_stats(np.ones((5, 3)), 0)
    assert mean.shape == rstd.shape == (3,) and not mean.any() and not rstd.any()
    assert R.adain(np.ones((5, 3)), 0, np.zeros(6)).shape == (0, 3)
    assert R.adain(np.ones((5, 3)), 0, np.zeros(6), pool_w=np.ones((3, 3)), pool_b=np.ones(3)).shape == (0, 3)


@pytest.mark.parametrize("act", ["none", "lrelu", "snake"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("n", [1, 2, 31, 50])
def test_adain_matches_torch(act, pool, n):
    rng = np.random.default_rng(100 + n)
    L, C = 50, 11
    x = rng.standard_normal((L, C)) * 2 + 3
    gb = rng.standard_normal(2 * C) * 0.5
    alpha = rng.uniform(0.5, 1.5, C)
    pw, pb = rng.standard_normal((C, 3)), rng.standard_normal(C)
    code = {"none": R.ACT_NONE, "lrelu": R.ACT_LRELU, "snake": R.ACT_SNAKE}[act]
    got = R.adain(x, n, gb, code, 0.2, alpha, pw if pool else None, pb if pool else None)
    y = (1 + _t(gb[:C])[None, :, None]) * _inorm(x[:n]) + _t(gb[C:])[None, :, None]  # [1][C][n]
    if act == "snake":
        a = _t(alpha)[None, :, None]
        y = y + (1 / a) * torch.sin(a * y) ** 2
    elif act == "lrelu":
        y = F.leaky_relu(y, 0.2)
    if pool:
        y = F.pad(F.conv_transpose1d(y, _t(pw)[:, None, :], _t(pb), 2, 1, 0, C), (1, 0))
    _close(got, y[0].T.numpy())
    assert got.shape[0] == (2 * n if pool else n)


@pytest.mark.parametrize("C", [1, 8, 100])
@pytest.mark.parametrize("form", ["wb", "gb"])
@pytest.mark.parametrize("res", [False, True])
def test_layernorm_matches_layer_norm(C, form, res):
    rng = np.random.default_rng(C)
    L, n, ld = 9, 7, C + 3
    x = rng.standard_normal((L, ld)) * 2 + 3
    r = rng.standard_normal((L, ld + 2)) if res else None
    w, b, gb = rng.standard_normal(C), rng.standard_normal(C), rng.standard_normal(2 * C)
    t = _t(x[:n, :C] + (r[:n, :C] if res else 0.0))
    for act in (R.ACT_NONE, R.ACT_LRELU):
        if form == "wb":
            got = R.layernorm(x, r, n, C, w=w, b=b, eps=1e-5, act=act, slope=0.1)
            ref = F.layer_norm(t, (C,), _t(w), _t(b), 1e-5)
        else:
            got = R.layernorm(x, r, n, C, gb=gb, eps=1e-5, act=act, slope=0.1)
            ref = (1 + _t(gb[:C])) * F.layer_norm(t, (C,), None, None, 1e-5) + _t(gb[C:])
        if act == R.ACT_LRELU:
            ref = F.leaky_relu(ref, 0.1)
        _close(got, ref.numpy())


@pytest.mark.parametrize("L", [0, 1, 128, 300])
def test_finalize_tiles_and_fold(L):
    """Exact tile sums of a data set give that data set's statistics; fold is the AdaIN affine re-associated."""
    rng = np.random.default_rng(L)
    ntiles, C = 3, 6
    x = np.zeros((ntiles * 128, C))
    x[:L] = rng.standard_normal((L, C)) * 2 + 3
    tiles = x.reshape(ntiles, 128, C)
    part = np.stack([tiles.sum(1), (tiles**2).sum(1)], 1)  # [ntiles][2][C], float64: no rounding of the partials here
    gb = rng.standard_normal(2 * C)
    mean, rstd, pa, pb = R.finalize_tiles(part, L, 1e-5, gb)
    m2, r2 = R.instnorm_stats(x, L)
    # one-pass variance in float64 on N(3, 2^2): cancellation costs ~ (mean / std)^2 * 2^-53, far under the tolerance
    _close(mean, m2)
    _close(rstd, r2)
    if L:
        _close(x[:L] * pa + pb, R.adain(x, L, gb))
        ref = (1 + _t(gb[:C])[None, :, None]) * _inorm(x[:L]) + _t(gb[C:])[None, :, None]
        _close(x[:L] * pa + pb, ref[0].T.numpy())
    else:
        assert not pa.any() and np.array_equal(pb, gb[C:])
    pa2, pb2 = R.fold(mean, rstd, gb)
    assert np.array_equal(pa, pa2) and np.array_equal(pb, pb2)
    assert R.finalize_tiles(part, L)[2:] == (None, None)


def test_finalize_tiles_clamps_a_negative_variance():
    part = np.zeros((1, 2, 1))
    part[0, 0, 0], part[0, 1, 0] = 64.0, 31.999  # SS / L < mean^2
    mean, rstd, _, _ = R.finalize_tiles(part, 128)
    assert mean[0] == 0.5 and rstd[0] == 1.0 / np.sqrt(1e-5)
