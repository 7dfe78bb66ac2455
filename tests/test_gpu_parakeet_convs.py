"""The Conformer conv core and the sub-sampling 2-D convs on the device (parakeet.conformer_dwconv / conv2d_s2, csrc/kk_parakeet.hip)
against float64 restatements on the identical bf16 inputs.

Bar, per element: |out - ref| <= 2^-8 |ref| (the output's one bf16 rounding) + 4 x the largest error of the same restatement run in float32
(the project's margin for another summation order and another exp).  Both figures are printed.
Conv core: T = 1 and 5 are shorter than the halo of k = 31 on both sides, 70 crosses the 64-step tile; D = 128 is two channel slabs; the BatchNorm
statistics are non-trivial and are folded by parakeet.fold_batch_norm, while the restatement applies them unfolded.
2-D convs: odd and even sizes on both axes, a single pixel, and F x C past one workgroup."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _parakeet_ref as R  # noqa: E402

from mlx_audio_amd import parakeet  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(got, ref, ref32, what):
    e32 = float(np.abs(ref32 - ref).max())
    err = np.abs(got - ref)
    print(f"{what}: max error {float(err.max()):.3e}, float32 restatement {e32:.3e}")
    assert (err <= 2.0 ** -8 * np.abs(ref) + 4 * e32).all(), float((err - 2.0 ** -8 * np.abs(ref)).max())


@pytest.mark.parametrize("k", [9, 31])
@pytest.mark.parametrize("T", [1, 5, 70])
def test_conv_core(T, k):
    B, D = 2, 128
    g = np.random.default_rng(100 * k + T)
    x = R.bf16_round(g.standard_normal((B, T, 2 * D)))
    dw_w, dw_b = g.standard_normal((D, k)) / np.sqrt(k), 0.1 * g.standard_normal(D)
    bn = [1 + 0.2 * g.standard_normal(D), 0.2 * g.standard_normal(D), 0.3 * g.standard_normal(D), g.uniform(0.5, 2.0, D)]  # weight, bias, mean, var
    w, b = parakeet.fold_batch_norm(dw_w, dw_b, *bn)
    got = parakeet.conformer_dwconv(torch.from_numpy(x).cuda().bfloat16(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda())
    _check(got.float().cpu().numpy(), R.conv_core(x, dw_w, dw_b, *bn), R.conv_core(x, dw_w, dw_b, *bn, dtype=torch.float32), f"T {T} k {k}")


@pytest.mark.parametrize("stem", [True, False])
@pytest.mark.parametrize("T,F", [(1, 1), (7, 10), (33, 80)])
def test_conv2d_s2(T, F, stem):
    B, Cn = 2, 32
    g = np.random.default_rng(10 * T + F + stem)
    x = g.standard_normal((B, T, F) if stem else (B, T, F, Cn)).astype(np.float32)
    x = x if stem else R.bf16_round(x)
    w, b = g.standard_normal((Cn, 1, 3, 3)).astype(np.float32) / 3, (0.1 * g.standard_normal(Cn)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    got = parakeet.conv2d_s2(xd if stem else xd.bfloat16(), torch.from_numpy(np.ascontiguousarray(w.reshape(Cn, 9).T)).cuda(), torch.from_numpy(b).cuda(), stem)
    assert got.shape == (B, (T - 1) // 2 + 1, (F - 1) // 2 + 1, Cn)
    _check(got.float().cpu().numpy(), R.conv2d_s2(x, w, b, stem), R.conv2d_s2(x, w, b, stem, dtype=torch.float32), f"T {T} F {F} stem {stem}")
