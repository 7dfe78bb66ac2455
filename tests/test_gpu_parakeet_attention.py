"""The relative-position attention kernel (parakeet.rel_pos_attention, kk_op_rel_pos_attention, csrc/kk_parakeet.hip) against the
float64 restatement on the identical bf16 operands, the positional term through the reference's literal pad / reshape / slice rel_shift.

Bound, as in test_gpu_whisper_attention.py: |out - ref| <= 2^-7 max|v| per (item, head): the probabilities enter the second product rounded to
bf16 (2^-9 each, weights summing to 1), the normaliser is taken before that rounding (2^-9), the output is rounded to bf16 (2^-9), one 2^-9 is
spare.  T = 1, 17: one tile, a one-row and a short table; 64, 65: the tile edge; 130: three key tiles, three query tiles, a moving band."""
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
B, H, SLACK = 2, 2, 3


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("T", [1, 17, 64, 65, 130])
def test_against_float64(T, hd):
    g = np.random.default_rng(1000 * hd + T)
    x = R.bf16_round(g.standard_normal((B, T, 3, H, hd)))
    p = R.bf16_round(g.standard_normal((2 * T - 1, H, hd)))
    u, v = (0.5 * g.standard_normal((H, hd))).astype(np.float32), (0.5 * g.standard_normal((H, hd))).astype(np.float32)
    ref = R.rel_pos_attention(*(x[:, :, i].transpose(0, 2, 1, 3) for i in range(3)), p.transpose(1, 0, 2), u, v)

    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt)  # noqa: E731
    rows = np.concatenate([x.reshape(B, T, -1), np.full((B, SLACK, 3 * H * hd), np.nan, np.float32)], axis=1)  # rows past T: never read
    qkv, pos = dev(rows, torch.bfloat16), dev(p.reshape(2 * T - 1, H * hd), torch.bfloat16)
    ud, vd = dev(u, torch.float32), dev(v, torch.float32)
    out = torch.full((B, T + SLACK, H * hd), 7.0, dtype=torch.bfloat16, device="cuda")
    parakeet.rel_pos_attention(qkv, pos, ud, vd, H, T=T, out=out)
    got = out.float().cpu().numpy()
    assert (got[:, T:] == 7.0).all(), "rows past T were written"
    assert not np.isnan(got[:, :T]).any(), "a row past T reached the output"
    worst = 0.0
    for b in range(B):
        for h in range(H):
            err = float(np.abs(got[b, :T, h * hd : (h + 1) * hd] - ref[b, h]).max())
            bound = 2.0 ** -7 * float(np.abs(x[b, :, 2, h]).max())
            worst = max(worst, err / bound)
            assert err <= bound, (b, h, err, bound)
    print(f"hd {hd} T {T}: max error / bound = {worst:.3f}")

    alone = parakeet.rel_pos_attention(qkv[1:2].contiguous(), pos, ud, vd, H, T=T)  # an item's bits do not depend on the batch
    assert torch.equal(alone[0, :T], out[1, :T])
