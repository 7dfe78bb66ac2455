"""GPU tests of BigVGAN's fused anti-aliased Snake activation (csrc/kk_bigvgan.hip through bigvgan.amp_act) and of the vocoder, against the float64
restatement of tests/_bigvgan_ref.py.

fp32: the kernel and every noted stage within 2e-4 of the reference's max, the pcm within 1e-3; item 1 alone equals its rows in the batch and a run
with another segment length equals the first, bit for bit; the padding columns of `out` keep their sentinel.

bf16: against float64 on the bf16-rounded inputs (and weights); the bars are twice the largest rel_max measured on an MI355X over the seeds BF16_SEEDS:
  kernel  (L, C) (1, 24): 1.48e-3, 2.44e-3, 1.84e-3; (5, 24): 2.18e-3, 2.10e-3, 1.75e-3; (23, 96): 2.62e-3, 1.72e-3, 1.77e-3; (24, 24): 1.86e-3, 1.98e-3,
          3.05e-3; (25, 96): 2.63e-3, 3.25e-3, 2.58e-3; (49, 25): 2.14e-3, 1.44e-3, 2.56e-3; (30, 24): 1.86e-3, 2.04e-3, 1.74e-3;
          (7, 1536): 2.80e-3, 3.3207e-3, 2.93e-3  -> bar 6.64e-3
  model   pcm, resblock "1": 6.41e-3, 6.9396e-3, 5.30e-3 -> bar 1.387e-2; resblock "2": 9.2484e-3, 8.59e-3, 5.90e-3 -> bar 1.849e-2
(fp32 measured: kernel 2.4e-7, stages 4.1e-7 at the worst.)"""
import numpy as np
import pytest
import torch

import _bigvgan_ref as R
from _util import err_stats
from mlx_audio_amd import bigvgan

pytestmark = pytest.mark.gpu

BF16_SEEDS = (7, 8, 9)
BF16_KERNEL_BAR, BF16_MODEL_BAR = 6.64e-3, {"1": 1.387e-2, "2": 1.849e-2}
# (L, C, pitch beyond C).  Small tensors run segments of 24 rows.  L 1 and 5: every tap clamps; 23 / 24 / 25: the halo hand-over at one segment +- 1; C 24 does
# not fill a wave (several segments share it); 96 with ld > C; 25 on an even pitch: a channel pair straddles C; 24 on an odd pitch: the one-channel path;
# 1536 x 7: three workgroups of channel groups
SHAPES = [(1, 24, 0), (5, 24, 0), (23, 96, 8), (24, 24, 0), (25, 96, 8), (49, 25, 1), (30, 24, 1), (7, 1536, 0)]
bf16_round = lambda a: torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def kernel_error(L, C, pad, dtype, seed):
    rng = np.random.default_rng(seed)
    tdt = torch.bfloat16 if dtype else torch.float32
    x = torch.tensor(rng.standard_normal((2, L, C + pad)), dtype=torch.float32).to(tdt).cuda()
    alpha, beta = rng.uniform(-1, 1, C), rng.uniform(-1, 1, C)
    out = torch.full((2, L, C + pad), -512.0, dtype=tdt, device="cuda")
    bigvgan.amp_act(x[:, :, :C], alpha, beta, True, out=out[:, :, :C])
    assert bool((out[:, :, C:] == -512.0).all())
    assert torch.equal(bigvgan.amp_act(x[1:, :, :C].contiguous(), alpha, beta, True)[0], out[1, :, :C])
    assert torch.equal(bigvgan.amp_act(x[:, :, :C], alpha, beta, True, seg=12), out[:, :, :C])
    ref = R.activation1d(x[:, :, :C].float().cpu().numpy(), alpha, beta, True)
    e = err_stats(out[:, :, :C].float().cpu().numpy(), ref)
    print(f"[bigvgan] kernel L {L} C {C} pad {pad} dtype {dtype} seed {seed}: rel_max {e['rel_max']:.4e}")
    return e["rel_max"]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("L,C,pad", SHAPES)
def test_kernel(L, C, pad, dtype):
    assert max(kernel_error(L, C, pad, dtype, s) for s in (BF16_SEEDS if dtype else BF16_SEEDS[:1])) <= (BF16_KERNEL_BAR if dtype else 2e-4)


_cache = {}


def model_case(resblock, final, seed, dtype):
    """(model, mel, reference pcm, reference stages) on bf16-representable parameters and input, shared by the fp32 and the bf16 test"""
    cfg = bigvgan.BigVGANConfig(**dict(R.TINY, resblock=resblock, use_tanh_at_final=final, use_bias_at_final=final))
    key = (resblock, final, seed)
    if key not in _cache:
        w = {k: bf16_round(v) if not k.endswith(".filter") else v for k, v in R.synth_weights(bigvgan.param_shapes(cfg), seed).items()}
        mel = bf16_round(np.random.default_rng(100 + seed).standard_normal((2, 8, 24)))
        _cache[key] = (w, mel) + R.forward(w, cfg, mel)
    w, mel, ref, stages = _cache[key]
    return bigvgan.BigVGAN(cfg, w, compute_dtype=dtype), mel, ref, stages


@pytest.mark.parametrize("final", [True, False])
@pytest.mark.parametrize("resblock", ["1", "2"])
def test_model_fp32(resblock, final):
    m, mel, ref, stages = model_case(resblock, final, BF16_SEEDS[0], "float32")
    pcm = m(mel)
    assert tuple(pcm.shape) == (2, 1, 24 * 8) and set(stages) == {"conv_pre", "stage0", "stage1", "activation_post"}
    for k, v in stages.items():
        e = err_stats(m.debug_fetch(k).cpu().numpy(), v)
        print(f"[bigvgan] fp32 resblock {resblock} final {final} {k}: rel_max {e['rel_max']:.4e}")
        assert e["max_abs"] <= 2e-4 * e["ref_max"], (k, e)
    e = err_stats(pcm.cpu().numpy(), ref)
    assert e["max_abs"] <= 1e-3 * max(1.0, e["ref_max"]) and np.abs(ref).max() > 0.05, e
    assert torch.equal(m(mel[1:])[0], pcm[1])
    assert tuple(m(mel[:1, :, :1]).shape) == (1, 1, 8)


@pytest.mark.parametrize("resblock", ["1", "2"])
def test_model_bf16(resblock):
    worst = 0.0
    for seed in BF16_SEEDS:
        m, mel, ref, _ = model_case(resblock, True, seed, "bfloat16")
        e = err_stats(m(mel).cpu().numpy(), ref)
        print(f"[bigvgan] bf16 resblock {resblock} seed {seed}: rel_max {e['rel_max']:.4e} rms_rel {e['rms_rel']:.4e}")
        worst = max(worst, e["rel_max"])
    assert worst <= BF16_MODEL_BAR[resblock]
