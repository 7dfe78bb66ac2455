"""GPU tests of Vocos' two kernels (csrc/kk_vocos.hip through vocos.dwconv_layernorm and vocos.istft_head) and of the vocoder, against the float64
restatement of tests/_vocos_ref.py.

fp32: both kernels and every noted stage within 2e-4 of the reference's max, the pcm within 1e-3; item 1 alone equals its rows in the batch and a run
with another rows= / group= equals the first, bit for bit; the padding columns of `out` keep their sentinel.  A bf16 `out` of the dwconv -> LayerNorm
kernel is the fp32 bar plus one bf16 rounding, element by element.

bf16 model: against float64 on the bf16-rounded parameters and features; the bar is twice the largest rel_max measured on an MI355X over the seeds
BF16_SEEDS:
  pcm, LayerNorm model (TINY): 2.8787e-3, 3.5139e-3, 3.1728e-3 -> bar 7.03e-3; AdaLayerNorm twin: 5.0384e-3, 3.4825e-3, 2.6941e-3 -> bar 1.008e-2
(fp32 measured: dwconv -> LayerNorm 1.1e-7 at C = 1024, bf16 out 2.7e-3 at the worst; iSTFT 2.2e-7; stages 2.4e-7, pcm 3.0e-7 at the worst.)"""
import numpy as np
import pytest
import torch

import _vocos_ref as R
from _util import err_stats
from mlx_audio_amd import vocos

pytestmark = pytest.mark.gpu

BF16_SEEDS = (7, 8, 9)
BF16_MODEL_BAR = {False: 7.03e-3, True: 1.008e-2}  # by adanorm
# (T, C, pitch beyond C); C <= 512 runs 16 rows per workgroup, 1024 runs 12.  T 1 and 3: every tap window hangs over an edge; 15 / 16 / 17: the halo
# hand-over at one tile -+ 1; C 24 does not fill a wave, 100 is no multiple of 64 (with ld > C and an unaligned pitch: the one-float staging path);
# 384 / 512: the public checkpoints, two tiles; 1024: the widest, 16 channels per lane
DW_SHAPES = [(1, 24, 0), (3, 24, 0), (7, 100, 0), (15, 24, 0), (16, 24, 0), (17, 100, 3), (17, 384, 0), (17, 512, 0), (9, 1024, 0)]
bf16_round = lambda a: torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,C,pad", DW_SHAPES)
def test_dwconv_ln(T, C, pad, out_dtype):
    rng = np.random.default_rng(T * 10007 + C)
    x = torch.tensor(rng.standard_normal((2, T, C + pad)), dtype=torch.float32).cuda()
    w, b, lw, lb = rng.standard_normal((C, 7, 1)) / 7**0.5, 0.1 * rng.standard_normal(C), rng.uniform(0.5, 1.5, C), 0.1 * rng.standard_normal(C)
    ss = None if (T, C) != (17, 100) else np.stack([rng.uniform(0.5, 1.5, (2, C)), rng.standard_normal((2, C))], 1)  # the per-item (scale, shift) form
    assert vocos.dwconv_rows(C) == (12 if C == 1024 else 16)
    run = lambda xx, s=ss, **kw: vocos.dwconv_layernorm(xx, w, b, lw, lb, scale_shift=s, out_dtype=out_dtype, **kw)
    out = torch.full((2, T, C + pad), -512.0, dtype=out_dtype, device="cuda")
    run(x[:, :, :C], out=out[:, :, :C])
    assert bool((out[:, :, C:] == -512.0).all())
    assert torch.equal(run(x[1:, :, :C].contiguous(), None if ss is None else ss[1:])[0], out[1, :, :C])
    assert torch.equal(run(x[:, :, :C], rows=5), out[:, :, :C])
    ref = R.dwconv_ln(x[:, :, :C].cpu().numpy(), w.astype(np.float32), b.astype(np.float32), lw.astype(np.float32), lb.astype(np.float32), scale_shift=ss)
    got = out[:, :, :C].float().cpu().numpy()
    e = err_stats(got, ref)
    print(f"[vocos] dwconv_ln T {T} C {C} pad {pad} {out_dtype}: rel_max {e['rel_max']:.4e}")
    if out_dtype == torch.float32:
        assert e["max_abs"] <= 2e-4 * e["ref_max"], e
    else:
        assert bool((np.abs(got - ref) <= 2e-4 * e["ref_max"] + 2.0**-8 * np.abs(ref)).all()), e


@pytest.mark.parametrize("T", [2, 4, 5, 7, 8, 9])  # the default group is 5 hops: G + 2, G + 3, G + 4 frames are one group exactly, one + 1 hop, + 2
@pytest.mark.parametrize("n_fft,hop", [(256, 64), (320, 80), (512, 128), (1024, 256), (1280, 320)])
def test_istft_head(n_fft, hop, T):
    rng = np.random.default_rng(n_fft + T)
    F = n_fft // 2 + 1
    h = rng.standard_normal((2, T, n_fft + 2 + 6)) * np.r_[np.full(F, 2.5), np.full(F, 4.0), np.ones(6)]  # a few per cent of the bins clip; phases beyond +-pi
    hd = torch.tensor(h, dtype=torch.float32).cuda()
    ref, clipped = R.istft_head(hd[:, :, : n_fft + 2].cpu().numpy(), n_fft, hop)
    assert 0.01 <= clipped <= 0.10, clipped
    out = vocos.istft_head(hd[:, :, : n_fft + 2], n_fft, hop)
    assert tuple(out.shape) == (2, (T - 1) * hop)
    assert torch.equal(vocos.istft_head(hd[1:, :, : n_fft + 2].contiguous(), n_fft, hop)[0], out[1])
    assert torch.equal(vocos.istft_head(hd[:, :, : n_fft + 2], n_fft, hop, group=3), out)
    e = err_stats(out.cpu().numpy(), ref)
    print(f"[vocos] istft n_fft {n_fft} T {T}: rel_max {e['rel_max']:.4e} clipped {clipped:.3f}")
    assert e["max_abs"] <= 2e-4 * e["ref_max"], e


_cache = {}


def model_case(ada, seed, dtype):
    """(model, features, condition, reference pcm, reference stages) on bf16-representable parameters and inputs, shared by the fp32 and the bf16 test"""
    cfg = vocos.VocosConfig(**(R.TINY_ADA if ada else R.TINY))
    if (ada, seed) not in _cache:
        rng = np.random.default_rng(100 + seed)
        w = {k: bf16_round(v) for k, v in R.synth_weights(vocos.param_shapes(cfg), seed).items()}
        feat, cond = bf16_round(rng.standard_normal((2, 9, 24))), bf16_round(rng.uniform(0, 3, (2, 4))) if ada else None
        _cache[(ada, seed)] = (w, feat, cond) + R.forward(w, cfg, feat, cond)
    w, feat, cond, ref, stages = _cache[(ada, seed)]
    return vocos.Vocos(cfg, w, compute_dtype=dtype), feat, cond, ref, stages


@pytest.mark.parametrize("ada", [False, True])
def test_model_fp32(ada):
    m, feat, cond, ref, stages = model_case(ada, BF16_SEEDS[0], "float32")
    pcm = m.decode(feat, bandwidth_id=cond)
    assert tuple(pcm.shape) == (2, 8 * 64) and set(stages) == {"embed", "block0", "block1", "backbone", "head"}
    for k, v in stages.items():
        e = err_stats(m.debug_fetch(k).cpu().numpy(), v)
        print(f"[vocos] fp32 ada {ada} {k}: rel_max {e['rel_max']:.4e}")
        assert e["max_abs"] <= 2e-4 * e["ref_max"], (k, e)
    e = err_stats(pcm.cpu().numpy(), ref)
    print(f"[vocos] fp32 ada {ada} pcm: rel_max {e['rel_max']:.4e} ref_max {e['ref_max']:.3f}")
    assert e["max_abs"] <= 1e-3 * max(1.0, e["ref_max"]) and np.abs(ref).max() > 0.05, e
    assert torch.equal(m.decode(feat[1:], bandwidth_id=None if cond is None else cond[1:])[0], pcm[1])
    assert torch.equal(m.decode(np.transpose(feat, (0, 2, 1)), bandwidth_id=cond), pcm)  # channels-first, the reference's transpose rule


@pytest.mark.parametrize("ada", [False, True])
def test_model_bf16(ada):
    worst = 0.0
    for seed in BF16_SEEDS:
        m, feat, cond, ref, _ = model_case(ada, seed, "bfloat16")
        e = err_stats(m.decode(feat, bandwidth_id=cond).cpu().numpy(), ref)
        print(f"[vocos] bf16 ada {ada} seed {seed}: rel_max {e['rel_max']:.4e} rms_rel {e['rms_rel']:.4e}")
        worst = max(worst, e["rel_max"])
    assert worst <= BF16_MODEL_BAR[ada]
