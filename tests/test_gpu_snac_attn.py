"""GPU tests of SNAC's windowed attention (csrc/kk_snac_attn.hip through kk_op_snac_local_attn) and of the codec with LocalMHA, against the
float64 restatement of tests/_snac_attn_ref.py.

fp32: the kernel, `decoder_attn` / `encoder_attn` and every stage within 2e-4 of the reference's max (the codec's stage bar), the pcm within
1e-3; rows of item 1 alone equal its rows in the batch, bit for bit.  encode: tests/test_gpu_snac.py's criterion (near-ties, 5 % cap).

bf16: against float64 on the bf16-rounded inputs; the bars are twice the largest rel_max measured on an MI355X over the seeds BF16_SEEDS:
  kernel  T 32 H 1: 2.47e-3, 4.67e-3, 3.24e-3; T 96 H 3: 4.07e-3, 3.97e-3, 4.02e-3; T 64 H 24: 3.73e-3, 3.62e-3, 3.81e-3  -> bar 9.35e-3
  decode  decoder_dim 128: 4.54e-2, 3.83e-2, 3.49e-2 -> bar 9.08e-2; decoder_dim 192: 4.40e-2, 3.85e-2, 4.17e-2 -> bar 8.80e-2
(fp32 measured: kernel 6.9e-7, stages 7.2e-7 at the worst.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import _snac_attn_ref as A
import _snac_ref as R
from _util import err_stats
from mlx_audio_amd import _lib, snac

pytestmark = pytest.mark.gpu

BF16_SEEDS = (7, 8, 9)
BF16_KERNEL_BAR, BF16_DECODE_BAR = 9.35e-3, {128: 9.08e-2, 192: 8.80e-2}
SHAPES = [(32, 1, 0), (96, 3, 8), (64, 24, 0)]  # (T, H, pitch beyond 3 D): one wave; heads that do not fill a workgroup, ld > 3 D; the 44 kHz decoder width
_cache = {}


def kernel_error(T, H, pad, dtype, seed):
    """rel_max of the kernel on random q | k | v, B = 2, after checking that item 1 alone gives the same bits."""
    lib, tdt, D = _lib.load(), torch.bfloat16 if dtype else torch.float32, 64 * H
    x = torch.tensor(np.random.default_rng(seed).standard_normal((2, T, 3 * D + pad)), dtype=torch.float32).to(tdt).cuda()
    out = torch.full((2, T, D + pad), -512.0, dtype=tdt, device="cuda")
    one = torch.empty((1, T, D), dtype=tdt, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.kk_op_snac_local_attn(st, 2, T, H, C.c_void_p(x.data_ptr()), 3 * D + pad, dtype, C.c_void_p(out.data_ptr()), D + pad) == 0, lib.kk_last_error()
    assert lib.kk_op_snac_local_attn(st, 1, T, H, C.c_void_p(x[1:].data_ptr()), 3 * D + pad, dtype, C.c_void_p(one.data_ptr()), D) == 0, lib.kk_last_error()
    assert torch.equal(one[0], out[1, :, :D]) and bool((out[:, :, D:] == -512.0).all())
    e = err_stats(out[:, :, :D].float().cpu().numpy(), A.attention(x[:, :, : 3 * D].float().cpu().numpy()))
    print(f"[snac attn] kernel T {T} H {H} dtype {dtype} seed {seed}: rel_max {e['rel_max']:.4e}")
    return e["rel_max"]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("T,H,pad", SHAPES)
def test_kernel(T, H, pad, dtype):
    assert max(kernel_error(T, H, pad, dtype, s) for s in BF16_SEEDS) <= (BF16_KERNEL_BAR if dtype else 2e-4)


def setup(dim, seed=A.WEIGHT_SEED, dtype="float32"):
    if (dim, seed, dtype) not in _cache:
        cfg = snac.SNACConfig(**A.CONFIGS[dim])
        w = _cache.setdefault((dim, seed), A.synth_weights(snac.param_shapes(cfg, local_attention=True), seed))
        _cache[(dim, seed, dtype)] = (cfg, w, snac.SNAC(cfg, w, compute_dtype=dtype, local_attention=True))
    return _cache[(dim, seed, dtype)]


def decode_case(dim, seed, dtype):
    cfg, w, m = setup(dim, seed, dtype)
    rng = np.random.default_rng(300 + seed)
    codes = [rng.integers(0, cfg.codebook_size, (2, 64 // s)).astype(np.int32) for s in cfg.vq_strides]
    noise = m.draw_noise(2, seed=3)
    if (dim, seed, "ref") not in _cache:
        _cache[(dim, seed, "ref")] = A.decoder(R.Weights(w), cfg, R.from_codes(R.Weights(w), cfg, codes), [n.numpy() for n in noise])
    return m, codes, noise, _cache[(dim, seed, "ref")]


@pytest.mark.parametrize("dim", sorted(A.CONFIGS))
def test_decode_fp32(dim):
    m, codes, noise, (ref, stages) = decode_case(dim, A.WEIGHT_SEED, "float32")
    pcm = m.decode(codes, noise=noise)
    for k, v in stages.items():
        e = err_stats(m.debug_fetch(k).cpu().numpy(), v)
        print(f"[snac attn] decode fp32 dim {dim} {k}: rel_max {e['rel_max']:.4e}")
        assert e["max_abs"] <= 2e-4 * e["ref_max"], (k, e)
    e = err_stats(pcm.cpu().numpy(), ref)
    assert e["max_abs"] <= 1e-3 * max(1.0, e["ref_max"]) and np.abs(ref).max() > 0.05, e
    assert torch.equal(m.decode([c[1:] for c in codes], noise=[n[1:] for n in noise])[0], pcm[1])


@pytest.mark.parametrize("dim", sorted(A.CONFIGS))
def test_decode_bf16(dim):
    worst = 0.0
    for seed in BF16_SEEDS:
        m, codes, noise, (ref, _) = decode_case(dim, seed, "bfloat16")
        e = err_stats(m.decode(codes, noise=noise).cpu().numpy(), ref)
        print(f"[snac attn] decode bf16 dim {dim} seed {seed}: rel_max {e['rel_max']:.4e} rms_rel {e['rms_rel']:.4e}")
        worst = max(worst, e["rel_max"])
    assert worst <= BF16_DECODE_BAR[dim]


@pytest.mark.parametrize("case", sorted(A.ENCODE_CASES))
def test_encode(case):
    B, N, seed = A.ENCODE_CASES[case]
    cfg, w, m = setup(128)
    x = R.audio(B, N, seed)
    codes = m.encode(torch.tensor(x))
    ref, trace, z, att = A.encode(R.Weights(w), cfg, x)
    for name, v in (("encoder_attn", att), ("encoder", z)):
        e = err_stats(m.debug_fetch(name).cpu().numpy(), v)
        print(f"[snac attn] encode {case} {name}: rel_max {e['rel_max']:.4e}")
        assert e["max_abs"] <= 2e-4 * e["ref_max"], (name, e)
    excused, frames = R.excused_frames([c.cpu().numpy() for c in codes], ref, trace, cfg.vq_strides)
    assert [tuple(c.shape) for c in codes] == [(B, 64 // s) for s in cfg.vq_strides] and excused <= R.EXCUSED_CAP * frames, (excused, frames)
    assert all(torch.equal(a[0], b[1]) for a, b in zip(m.encode(torch.tensor(x[1:])), codes))
