"""SNAC with LocalMHA, no GPU: the float64 reference of tests/_snac_attn_ref.py against an independent torch restatement
(scaled_dot_product_attention per window on rotary-embedded inputs), the opt-in surface, and the pinned encode inputs."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import _snac_attn_ref as A
import _snac_ref as R
from mlx_audio_amd import _lib, snac


def mha_torch(w, p, x, dtype):
    """LocalMHA on x [B][T][D] as the torch code the reference was translated from computes it (rotate_half drops the split axis)."""
    t = lambda n: torch.tensor(np.asarray(w[p + n], np.float64)).to(dtype)
    (B, T, D), rot = x.shape, lambda u: torch.cat([-u[..., 32:], u[..., :32]], -1)
    n = TF.layer_norm(x, (D,), t(".norm.weight"), t(".norm.bias"), 1e-5)
    q, k, v = (u.reshape(B, T // 32, 32, D // 64, 64).transpose(2, 3) for u in TF.linear(n, t(".to_qkv.weight")).chunk(3, -1))
    f = torch.arange(32, dtype=dtype)[:, None] * (1.0 / 10000 ** (torch.arange(0, 64, 2, dtype=dtype) / 64))
    f = torch.cat([f, f], -1)
    q, k = q * f.cos() + rot(q) * f.sin(), k * f.cos() + rot(k) * f.sin()
    return TF.linear(TF.scaled_dot_product_attention(q, k, v).transpose(2, 3).reshape(B, T, D), t(".to_out.weight")) + x


def encode_torch(w, cfg, audio, dtype):
    """SNAC.encode with LocalMHA on torch.nn.functional in `dtype`: (codes, the attention block's output [B][T][D])."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)

    def cv(x, p, **kw):
        v, g = t(w[p + ".weight_v"]), t(w[p + ".weight_g"])
        return TF.conv1d(x, (g * v / torch.sqrt((v**2).sum(dim=(1, 2), keepdim=True))).permute(0, 2, 1).contiguous(), t(w[p + ".bias"]), **kw)

    def sn(x, p):
        a = t(w[p + ".alpha"]).reshape(1, -1, 1)
        return x + (1.0 / (a + 1e-9)) * torch.sin(a * x) ** 2

    e, n, a = "encoder.block.layers.", len(cfg.encoder_rates), np.asarray(audio, np.float64)
    y = cv(t(np.pad(a, [(0, 0), (0, 0), (0, A.preprocess_length(cfg, a.shape[-1]) - a.shape[-1])])), e + "0", padding=3)
    for l, s in enumerate(cfg.encoder_rates):
        p = f"{e}{l + 1}.block.layers."
        for i, dil in enumerate((1, 3, 9)):
            b = f"{p}{i}.block.layers."
            y = y + cv(sn(cv(sn(y, b + "0"), b + "1", padding=3 * dil, dilation=dil, groups=y.shape[1]), b + "2"), b + "3")
        y = cv(sn(y, p + "3"), p + "4", stride=s, padding=math.ceil(s / 2))
    att = mha_torch(w, f"{e}{n + 1}", y.permute(0, 2, 1), dtype)
    residual, codes = cv(att.permute(0, 2, 1), f"{e}{n + 2}", padding=3, groups=y.shape[1]), []
    for i, s in enumerate(cfg.vq_strides):
        q = f"quantizer.quantizers.{i}"
        ze, cb = cv(TF.avg_pool1d(residual, s) if s > 1 else residual, q + ".in_proj"), t(w[q + ".codebook.weight"])
        en, cn = TF.normalize(ze.permute(0, 2, 1), dim=-1, eps=1e-12), TF.normalize(cb, dim=-1, eps=1e-12)
        codes.append(torch.argmax(-((en**2).sum(-1, keepdim=True) - 2 * en @ cn.T + (cn**2).sum(-1)), dim=-1))
        residual = residual - cv(ze + (cb[codes[-1]].permute(0, 2, 1) - ze), q + ".out_proj").repeat_interleave(s, dim=2)
    return [c.numpy() for c in codes], att.numpy()


@pytest.mark.parametrize("case", sorted(A.ENCODE_CASES))
def test_reference_matches_torch_and_float32_stays_under_the_cap(case):
    B, N, seed = A.ENCODE_CASES[case]
    cfg = snac.SNACConfig(**A.CONFIGS[128])
    w = A.synth_weights(snac.param_shapes(cfg, local_attention=True), A.WEIGHT_SEED)
    x = R.audio(B, N, seed)
    codes, trace, z, att = A.encode(R.Weights(w), cfg, x)
    c64, a64 = encode_torch(w, cfg, x, torch.float64)
    assert att.shape == (B, 64, 64) and np.abs(a64 - att).max() <= 1e-12 * np.abs(att).max() and all(np.array_equal(a, b) for a, b in zip(c64, codes))
    excused, frames = R.excused_frames(encode_torch(w, cfg, x, torch.float32)[0], codes, trace, cfg.vq_strides)
    assert excused <= R.EXCUSED_CAP * frames, (excused, frames)


def test_opt_in_surface():
    cfg, base = snac.SNACConfig(**A.CONFIGS[128]), snac.SNACConfig(**dict(A.CONFIGS[128], attn_window_size=None))
    with pytest.raises(NotImplementedError, match="local_attention=True"):
        snac.SNAC(cfg)
    with pytest.raises(NotImplementedError, match="attn_window_size=16"):
        snac.SNAC(snac.SNACConfig(**dict(A.CONFIGS[128], attn_window_size=16)), local_attention=True)
    with pytest.raises(ValueError, match="multiples of 64"):
        snac.param_shapes(snac.SNACConfig(**dict(A.CONFIGS[128], decoder_dim=96)), local_attention=True)
    assert snac.param_shapes(base, local_attention=True) == snac.param_shapes(base) and snac.snac_44khz() == snac.SNACConfig()
    names, plain = snac.param_shapes(cfg, local_attention=True), snac.param_shapes(base)
    assert names["encoder.block.layers.3.to_qkv.weight"] == (192, 64) and names["decoder.model.layers.2.to_out.weight"] == (128, 128)
    assert names["encoder.block.layers.3.norm.bias"] == (64,) and names["encoder.block.layers.4.weight_v"] == plain["encoder.block.layers.3.weight_v"]
    assert names["decoder.model.layers.3.block.layers.1.weight_v"] == plain["decoder.model.layers.2.block.layers.1.weight_v"]
    assert names["decoder.model.layers.6.weight_v"] == (1, 7, 32) and len(names) == len(plain) + 8
    big = snac.param_shapes(snac.snac_44khz(), local_attention=True)
    assert big["decoder.model.layers.2.to_qkv.weight"] == (4608, 1536) and big["encoder.block.layers.5.to_qkv.weight"] == (3072, 1024)
    m = snac.SNAC(cfg, local_attention=True)  # (kk_snac_create_attn; no weights, no GPU)
    assert m.pad_to() == 4 * 32 == A.preprocess_length(cfg, 1) and snac.SNAC(base, local_attention=True).pad_to() == 8
    assert m.preprocess(torch.zeros(2, 1, 201)).shape == (2, 1, 256)
    m._final = True  # (the length check of decode comes before anything touches the device)
    with pytest.raises(ValueError, match="attention window"):
        m.decode([torch.zeros(1, 24, dtype=torch.int32), torch.zeros(1, 48, dtype=torch.int32)])
    lib, kc, h = _lib.load(), _lib.KKSnacConfig(), C.c_void_p()
    kc.encoder_dim, kc.latent_dim, kc.decoder_dim, kc.codebook_size, kc.codebook_dim, kc.depthwise, kc.attn_window_size = 16, 64, 128, 64, 8, 1, 32
    kc.n_encoder_rates = kc.n_decoder_rates = kc.n_vq = kc.vq_strides[0] = 1
    kc.encoder_rates[0] = kc.decoder_rates[0] = 2
    assert lib.kk_snac_create(C.byref(kc), C.byref(h)) != 0 and lib.kk_snac_create_attn(C.byref(kc), C.byref(h)) == 0
    lib.kk_snac_destroy(h)
    kc.attn_window_size = 16
    assert lib.kk_snac_create_attn(C.byref(kc), C.byref(h)) != 0 and b"attn_window_size 16" in lib.kk_last_error()
