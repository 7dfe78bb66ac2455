"""Float64 numpy restatement of SNAC with LocalMHA (mlx_audio/codec/models/snac/attention.py; layers.py:147-152, 185-194), composed from the
primitives of tests/_snac_ref.py.  rotate_half is NOT the reference's as written (its mx.split keeps the split axis and the result does not
broadcast): rot(u)[c] = -u[c + 32] for c < 32, u[c - 32] otherwise.  tests/test_snac_attn_cpu.py pins these functions against torch."""
import math

import numpy as np

import _snac_ref as R
from _snac_ref import F64

CONFIGS = {d: dict(sampling_rate=44100, encoder_dim=16, encoder_rates=[2, 2], latent_dim=64, decoder_dim=d, decoder_rates=[2, 2], attn_window_size=32,
                   codebook_size=64, codebook_dim=8, vq_strides=[2, 1], noise=True) for d in (128, 192)}  # heads: 1 (encoder), 2 / 3 (decoder)
# encode inputs (B, N, seed): N = 201 is padded to 256 = hop 4 * lcm(2, 1, 32).  Seeds pinned by test_snac_attn_cpu.py (float32 under the cap).
WEIGHT_SEED, ENCODE_CASES = 7, {"even": (2, 256, 21), "unpadded": (2, 201, 22)}


def rope(u):
    """Step 4 on u [..., W, 64]: position i = 0 .. W - 1 inside the window, angle(i, c) = i * 10000^(-2 (c mod 32) / 64)."""
    th = np.arange(u.shape[-2], dtype=F64)[:, None] * 10000.0 ** (-np.arange(0, 64, 2, dtype=F64) / 64)
    th = np.concatenate([th, th], -1)
    return u * np.cos(th) + np.concatenate([-u[..., 32:], u[..., :32]], -1) * np.sin(th)


def attention(qkv, window=32):
    """Steps 3-6: qkv [B][T][3 D] (q | k | v, heads of 64 channels) -> o [B][T][D]."""
    qkv = np.asarray(qkv, F64)
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    q, k, v = (qkv[..., i * D : (i + 1) * D].reshape(B, T // window, window, D // 64, 64).transpose(0, 3, 1, 2, 4) for i in range(3))
    s = rope(q) @ rope(k).swapaxes(-1, -2) / 8.0
    p = np.exp(s - s.max(-1, keepdims=True))
    return ((p / p.sum(-1, keepdims=True)) @ v).transpose(0, 2, 3, 1, 4).reshape(B, T, D)


def local_mha(W, p, x, window=32):
    """The seven steps on x [B][T][D]."""
    x, g = np.asarray(x, F64), lambda n: np.asarray(W.w[p + n], F64)
    mu = x.mean(-1, keepdims=True)
    n = (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * g(".norm.weight") + g(".norm.bias")
    return attention(n @ g(".to_qkv.weight").T, window) @ g(".to_out.weight").T + x


def encoder(W, cfg, x):
    """layers.py:133-156 with LocalMHA as layer n + 1: x [B][N][1] -> ([B][T][latent], the attention block's output)."""
    e, n = "encoder.block.layers.", len(cfg.encoder_rates)
    y = R.conv(x, W.wn(e + "0"), W.bias(e + "0"), pad=3)
    for l, s in enumerate(cfg.encoder_rates):
        p = f"{e}{l + 1}.block.layers."
        for i, dil in enumerate((1, 3, 9)):
            y = R.residual_unit(W, p + str(i), y, dil)
        y = R.conv(R.snake(y, W.alpha(p + "3")), W.wn(p + "4"), W.bias(p + "4"), stride=s, pad=math.ceil(s / 2))
    a = local_mha(W, f"{e}{n + 1}", y, cfg.attn_window_size)
    return R.dw_conv(a, W.wn(f"{e}{n + 2}"), W.bias(f"{e}{n + 2}")), a


def decoder(W, cfg, z, noise):
    """layers.py:159-205 with LocalMHA as layer 2: (audio [B][N][1], {"decoder_attn", "block0", ...})."""
    m, n = "decoder.model.layers.", len(cfg.decoder_rates)
    y = R.conv(R.dw_conv(z, W.wn(m + "0"), W.bias(m + "0")), W.wn(m + "1"), W.bias(m + "1"))
    y = local_mha(W, m + "2", y, cfg.attn_window_size)
    stages = {"decoder_attn": y}
    for l, s in enumerate(cfg.decoder_rates):
        p = f"{m}{l + 3}.block.layers."
        y = R.conv_transposed(R.snake(y, W.alpha(p + "0")), W.wn(p + "1"), W.bias(p + "1"), stride=s, pad=math.ceil(s / 2))
        if cfg.noise:
            y = y + np.asarray(noise[l], F64) * R.conv(y, W.wn(p + "2.linear"))
        for i, dil in enumerate((1, 3, 9)):
            y = R.residual_unit(W, p + str(i + (3 if cfg.noise else 2)), y, dil)
        stages[f"block{l}"] = y
    return R.conv_cout1(y, W.wn(f"{m}{n + 4}"), W.bias(f"{m}{n + 4}"), pad=3, alpha=W.alpha(f"{m}{n + 3}"), tanh=True)[..., None], stages


def preprocess_length(cfg, n, window=32):
    unit = math.lcm(*cfg.vq_strides, window) * int(np.prod(cfg.encoder_rates))
    return math.ceil(n / unit) * unit


def encode(W, cfg, audio):
    """SNAC.encode: (codes, trace, encoder output, attention block's output)."""
    a = np.asarray(audio, F64)
    a = np.pad(a, [(0, 0), (0, 0), (0, preprocess_length(cfg, a.shape[-1], cfg.attn_window_size) - a.shape[-1])])
    z, att = encoder(W, cfg, np.moveaxis(a, 1, 2))
    _, codes, trace = R.quantizer(W, cfg, z)
    return codes, trace, z, att


def synth_weights(shapes, seed):
    """_snac_ref.synth_weights, the attention matrices redrawn as N(0, 1 / D) and norm.weight around 1: a softmax neither flat nor one-hot."""
    w, rng = R.synth_weights(shapes, seed), np.random.default_rng(seed + 1000)
    for name, shape in shapes.items():
        if name.endswith(("to_qkv.weight", "to_out.weight")):
            w[name] = (rng.standard_normal(shape) / math.sqrt(shape[1])).astype(np.float32)
        elif name.endswith("norm.weight"):
            w[name] = rng.uniform(0.8, 1.2, shape).astype(np.float32)
    return w
