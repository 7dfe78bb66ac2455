"""float64 numpy restatement of the reference's Vocos decode path (mlx_audio/codec/models/vocos/vocos.py, utils.istft), written the reference's way:
zero-padded depth-wise conv, LayerNorm / AdaLayerNorm, the ConvNeXt blocks, ISTFTHead as exp / clip / cos / sin, irfft, Hann, overlap-add."""
import math

import numpy as np
from scipy.special import erf

TINY = dict(input_channels=24, dim=40, intermediate_dim=72, num_layers=2, n_fft=256, hop_length=64)
TINY_ADA = dict(TINY, adanorm_num_embeddings=4)


def layer_norm(x, eps=1e-6):
    m = x.mean(-1, keepdims=True)
    return (x - m) / np.sqrt(((x - m) ** 2).mean(-1, keepdims=True) + eps)


def conv1d(x, w, b, groups=1):
    """mx.conv1d with padding (K - 1) / 2: x [B][T][Cin], w [O][K][Cin / groups] -> [B][T][O]"""
    K, T = w.shape[1], x.shape[1]
    xp = np.pad(x, ((0, 0), (K // 2, K // 2), (0, 0)))
    if groups == 1:
        return sum(xp[:, k : k + T] @ w[:, k].T for k in range(K)) + b
    return sum(xp[:, k : k + T] * w[:, k, 0] for k in range(K)) + b


def dwconv_ln(x, w, b, ln_w=None, ln_b=None, eps=1e-6, scale_shift=None):
    """x [B][T][C], w [C][7][1] -> LN(dwconv(x)) * ln_w + ln_b, or * scale[b] + shift[b] with scale_shift [B][2][C]"""
    y = layer_norm(conv1d(np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64), groups=x.shape[-1]), eps)
    if scale_shift is not None:
        ss = np.asarray(scale_shift, np.float64)
        return y * ss[:, None, 0] + ss[:, None, 1]
    return y * (1.0 if ln_w is None else np.asarray(ln_w, np.float64)) + (0.0 if ln_b is None else np.asarray(ln_b, np.float64))


def hanning(n):  # utils.hanning: the symmetric form
    return 0.5 * (1 - np.cos(2 * np.pi * np.arange(n) / (n - 1)))


def istft_head(h, n_fft, hop):
    """h [B][T][>= n_fft + 2] -> (audio [B][(T - 1) hop], share of the bins whose magnitude took the clip at 100)"""
    h = np.asarray(h, np.float64)
    B, T, F = h.shape[0], h.shape[1], n_fft // 2 + 1
    mag, p = np.exp(h[..., :F]), h[..., F : 2 * F]
    S = np.minimum(mag, 1e2) * (np.cos(p) + 1j * np.sin(p))
    frames, w = np.fft.irfft(S, n=n_fft, axis=-1), hanning(n_fft)
    y, ws = np.zeros((B, (T - 1) * hop + n_fft)), np.zeros((T - 1) * hop + n_fft)
    for f in range(T):
        y[:, f * hop : f * hop + n_fft] += frames[:, f] * w
        ws[f * hop : f * hop + n_fft] += w
    y = np.where(ws != 0, y / np.where(ws != 0, ws, 1.0), y)
    return y[:, n_fft // 2 : -(n_fft // 2)], float((mag > 1e2).mean())


def forward(W, cfg, features, cond=None):
    """features [B][T][input_channels], cond [B][num_embeddings] -> (pcm [B][(T - 1) hop], {stage: [B][T][C]}) as Vocos.decode (vocos.py:351-354)"""
    g = lambda k: np.asarray(W[k], np.float64)
    stages = {}

    def norm(p, x):
        if cfg.adanorm_num_embeddings:
            c = np.asarray(cond, np.float64)
            return layer_norm(x) * (c @ g(p + ".scale.weight").T + g(p + ".scale.bias"))[:, None] + (c @ g(p + ".shift.weight").T + g(p + ".shift.bias"))[:, None]
        return layer_norm(x) * g(p + ".weight") + g(p + ".bias")

    x = conv1d(np.asarray(features, np.float64), g("backbone.embed.weight"), g("backbone.embed.bias"))
    stages["embed"] = x
    x = norm("backbone.norm", x)
    for i in range(cfg.num_layers):
        p = f"backbone.convnext.{i}"
        y = norm(p + ".norm", conv1d(x, g(p + ".dwconv.weight"), g(p + ".dwconv.bias"), groups=cfg.dim))
        y = y @ g(p + ".pwconv1.weight").T + g(p + ".pwconv1.bias")
        y = 0.5 * y * (1 + erf(y / math.sqrt(2)))
        x = x + g(p + ".gamma") * (y @ g(p + ".pwconv2.weight").T + g(p + ".pwconv2.bias"))
        stages[f"block{i}"] = x
    x = layer_norm(x) * g("backbone.final_layer_norm.weight") + (g("backbone.final_layer_norm.bias") if cfg.bias else 0.0)
    stages["backbone"] = x
    stages["head"] = x @ g("head.out.weight").T + g("head.out.bias")
    return istft_head(stages["head"], cfg.n_fft, cfg.hop_length)[0], stages


def synth_weights(shapes, seed=0):
    """seeded parameters for `param_shapes`: unit-gain matrices, norm weights around 1, gamma around 0.5; the head's magnitude rows damped so that
    exp stays well under the clip and its phase rows at unit gain"""
    rng, w = np.random.default_rng(seed), {}
    for name, shape in shapes.items():
        if name.endswith(".weight") and len(shape) >= 2:
            v = rng.standard_normal(shape) / math.sqrt(np.prod(shape[1:]))
            if name == "head.out.weight":
                v[: shape[0] // 2] *= 0.5
        elif name.endswith((".norm.weight", "_norm.weight", ".scale.bias")):
            v = rng.uniform(0.8, 1.2, shape)
        elif name.endswith(".gamma"):
            v = rng.uniform(0.3, 0.7, shape)
        else:
            v = 0.1 * rng.standard_normal(shape)
        w[name] = v.astype(np.float32)
    return w
