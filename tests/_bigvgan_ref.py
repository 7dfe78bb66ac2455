"""float64 restatement of the reference's BigVGAN (mlx_audio/codec/models/bigvgan), written the reference's way on torch-CPU: Activation1d as
edge pad, depth-wise transposed conv, slice, SnakeBeta, edge pad, strided depth-wise conv; weight-normed convs; the AMP blocks; the forward."""
import math

import numpy as np
import torch
import torch.nn.functional as F

TINY = dict(num_mels=8, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=64, resblock="1", resblock_kernel_sizes=[3, 7, 11],
            resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation="snakebeta", snake_logscale=True)


def kaiser_sinc(cutoff=0.25, half_width=0.3, K=12):  # resample.py:17-46
    half = K // 2
    A = 2.285 * (half - 1) * math.pi * 4 * half_width + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21) ** 0.4 + 0.07886 * (A - 21) if A >= 21 else 0.0)
    time = np.arange(-half, half) + 0.5 if K % 2 == 0 else np.arange(K) - half
    f = 2 * cutoff * np.kaiser(K, beta) * np.sinc(2 * cutoff * time)
    return f / f.sum()


def activation1d(x, alpha, beta, logscale):
    """x [B][L][C] -> [B][L][C] (resample.py:157-177 around activation.py:42-51)"""
    x = torch.as_tensor(np.asarray(x, np.float64)).permute(0, 2, 1)
    Cn = x.shape[1]
    f = torch.as_tensor(kaiser_sinc()).expand(Cn, 1, 12)
    a, b = (torch.as_tensor(np.asarray(v, np.float64)).reshape(1, Cn, 1) for v in (alpha, beta))
    if logscale:
        a, b = a.exp(), b.exp()
    u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), f, stride=2, groups=Cn)[..., 15:-15]  # UpSample1d: pad 5, pad_left = pad_right = 15
    u = u + (1.0 / (b + 1e-9)) * torch.sin(u * a) ** 2
    y = F.conv1d(F.pad(u, (5, 6), mode="replicate"), f, stride=2, groups=Cn)  # LowPassFilter1d: pad_left 5, pad_right 6
    return y.permute(0, 2, 1).numpy()


def _wn(W, p, keep):  # conv.py:7-12: g v / |v|, the norm over the axes except `keep`
    v, g = (torch.as_tensor(np.asarray(W[p + s], np.float64)) for s in (".weight_v", ".weight_g"))
    return g * v / v.pow(2).sum(tuple(i for i in range(3) if i != keep), keepdim=True).sqrt()


def conv(W, p, x, dil=1):  # WNConv1d, x [B][C][L], "same" padding
    w = _wn(W, p, 0).permute(0, 2, 1)
    b = torch.as_tensor(np.asarray(W[p + ".bias"], np.float64)) if p + ".bias" in W else None
    return F.conv1d(x, w, b, padding=(w.shape[2] - 1) * dil // 2, dilation=dil)


def forward(W, cfg, mel):
    """mel [B][num_mels][T] -> (pcm [B][1][N], {name: [B][L][C]}) as BigVGAN.__call__ (bigvgan.py:97-122)"""
    stages = {}
    keep = lambda name, t: stages.__setitem__(name, t.permute(0, 2, 1).numpy())
    act = lambda p, t: torch.as_tensor(activation1d(t.permute(0, 2, 1).numpy(), W[p + ".act.alpha"], W[p + ".act.beta"], cfg.snake_logscale)).permute(0, 2, 1)
    x = conv(W, "conv_pre", torch.as_tensor(np.asarray(mel, np.float64)))
    keep("conv_pre", x)
    nk = len(cfg.resblock_kernel_sizes)
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        p = f"ups.{i}.0"
        x = F.conv_transpose1d(x, _wn(W, p, 2).permute(2, 0, 1), torch.as_tensor(np.asarray(W[p + ".bias"], np.float64)), stride=u, padding=(k - u) // 2)
        xs = 0
        for j, dils in enumerate(cfg.resblock_dilation_sizes):
            p, y = f"resblocks.{i * nk + j}", x
            for m, d in enumerate(dils):
                if str(cfg.resblock) == "1":
                    y = y + conv(W, f"{p}.convs2.{m}", act(f"{p}.activations.{2 * m + 1}", conv(W, f"{p}.convs1.{m}", act(f"{p}.activations.{2 * m}", y), d)))
                else:
                    y = y + conv(W, f"{p}.convs.{m}", act(f"{p}.activations.{m}", y), d)
            xs = xs + y
        x = xs / nk
        keep(f"stage{i}", x)
    x = act("activation_post", x)
    keep("activation_post", x)
    x = conv(W, "conv_post", x)
    return (torch.tanh(x) if cfg.use_tanh_at_final else x.clamp(-1.0, 1.0)).numpy(), stages


def synth_weights(shapes, seed=0):
    """seeded parameters for `param_shapes`: unit-gain convs, the residual branches and the last conv damped, alpha / beta in [-0.5, 0.5]"""
    rng, w = np.random.default_rng(seed), {}
    for name, shape in shapes.items():
        if name.endswith(".weight_v"):
            v = rng.standard_normal(shape) / math.sqrt(shape[1] * shape[2])
            g = w[name[:-1] + "g"] = np.empty(shapes[name[:-1] + "g"], np.float32)
            gain = 0.3 if ".convs" in name else (0.5 if name.startswith("conv_post") else 1.0)
            g[...] = gain * np.sqrt((v**2).sum(axis=tuple(i for i in range(3) if g.shape[i] == 1), keepdims=True)) * rng.uniform(0.8, 1.2, g.shape)
        elif name.endswith(".weight_g"):
            continue
        elif name.endswith(".filter"):
            v = kaiser_sinc().reshape(shape)
        elif name.endswith((".alpha", ".beta")):
            v = rng.uniform(-0.5, 0.5, shape)
        else:
            v = 0.05 * rng.standard_normal(shape)
        w[name] = v.astype(np.float32)
    return w
