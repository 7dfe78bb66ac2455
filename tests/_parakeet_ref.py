"""Restatements of the Parakeet encoder's blocks (mlx_audio/stt/models/parakeet/attention.py, conformer.py) for the tests of csrc/kk_parakeet.hip:
numpy / torch on the CPU, float64 unless a dtype is asked for, written from the reference's semantics."""
import math

import numpy as np
import torch


def bf16_round(a):
    """float32 -> nearest-even bf16, returned as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def rel_shift(x):
    """attention.py:82-91, literally: pad one column on the left, view as [pos_len + 1][Tq], drop the first row, view as [Tq][pos_len]"""
    B, H, Tq, pos_len = x.shape
    x = np.pad(x, [(0, 0), (0, 0), (0, 0), (1, 0)])
    x = x.reshape(B, H, pos_len + 1, Tq)[:, :, 1:, :]
    return x.reshape(B, H, Tq, pos_len)


def rel_pos_attention(q, k, v, p, u, vb):
    """attention.py:113-135 in float64 on the kernel's operands: q, k, v [B][H][T][hd] and p [H][2T-1][hd] bf16-exact, u, vb fp32 [H][hd];
    q + u and q + v are taken in float32 and rounded to bf16 once (the operand contract).  Returns [B][H][T][hd]."""
    T, hd = q.shape[2], q.shape[3]
    q_u = bf16_round(q.astype(np.float32) + u[None, :, None, :].astype(np.float32)).astype(np.float64)
    q_v = bf16_round(q.astype(np.float32) + vb[None, :, None, :].astype(np.float32)).astype(np.float64)
    k, v, p = k.astype(np.float64), v.astype(np.float64), p.astype(np.float64)
    bd = rel_shift(q_v @ p[None].swapaxes(-2, -1))[:, :, :, :T]
    s = (q_u @ k.swapaxes(-2, -1) + bd) * hd ** -0.5
    s -= s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return (e / e.sum(axis=-1, keepdims=True)) @ v


def conv_core(x, dw_w, dw_b, bn_w, bn_b, mean, var, dtype=torch.float64, eps=1e-5):
    """conformer.py:83-87 between the two pointwise convs: x [B][T][2D] -> silu(batch_norm(depthwise_conv(glu(x)))) [B][T][D], BatchNorm in
    inference form and NOT folded.  dw_w [D][k], the rest [D]."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    x, dw_w = t(x), t(dw_w)
    D, k = dw_w.shape
    g = x[..., :D] * torch.sigmoid(x[..., D:])
    y = torch.nn.functional.conv1d(g.transpose(1, 2), dw_w[:, None, :], t(dw_b), padding=(k - 1) // 2, groups=D).transpose(1, 2)
    y = (y - t(mean)) / torch.sqrt(t(var) + eps) * t(bn_w) + t(bn_b)
    return (y * torch.sigmoid(y)).numpy()


def conv2d_s2(x, w, b, stem, dtype=torch.float64):
    """conformer.py:174-196: a 3 x 3, stride 2, padding 1 Conv2d over channels-last x.  stem: x [B][T][F], w [C][1][3][3], ReLU.  Otherwise
    x [B][T][F][C], depth-wise, no activation.  Returns [B][T'][F'][C]."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    x = t(x)[:, None] if stem else t(x).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, t(w), t(b), stride=2, padding=1, groups=1 if stem else w.shape[0])
    return (torch.relu(y) if stem else y).permute(0, 2, 3, 1).numpy()


def subsampled_lengths(lengths, factor):
    """conformer.py:241-248 in the reference's floating-point form"""
    n = np.asarray(lengths, dtype=np.float32)
    for _ in range(int(math.log(factor, 2))):
        n = np.floor((n + 2 * 1 - 3) / 2) + 1.0
    return n.astype(np.int32)


def rel_positions(T, d_model, max_len=5000):
    """attention.py:155-185: the table for max_len, then the slice the call takes for a sequence of T"""
    pos = np.arange(max_len - 1, -max_len, -1, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, d_model, 2, dtype=np.float64) * -(math.log(10000.0) / d_model))
    pe = np.zeros((2 * max_len - 1, d_model))
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe[pe.shape[0] // 2 - (T - 1) : pe.shape[0] // 2 + (T - 1) + 1]


# ---- the encoder as a small module (conformer.py:93-331), parameter names as in the reference; .bfloat16() gives the independent bf16 run -------------
class _Block(torch.nn.Module):
    def __init__(self, a):
        super().__init__()
        nn, D, b = torch.nn, a["d_model"], a.get("use_bias", True)
        ff = lambda: nn.ModuleDict(dict(linear1=nn.Linear(D, D * a["ff_expansion_factor"], bias=b), linear2=nn.Linear(D * a["ff_expansion_factor"], D, bias=b)))  # noqa: E731
        self.H, k = a["n_heads"], a["conv_kernel_size"]
        self.norm_feed_forward1, self.norm_self_att, self.norm_conv, self.norm_feed_forward2, self.norm_out = (nn.LayerNorm(D) for _ in range(5))
        self.feed_forward1, self.feed_forward2 = ff(), ff()
        self.self_attn = nn.ModuleDict({n: nn.Linear(D, D, bias=b and n != "linear_pos") for n in ("linear_q", "linear_k", "linear_v", "linear_out", "linear_pos")})
        self.self_attn.pos_bias_u, self.self_attn.pos_bias_v = (nn.Parameter(0.3 * torch.randn(self.H, D // self.H)) for _ in range(2))
        self.conv = nn.ModuleDict(dict(pointwise_conv1=nn.Conv1d(D, 2 * D, 1, bias=b), depthwise_conv=nn.Conv1d(D, D, k, padding=(k - 1) // 2, groups=D, bias=b),
                                       batch_norm=nn.BatchNorm1d(D), pointwise_conv2=nn.Conv1d(D, D, 1, bias=b)))

    def forward(self, x, pos):
        F, at = torch.nn.functional, self.self_attn
        for ff, ln in ((self.feed_forward1, self.norm_feed_forward1),):
            x = x + 0.5 * ff["linear2"](F.silu(ff["linear1"](ln(x))))
        h = self.norm_self_att(x)
        B, T, D = h.shape
        heads = lambda t: t.reshape(t.shape[0], -1, self.H, D // self.H)  # noqa: E731
        q, k, v, p = heads(at["linear_q"](h)), heads(at["linear_k"](h)), heads(at["linear_v"](h)), heads(at["linear_pos"](pos))
        bd = (q + at.pos_bias_v).transpose(1, 2) @ p.permute(0, 2, 3, 1)  # [B][H][T][2T-1]
        bd = F.pad(bd, (1, 0)).reshape(B, self.H, 2 * T, T)[:, :, 1:].reshape(B, self.H, T, 2 * T - 1)[..., :T]  # rel_shift, literally
        s = ((q + at.pos_bias_u).transpose(1, 2) @ k.permute(0, 2, 3, 1) + bd) * (D // self.H) ** -0.5
        x = x + at["linear_out"]((torch.softmax(s, -1) @ v.transpose(1, 2)).transpose(1, 2).reshape(B, T, D))
        c = self.conv
        h = F.glu(c["pointwise_conv1"](self.norm_conv(x).transpose(1, 2)), dim=1)
        x = x + c["pointwise_conv2"](F.silu(c["batch_norm"](c["depthwise_conv"](h)))).transpose(1, 2)
        ff = self.feed_forward2
        x = x + 0.5 * ff["linear2"](F.silu(ff["linear1"](self.norm_feed_forward2(x))))
        return self.norm_out(x)


class Encoder(torch.nn.Module):
    def __init__(self, a, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        nn, Cc, self.a = torch.nn, a["subsampling_conv_channels"], a
        conv, f = [nn.Conv2d(1, Cc, 3, 2, 1), nn.ReLU()], a["feat_in"]
        for _ in range(int(math.log2(a["subsampling_factor"])) - 1):
            conv += [nn.Conv2d(Cc, Cc, 3, 2, 1, groups=Cc), nn.Conv2d(Cc, Cc, 1), nn.ReLU()]
        for _ in range(int(math.log2(a["subsampling_factor"]))):
            f = (f - 1) // 2 + 1
        self.pre_encode = nn.ModuleDict(dict(conv=nn.Sequential(*conv), out=nn.Linear(Cc * f, a["d_model"])))
        self.layers = nn.ModuleList(_Block(a) for _ in range(a["n_layers"]))
        for m in self.modules():  # non-trivial BatchNorm statistics and LayerNorm parameters
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 2.0), m.weight.data.normal_(1, 0.2), m.bias.data.normal_(0, 0.2)
            if isinstance(m, nn.LayerNorm):
                m.weight.data.normal_(1, 0.1), m.bias.data.normal_(0, 0.1)
        self.eval()

    @torch.no_grad()
    def forward(self, mel):
        dt = self.pre_encode["out"].weight.dtype
        x = self.pre_encode["conv"](mel.to(dt)[:, None])  # [B][C][T'][F']
        x = self.pre_encode["out"](x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1))
        x = x * math.sqrt(self.a["d_model"]) if self.a.get("xscaling", False) else x
        pos = torch.from_numpy(rel_positions(x.shape[1], self.a["d_model"])).to(dt)[None]
        for layer in self.layers:
            x = layer(x, pos)
        return x.float()

    def weights(self):
        return {"encoder." + k: v.detach().float().numpy() for k, v in self.state_dict().items() if "num_batches" not in k}


# ---- features (parakeet/audio.py:38-70, mlx_audio/utils.py stft and mel_filters) ------------------------------------------------------------------
def log_mel(x, sample_rate, n_fft, win, hop, features, per_feature, pad_to=0, pad_value=0.0, dtype=np.float64):
    """[1 + n // hop][features] with a direct DFT (frames @ cos, no FFT), every operation in `dtype`"""
    x = np.asarray(x, dtype=dtype)
    if pad_to > len(x):
        x = np.concatenate([x, np.full(pad_to - len(x), pad_value, dtype)])
    w = np.concatenate([0.5 * (1 - np.cos(2 * math.pi * np.arange(win) / (win - 1))), np.zeros(n_fft - win)]).astype(dtype)  # zero-padded at its end
    p = n_fft // 2
    x = np.concatenate([x[1 : p + 1][::-1], x, x[-(p + 1) : -1][::-1]])
    frames = np.lib.stride_tricks.sliding_window_view(x, n_fft)[::hop] * w
    ang = 2 * math.pi * np.outer(np.arange(n_fft), np.arange(n_fft // 2 + 1)) / n_fft
    power = (frames @ np.cos(ang).astype(dtype)) ** 2 + (frames @ np.sin(ang).astype(dtype)) ** 2
    f_sp, logstep = 200.0 / 3, math.log(6.4) / 27.0  # mel_scale=None: Slaney's scale; norm="per_feature" / anything but "slaney": no area normalisation
    to_mel = lambda f: 15.0 + math.log(f / 1000.0) / logstep if f >= 1000.0 else f / f_sp  # noqa: E731
    mels = np.linspace(to_mel(0.0), to_mel(sample_rate / 2), features + 2)
    pts = np.where(mels >= 15.0, 1000.0 * np.exp(logstep * (mels - 15.0)), f_sp * mels)
    slopes = pts[None, :] - np.linspace(0, sample_rate // 2, n_fft // 2 + 1)[:, None]
    bank = np.maximum(0.0, np.minimum(-slopes[:, :-2] / (pts[1:] - pts[:-1])[:-1], slopes[:, 2:] / (pts[1:] - pts[:-1])[1:])).astype(dtype)
    lg = np.log(power @ bank + dtype(1e-5))
    ax = 0 if per_feature else None
    return ((lg - lg.mean(axis=ax, keepdims=True)) / (lg.std(axis=ax, keepdims=True) + dtype(1e-5))).astype(dtype)


def signal(n, seed):
    """a chirp under an envelope plus noise, float32"""
    g, t = np.random.default_rng(seed), np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * math.pi * (200.0 + 1500.0 * t) * t) * (0.5 + 0.5 * np.cos(7.0 * t)) + 0.02 * g.standard_normal(n)).astype(np.float32)
