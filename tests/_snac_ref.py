"""Float64 numpy restatement of the reference's SNAC codec (mlx_audio/codec/models/snac/{snac,layers,vq}.py) and of every operation a
kernel of mlx-audio_amd/csrc/kk_snac.hip performs, one function each.  Tensors are channels-last [B][L][C] as in the reference.  The
restatement follows the PORT as written, not upstream PyTorch SNAC: no output padding on transposed convs (layers.py:105-121), NoiseBlock
noise of shape [B][1][C] (layers.py:261-267), a no-op residual crop (layers.py:226-231).  Noise is always explicit.
tests/test_snac_ref_cpu.py pins these functions against torch.nn.functional in float64."""
import math

import numpy as np

F64 = np.float64


def bf16_round(a):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def near_bf16_tie(e, rel=2.0**-14):
    """True where the float64 value e lies within rel * |e| of the midpoint of two neighbouring bf16 values."""
    e = np.asarray(e, F64)
    lo = bf16_round(e.astype(np.float32)).astype(F64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(e), 1e-30))) - 7)
    frac = np.abs(np.abs(e - lo) / ulp - 0.5)  # lo is the NEAREST bf16: distance to it is <= ulp / 2; a tie has it == ulp / 2
    return frac < rel * np.abs(e) / ulp + 1e-12


# ------------------------------------------------------------------------------------------------ layers.py
def weight_norm(g, v):
    """layers.py:9-14,57: g v / |v| over the axes except 0."""
    v = np.asarray(v, F64)
    n = np.sqrt((v**2).sum(axis=tuple(range(1, v.ndim)), keepdims=True))
    return np.asarray(g, F64).reshape((-1,) + (1,) * (v.ndim - 1)) * v / n


def snake(x, alpha):
    """layers.py:124-130: x + sin^2(alpha x) / (alpha + 1e-9); alpha [C] (the module's (1, C, 1) flattened)."""
    a = np.asarray(alpha, F64).reshape(-1)
    x = np.asarray(x, F64)
    return x + (1.0 / (a + 1e-9)) * np.sin(a * x) ** 2


def conv(x, w, bias=None, *, stride=1, pad=0, dil=1, absum=False):
    """mx.conv1d, groups = 1 (layers.py:58): x [B][L][I], w [O][K][I] -> [B][(L + 2 pad - dil (K - 1) - 1) / stride + 1][O].
    absum: also sum |x| |w| (+ |bias|) per output, the rounding scale of the accumulation."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    B, L, I = x.shape
    O, K, _ = w.shape
    Lo = (L + 2 * pad - dil * (K - 1) - 1) // stride + 1
    xp = np.zeros((B, L + 2 * pad, I), F64)
    xp[:, pad : pad + L] = x
    y, s = np.zeros((B, Lo, O), F64), np.zeros((B, Lo, O), F64)
    for k in range(K):
        xs = xp[:, k * dil : k * dil + (Lo - 1) * stride + 1 : stride]
        y += xs @ w[:, k, :].T
        if absum:
            s += np.abs(xs) @ np.abs(w[:, k, :]).T
    if bias is not None:
        y += np.asarray(bias, F64)
        s += np.abs(np.asarray(bias, F64))
    return (y, s) if absum else y


def dw_conv(x, w, bias=None, *, dil=1, alpha_in=None, alpha_out=None, absum=False):
    """Depth-wise mx.conv1d (groups = C), K taps, pad = (K - 1) dil / 2 (layers.py:211-221), with the Snakes a fused kernel applies around
    it: out = snake_out?(sum_k w[c][k] snake_in?(x[t - pad + k dil][c]) + bias[c]).  x [B][L][C], w [C][K][1].  With absum the rounding
    scale of the sum BEFORE the output Snake is returned too."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    B, L, C = x.shape
    K = w.shape[1]
    pad = (K - 1) * dil // 2
    if alpha_in is not None:
        x = snake(x, alpha_in)
    xp = np.zeros((B, L + 2 * pad, C), F64)
    xp[:, pad : pad + L] = x
    y, s = np.zeros((B, L, C), F64), np.zeros((B, L, C), F64)
    for k in range(K):
        y += xp[:, k * dil : k * dil + L] * w[:, k, 0]
        s += np.abs(xp[:, k * dil : k * dil + L] * w[:, k, 0])
    if bias is not None:
        y += np.asarray(bias, F64)
        s += np.abs(np.asarray(bias, F64))
    pre = y
    if alpha_out is not None:
        y = snake(y, alpha_out)
    return (y, s, pre) if absum else y


def conv_transposed(x, w, bias=None, *, stride, pad, absum=False):
    """mx.conv_transpose1d WITHOUT output padding (layers.py:105-121): x [B][L][I], w [I][K][O] (the module's layout) ->
    [B][(L - 1) stride - 2 pad + K][O]; out[p] sums x[t] w[:, k, :] over t stride + k - pad == p."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    B, L, I = x.shape
    _, K, O = w.shape
    full, fs = np.zeros((B, (L - 1) * stride + K, O), F64), np.zeros((B, (L - 1) * stride + K, O), F64)
    for k in range(K):
        full[:, k : k + (L - 1) * stride + 1 : stride] += x @ w[:, k, :]
        if absum:
            fs[:, k : k + (L - 1) * stride + 1 : stride] += np.abs(x) @ np.abs(w[:, k, :])
    y, s = full[:, pad : full.shape[1] - pad], fs[:, pad : full.shape[1] - pad]
    if bias is not None:
        y = y + np.asarray(bias, F64)
        s = s + np.abs(np.asarray(bias, F64))
    return (y, s) if absum else y


def conv_cout1(x, w, bias, *, pad, alpha=None, tanh=False, absum=False):
    """The decoder's last conv (layers.py:196-200): Snake, conv to one channel, tanh.  x [B][L][C], w [1][K][C] -> [B][L]."""
    xs = snake(x, alpha) if alpha is not None else np.asarray(x, F64)
    r = conv(xs, w, bias, pad=pad, absum=absum)
    y, s = (r[0][..., 0], r[1][..., 0]) if absum else (r[..., 0], None)
    pre = y
    if tanh:
        y = np.tanh(y)
    return (y, s, pre) if absum else y


class Weights:
    """A checkpoint in the reference's names and layouts, with weight norm folded on demand."""

    def __init__(self, w):
        self.w = w

    def alpha(self, p):
        return np.asarray(self.w[p + ".alpha"], F64).reshape(-1)

    def wn(self, p):
        return weight_norm(self.w[p + ".weight_g"], self.w[p + ".weight_v"])

    def bias(self, p):
        b = self.w.get(p + ".bias")
        return None if b is None else np.asarray(b, F64)


def residual_unit(W, p, x, dil):
    """layers.py:208-231 (depth-wise): x + conv1x1(snake(dw7(snake(x)))); the crop is a no-op."""
    b = p + ".block.layers."
    d = dw_conv(x, W.wn(b + "1"), W.bias(b + "1"), dil=dil, alpha_in=W.alpha(b + "0"), alpha_out=W.alpha(b + "2"))
    return x + conv(d, W.wn(b + "3"), W.bias(b + "3"))


def encoder(W, cfg, x):
    """layers.py:133-156: x [B][N][1] -> [B][T][latent]."""
    e = "encoder.block.layers."
    y = conv(x, W.wn(e + "0"), W.bias(e + "0"), pad=3)
    for l, s in enumerate(cfg.encoder_rates):
        p = f"{e}{l + 1}.block.layers."
        for i, dil in enumerate((1, 3, 9)):
            y = residual_unit(W, p + str(i), y, dil)
        y = conv(snake(y, W.alpha(p + "3")), W.wn(p + "4"), W.bias(p + "4"), stride=s, pad=math.ceil(s / 2))
    last = f"{e}{len(cfg.encoder_rates) + 1}"
    return dw_conv(y, W.wn(last), W.bias(last))


def normalize(x, eps=1e-12):
    """vq.py:132-135."""
    return x / np.maximum(np.sqrt((x**2).sum(-1, keepdims=True)), eps)


def vq_search(ze, cb):
    """vq.py:62-77 on rows ze [..., cd]: (indices, distances [..., bins]); argmax(-dist) takes the first index on ties."""
    e, c = normalize(np.asarray(ze, F64)), normalize(np.asarray(cb, F64))
    dist = (e**2).sum(-1, keepdims=True) - 2 * e @ c.T + (c**2).sum(-1)
    return np.argmax(-dist, axis=-1), dist


def quantizer(W, cfg, z):
    """ResidualVectorQuantize.__call__ (vq.py:97-107) on z [B][T][D]: (z_q, codes, per-quantiser trace (distances, residual after))."""
    zq_sum, residual, codes, trace = 0.0, np.asarray(z, F64), [], []
    B, T, D = residual.shape
    for i, s in enumerate(cfg.vq_strides):
        p = f"quantizer.quantizers.{i}"
        pooled = residual.reshape(B, T // s, s, D).sum(2) * (1.0 / s) if s > 1 else residual  # vq.py:26-30
        ze = conv(pooled, W.wn(p + ".in_proj"), W.bias(p + ".in_proj"))
        idx, dist = vq_search(ze, W.w[p + ".codebook.weight"])
        zq = np.asarray(W.w[p + ".codebook.weight"], F64)[idx]
        zq = ze + (zq - ze)  # vq.py:37, as written
        zo = np.repeat(conv(zq, W.wn(p + ".out_proj"), W.bias(p + ".out_proj")), s, axis=1)
        zq_sum = zq_sum + zo
        residual = residual - zo
        codes.append(idx)
        trace.append((dist, residual))
    return zq_sum, codes, trace


def from_codes(W, cfg, codes):
    """vq.py:109-129: [B][T][D]."""
    z = 0.0
    for i, s in enumerate(cfg.vq_strides):
        p = f"quantizer.quantizers.{i}"
        zp = np.asarray(W.w[p + ".codebook.weight"], F64)[np.asarray(codes[i])]
        z = z + np.repeat(conv(zp, W.wn(p + ".out_proj"), W.bias(p + ".out_proj")), s, axis=1)
    return z


def decoder(W, cfg, z, noise):
    """layers.py:159-205 on z [B][T][D]; noise: one [B][1][C] array per block (ignored without NoiseBlocks).  Returns (audio [B][N][1],
    {"block0": ...})."""
    m = "decoder.model.layers."
    y = dw_conv(z, W.wn(m + "0"), W.bias(m + "0"))
    y = conv(y, W.wn(m + "1"), W.bias(m + "1"))
    stages = {}
    for l, s in enumerate(cfg.decoder_rates):
        p = f"{m}{l + 2}.block.layers."
        y = conv_transposed(snake(y, W.alpha(p + "0")), W.wn(p + "1"), W.bias(p + "1"), stride=s, pad=math.ceil(s / 2))
        at = 2
        if cfg.noise:
            y = y + np.asarray(noise[l], F64) * conv(y, W.wn(f"{p}{at}.linear"))  # layers.py:261-267: noise [B][1][C]
            at += 1
        for i, dil in enumerate((1, 3, 9)):
            y = residual_unit(W, p + str(at + i), y, dil)
        stages[f"block{l}"] = y
    n = len(cfg.decoder_rates)
    pcm = conv_cout1(y, W.wn(f"{m}{n + 3}"), W.bias(f"{m}{n + 3}"), pad=3, alpha=W.alpha(f"{m}{n + 2}"), tanh=True)
    return pcm[..., None], stages


def preprocess_length(cfg, n):
    """snac.py:67-85 (attn_window_size None): the padded length."""
    lcm = 1
    for s in cfg.vq_strides:
        lcm = lcm * s // math.gcd(lcm, s)
    unit = int(np.prod(cfg.encoder_rates)) * lcm
    return math.ceil(n / unit) * unit


def encode(W, cfg, audio):
    """SNAC.encode (snac.py:95-99) on audio [B][1][N]: (codes, trace, encoder output)."""
    a = np.asarray(audio, F64)
    n = preprocess_length(cfg, a.shape[-1])
    a = np.pad(a, [(0, 0), (0, 0), (0, n - a.shape[-1])])
    z = encoder(W, cfg, np.moveaxis(a, 1, 2))
    _, codes, trace = quantizer(W, cfg, z)
    return codes, trace, z


def decode(W, cfg, codes, noise):
    """SNAC.decode (snac.py:101-104): (audio [B][N][1], stages with "z_q")."""
    z = from_codes(W, cfg, codes)
    pcm, stages = decoder(W, cfg, z, noise)
    stages["z_q"] = z
    return pcm, stages


def decode_length(cfg, T):
    for s in cfg.decoder_rates:
        T = (T - 1) * s - 2 * math.ceil(s / 2) + 2 * s
    return T


# ------------------------------------------------------------------------------------------------ synthetic checkpoints
def synth_weights(shapes, seed):
    """Random parameters for a name -> shape table (mlx_audio_amd.snac.param_shapes): weight_v ~ N(0, 1 / fan_in), weight_g = |v| times
    U[0.8, 1.2], small biases, Snake alphas in [0.5, 2], N(0, 1) code books; float32."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in shapes.items():
        if name.endswith(".weight_g"):
            continue  # (after every weight_v exists)
        if name.endswith(".alpha"):
            a = rng.uniform(0.5, 2.0, shape)
        elif name.endswith(".weight_v"):
            a = rng.standard_normal(shape) / math.sqrt(shape[1] * shape[2])
        elif name.endswith(".bias"):
            a = 0.05 * rng.standard_normal(shape)
        else:  # codebook.weight
            a = rng.standard_normal(shape)
        w[name] = np.ascontiguousarray(a, dtype=np.float32)
    for name in shapes:
        if name.endswith(".weight_g"):
            v = w[name[: -len("weight_g")] + "weight_v"].astype(F64)
            g = np.sqrt((v**2).sum(axis=(1, 2), keepdims=True))
            # the 1x1 of a ResidualUnit and the last conv (one output channel) are damped: twelve units in a row would otherwise grow the
            # signal by 2^6 and the tanh would see nothing but saturation
            gain = 0.3 if name.endswith(".block.layers.3.weight_g") else (0.25 if v.shape[0] == 1 else 1.0)
            w[name] = np.ascontiguousarray(gain * g * rng.uniform(0.8, 1.2, g.shape), dtype=np.float32)
    return {name: w[name] for name in shapes}


# ------------------------------------------------------------------------------------------------ float32 torch restatement of encode
def encode_torch(w, cfg, audio, dtype):
    """SNAC.encode with torch.nn.functional in `dtype` (torch.float32: what a single-precision implementation computes; the argmax can
    flip against float64 where two code-book rows are a near-tie).  Returns the code arrays."""
    import torch
    import torch.nn.functional as TF

    t = lambda a: torch.tensor(np.asarray(a, F64)).to(dtype)

    def wn(p):  # [O][K][I] -> torch [O][I][K]
        v, g = t(w[p + ".weight_v"]), t(w[p + ".weight_g"])
        return (g * v / torch.sqrt((v**2).sum(dim=(1, 2), keepdim=True))).permute(0, 2, 1).contiguous()

    def sn(x, p):  # x [B][C][L]
        a = t(w[p + ".alpha"]).reshape(1, -1, 1)
        return x + (1.0 / (a + 1e-9)) * torch.sin(a * x) ** 2

    def unit(x, p, dil):
        b = p + ".block.layers."
        C = x.shape[1]
        d = TF.conv1d(sn(x, b + "0"), wn(b + "1"), t(w[b + "1.bias"]), padding=3 * dil, dilation=dil, groups=C)
        return x + TF.conv1d(sn(d, b + "2"), wn(b + "3"), t(w[b + "3.bias"]))

    a = np.asarray(audio, F64)
    n = preprocess_length(cfg, a.shape[-1])
    x = t(np.pad(a, [(0, 0), (0, 0), (0, n - a.shape[-1])]))
    e = "encoder.block.layers."
    y = TF.conv1d(x, wn(e + "0"), t(w[e + "0.bias"]), padding=3)
    for l, s in enumerate(cfg.encoder_rates):
        p = f"{e}{l + 1}.block.layers."
        for i, dil in enumerate((1, 3, 9)):
            y = unit(y, p + str(i), dil)
        y = TF.conv1d(sn(y, p + "3"), wn(p + "4"), t(w[p + "4.bias"]), stride=s, padding=math.ceil(s / 2))
    last = f"{e}{len(cfg.encoder_rates) + 1}"
    z = TF.conv1d(y, wn(last), t(w[last + ".bias"]), padding=3, groups=y.shape[1])
    residual, codes = z, []
    for i, s in enumerate(cfg.vq_strides):
        p = f"quantizer.quantizers.{i}"
        pooled = TF.avg_pool1d(residual, s) if s > 1 else residual
        ze = TF.conv1d(pooled, wn(p + ".in_proj"), t(w[p + ".in_proj.bias"]))  # [B][cd][Ti]
        cb = t(w[p + ".codebook.weight"])
        en = ze.permute(0, 2, 1)
        en = en / torch.clamp(torch.sqrt((en**2).sum(-1, keepdim=True)), min=1e-12)
        cn = cb / torch.clamp(torch.sqrt((cb**2).sum(-1, keepdim=True)), min=1e-12)
        dist = (en**2).sum(-1, keepdim=True) - 2 * en @ cn.T + (cn**2).sum(-1)
        idx = torch.argmax(-dist, dim=-1)
        zq = cb[idx].permute(0, 2, 1)
        zq = ze + (zq - ze)
        zo = TF.conv1d(zq, wn(p + ".out_proj"), t(w[p + ".out_proj.bias"])).repeat_interleave(s, dim=2)
        residual = residual - zo
        codes.append(idx.numpy())
    return codes


def excused_frames(got, ref, trace, strides):
    """The encode criterion: per coarse frame (lcm of the strides latent frames) and item, walk the quantisers in order; at the FIRST one
    whose codes differ inside the frame every differing code must be a near-tie by the reference's own distances (gap < 1e-4 of the
    spread), and the later quantisers of that frame are not comparable.  Returns (frames excused, frames in all); raises AssertionError
    on a flip that is no near-tie."""
    lcm = 1
    for s in strides:
        lcm = lcm * s // math.gcd(lcm, s)
    B, T = ref[0].shape[0], ref[0].shape[1] * strides[0]
    excused = 0
    for b in range(B):
        for f in range(T // lcm):
            for i, s in enumerate(strides):
                n = lcm // s
                sl = slice(f * n, (f + 1) * n)
                g, r = np.asarray(got[i])[b, sl], np.asarray(ref[i])[b, sl]
                if np.array_equal(g, r):
                    continue
                for j in np.nonzero(g != r)[0]:
                    dist = trace[i][0][b, f * n + j]
                    gap = abs(float(dist[g[j]]) - float(dist[r[j]]))
                    assert gap < 1e-4 * float(dist.max() - dist.min()), (b, f, i, int(j), gap)
                excused += 1
                break
    return excused, B * (T // lcm)


# ------------------------------------------------------------------------------------------------ the test configurations and inputs
CONFIGS = {
    "even": dict(sampling_rate=24000, encoder_dim=4, encoder_rates=[2, 4], decoder_dim=32, decoder_rates=[4, 2], attn_window_size=None,
                 codebook_size=37, codebook_dim=8, vq_strides=[4, 2, 1], noise=True),
    "odd": dict(sampling_rate=24000, encoder_dim=4, encoder_rates=[3, 2], decoder_dim=32, decoder_rates=[2, 3], attn_window_size=None,
                codebook_size=37, codebook_dim=8, vq_strides=[2, 1], noise=False),
    "wide": dict(sampling_rate=24000, encoder_dim=16, encoder_rates=[2, 2], latent_dim=64, decoder_dim=256, decoder_rates=[2, 2],
                 attn_window_size=None, codebook_size=64, codebook_dim=8, vq_strides=[2, 1], noise=True),
}
WEIGHT_SEED = 7
# encode inputs: (configuration, B, N, seed).  N = 601 is no multiple of the padding unit (32).  The seeds are pinned by
# tests/test_snac_ref_cpu.py: a float32 restatement stays under the 5 % cap of excused coarse frames against float64.
ENCODE_CASES = {"even": ("even", 2, 640, 11), "odd": ("odd", 2, 240, 12), "unpadded": ("even", 2, 601, 13)}
EXCUSED_CAP = 0.05


def audio(B, N, seed):
    return (0.5 * np.random.default_rng(seed).standard_normal((B, 1, N))).astype(np.float32)
