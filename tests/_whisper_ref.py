"""CPU references of the Whisper audio side (mlx-audio_amd/whisper.py, csrc/kk_whisper.hip), written from the semantics of
mlx_audio/stt/models/whisper/audio.py:41-82 and whisper.py:81-199 in this repository's own words.  tests/test_whisper_cpu.py pins them
against an independent implementation (transformers); the GPU tests compare the kernels against them."""
import math

import numpy as np

N_FFT, HOP, N_BINS = 400, 160, 201


def hann_symmetric(dtype=np.float64):
    i = np.arange(N_FFT, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * i / (N_FFT - 1)))).astype(dtype)


def frames(x, padding=0):
    """x (n,) -> (F, 400) frames at hop 160 of [reflect 200 | x | `padding` zeros | reflect 200] with the LAST frame dropped: F = (n + padding) // 160."""
    x = np.concatenate([np.asarray(x), np.zeros(padding, dtype=np.asarray(x).dtype)])
    if x.shape[0] < N_FFT // 2 + 1:
        raise ValueError("too short for the reflect padding")
    y = np.concatenate([x[1 : N_FFT // 2 + 1][::-1], x, x[-(N_FFT // 2 + 1) : -1][::-1]])
    nf = 1 + (y.shape[0] - N_FFT) // HOP
    idx = np.arange(nf - 1)[:, None] * HOP + np.arange(N_FFT)[None, :]
    return y[idx]


def dft_tables(dtype=np.float64):
    """cos / sin [400][201] of 2 pi i k / 400, made in float64 from the reduced index (i k) mod 400"""
    ik = (np.arange(N_FFT)[:, None] * np.arange(N_BINS)[None, :]) % N_FFT
    a = 2.0 * np.pi * ik.astype(np.float64) / N_FFT
    return np.cos(a).astype(dtype), np.sin(a).astype(dtype)


def log_mel(x, n_mels, padding=0, dtype=np.float64, bank=None):
    """(F, n_mels) log-mel of one clip by a DIRECT DFT (a matrix product, no FFT) with every step in `dtype`: float64 is the reference, float32
    the yardstick of what single precision costs."""
    from mlx_audio_amd.whisper import mel_filters

    bank = (mel_filters(n_mels) if bank is None else bank).astype(dtype)
    fr = frames(np.asarray(x, dtype), padding) * hann_symmetric(dtype)[None, :]
    c, s = dft_tables(dtype)
    re, im = fr @ c, fr @ s
    power = re * re + im * im
    mel = power @ bank.T
    lg = np.log10(np.maximum(mel, dtype(1e-10)))
    lg = np.maximum(lg, lg.max() - dtype(8.0))
    out = (lg + dtype(4.0)) / dtype(4.0)
    assert out.dtype == dtype
    return out


def signal(n, seed):
    """Gaussian noise at 0.1 with one stretch scaled by 1e-3, one stretch of exact zeros and a 440 Hz tone over the first quarter (fp32)."""
    g = np.random.default_rng(seed)
    x = 0.1 * g.standard_normal(n)
    x[n // 2 : n // 2 + n // 8] *= 1e-3
    x[3 * n // 4 : 3 * n // 4 + n // 8] = 0.0
    q = n // 4
    x[:q] += 0.5 * np.sin(2.0 * np.pi * 440.0 * np.arange(q) / 16000.0)
    return x.astype(np.float32)


def sinusoids(length, channels, max_timescale=10000.0):
    """whisper.py:81-87 in float32: sin | cos of t * exp(-log(max_timescale) / (channels / 2 - 1) * j).  In torch's float32 arithmetic, step by step
    as the formula reads: at t ~ 1000 the argument's own rounding is ~1e-4, so two float32 evaluations agree to 1e-6 only when they round alike."""
    import torch

    half = channels // 2
    inv = torch.exp(-(math.log(max_timescale) / (half - 1)) * torch.arange(half))
    t = torch.arange(length).view(-1, 1) * inv.view(1, -1)
    return torch.cat([t.sin(), t.cos()], dim=1).numpy().astype(np.float32)


def bf16_round(a):
    """float32 -> nearest-even bf16, returned as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def attention(q, k, v):
    """float64 softmax(q k^T / 8) v for one (item, head): q, k, v (T, 64)"""
    s = q.astype(np.float64) @ k.astype(np.float64).T / 8.0
    s -= s.max(axis=1, keepdims=True)
    p = np.exp(s)
    return (p / p.sum(axis=1, keepdims=True)) @ v.astype(np.float64)


# ---- synthetic encoders -----------------------------------------------------------------------------------------------------------------
def dims(n_mels, ctx, width, heads, layers):
    from mlx_audio_amd.whisper import ModelDimensions

    return ModelDimensions(n_mels, ctx, width, heads, layers, 51866, 448, width, heads, 1)


def encoder_weights(d, seed, torch_conv_layout=False):
    """MLX-named encoder parameters: matrices N(0, 1 / fan_in), LayerNorm gains 1 + 0.2 N, biases 0.1 N, all pre-rounded to bf16; no key bias."""
    g = np.random.default_rng(seed)
    D, M = d.n_audio_state, d.n_mels

    def mat(*shape, fan_in):
        return bf16_round((g.standard_normal(shape) / math.sqrt(fan_in)).astype(np.float32))

    def vec(n, gain=False):
        return bf16_round(((1.0 if gain else 0.0) + (0.2 if gain else 0.1) * g.standard_normal(n)).astype(np.float32))

    w = {"encoder.conv1.weight": mat(D, 3, M, fan_in=3 * M), "encoder.conv1.bias": vec(D),
         "encoder.conv2.weight": mat(D, 3, D, fan_in=3 * D), "encoder.conv2.bias": vec(D)}
    for i in range(d.n_audio_layer):
        p = f"encoder.blocks.{i}."
        for lin in ("query", "key", "value", "out"):
            w[p + f"attn.{lin}.weight"] = mat(D, D, fan_in=D)
            if lin != "key":
                w[p + f"attn.{lin}.bias"] = vec(D)
        w[p + "mlp1.weight"], w[p + "mlp1.bias"] = mat(4 * D, D, fan_in=D), vec(4 * D)
        w[p + "mlp2.weight"], w[p + "mlp2.bias"] = mat(D, 4 * D, fan_in=4 * D), vec(D)
        for ln in ("attn_ln", "mlp_ln"):
            w[p + ln + ".weight"], w[p + ln + ".bias"] = vec(D, gain=True), vec(D)
    w["encoder.ln_post.weight"], w["encoder.ln_post.bias"] = vec(D, gain=True), vec(D)
    if torch_conv_layout:
        for k in ("encoder.conv1.weight", "encoder.conv2.weight"):
            w[k] = np.ascontiguousarray(w[k].transpose(0, 2, 1))
    return w


def hf_encoder(d, w):
    """transformers' WhisperEncoder (fp32, CPU, eval) carrying the MLX-named weights `w` (conv weights [O, K, I])."""
    import torch
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder

    cfg = WhisperConfig(num_mel_bins=d.n_mels, d_model=d.n_audio_state, encoder_layers=d.n_audio_layer, encoder_attention_heads=d.n_audio_head,
                        encoder_ffn_dim=4 * d.n_audio_state, max_source_positions=d.n_audio_ctx, activation_function="gelu", dropout=0.0,
                        attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layers=1, decoder_attention_heads=d.n_audio_head,
                        decoder_ffn_dim=8, attn_implementation="eager")
    enc = WhisperEncoder(cfg).eval()
    t = lambda k: torch.from_numpy(np.ascontiguousarray(w[k]))  # noqa: E731
    sd = {"conv1.weight": t("encoder.conv1.weight").permute(0, 2, 1).contiguous(), "conv1.bias": t("encoder.conv1.bias"),
          "conv2.weight": t("encoder.conv2.weight").permute(0, 2, 1).contiguous(), "conv2.bias": t("encoder.conv2.bias"),
          "layer_norm.weight": t("encoder.ln_post.weight"), "layer_norm.bias": t("encoder.ln_post.bias"),
          "embed_positions.weight": enc.embed_positions.weight.detach().clone()}
    names = {"attn.query": "self_attn.q_proj", "attn.key": "self_attn.k_proj", "attn.value": "self_attn.v_proj", "attn.out": "self_attn.out_proj",
             "mlp1": "fc1", "mlp2": "fc2", "attn_ln": "self_attn_layer_norm", "mlp_ln": "final_layer_norm"}
    for i in range(d.n_audio_layer):
        for ours, theirs in names.items():
            for part in ("weight", "bias"):
                k = f"encoder.blocks.{i}.{ours}.{part}"
                if k in w:
                    sd[f"layers.{i}.{theirs}.{part}"] = t(k)
    missing, unexpected = enc.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.endswith("k_proj.bias") for m in missing), (missing, unexpected)
    return enc


def hf_encode(enc, mel, bf16=False):
    """mel (B, 2 ctx, n_mels) float32 numpy -> (B, ctx, D) float32 numpy; bf16: the module converted with .bfloat16() and run on the CPU"""
    import copy

    import torch

    x = torch.from_numpy(np.ascontiguousarray(mel)).permute(0, 2, 1).contiguous()
    with torch.no_grad():
        if bf16:
            return copy.deepcopy(enc).bfloat16()(x.bfloat16()).last_hidden_state.float().numpy()
        return enc(x).last_hidden_state.numpy()


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).mean()) / np.sqrt((ref**2).mean()))
