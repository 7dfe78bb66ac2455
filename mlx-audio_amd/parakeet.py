"""Parakeet (FastConformer) on the device, audio side: the encoder's hot blocks that no other kernel of the library serves
(mlx_audio/stt/models/parakeet/attention.py, conformer.py).  The arithmetic runs in libkokoro_hip.so (csrc/kk_parakeet.hip); there is
no PyTorch fallback.  Tensors are torch tensors on the device; work is enqueued on torch's current stream.

    rel_pos_attention(qkv, pos, pos_bias_u, pos_bias_v, heads)   RelPositionMultiHeadAttention after its Linears, rel_shift included
    conformer_dwconv(x, w, bias)                                 silu(bn(depthwise_conv(glu(x)))) of the Convolution module
    conv2d_s2(x, w, bias, stem)                                  a 3 x 3 stride-2 Conv2d of DwStridingSubsampling, channels-last
    fold_batch_norm(...)                                         depth-wise taps and bias with the inference-form BatchNorm folded in (float64)
    rel_positions(T, d_model)                                    RelPositionalEncoding's table for positions T - 1 .. -(T - 1) (float64)
    subsampled_lengths(lengths, factor)                          DwStridingSubsampling's length formula

    Model(config).load_weights(w) / Model.from_pretrained(dir)   the FastConformer encoder behind one handle: encode(mel) -> (features, lengths)

    PreprocessArgs, log_mel_spectrogram(audio, args)             parakeet/audio.py's features on the device; Model.encode_audio(audio) chains the two

What is NOT built: the whole text side (TDT / RNNT / CTC decoding, alignment, chunked generate, streaming caches); ragged masking and sub-samplings
other than dw_striding."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, fields

import numpy as np

from . import _lib

BN_EPS = 1e-5  # mlx.nn.BatchNorm's default, which conformer.py:68 takes


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _want(t, name, dtype, ndim):
    if not (t.is_cuda and t.dtype == dtype and t.dim() == ndim and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous {ndim}-d {dtype} tensor on the device")


def rel_positions(T: int, d_model: int) -> np.ndarray:
    """attention.py:155-185: float64 [2 T - 1][d_model], row r is position T - 1 - r, sin in the even and cos in the odd channels.  The slice the
    reference takes from its max_len table depends on T alone, so the table is made for T."""
    pos = np.arange(T - 1, -T, -1, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, d_model, 2, dtype=np.float64) * -(math.log(10000.0) / d_model))
    pe = np.zeros((2 * T - 1, d_model))
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)
    return pe


def subsampled_lengths(lengths, factor: int):
    """conformer.py:241-248: log2(factor) times floor((n + 2 - 3) / 2) + 1"""
    n = np.asarray(lengths, dtype=np.int64)
    for _ in range(int(math.log(factor, 2))):
        n = (n - 1) // 2 + 1
    return n


def fold_batch_norm(dw_weight, dw_bias, bn_weight, bn_bias, running_mean, running_var, eps: float = BN_EPS):
    """Depth-wise Conv1d weight [D][k] (or MLX's [D][k][1]) and bias [D] or None, with y = (conv - mean) / sqrt(var + eps) * weight + bias folded in,
    in float64.  Returns (w fp32 [k][D], bias fp32 [D]) as kk_op_conformer_dwconv takes them."""
    w = np.asarray(dw_weight, dtype=np.float64)
    w = w.reshape(w.shape[0], -1)
    g = np.asarray(bn_weight, np.float64) / np.sqrt(np.asarray(running_var, np.float64) + eps)
    b0 = np.zeros(w.shape[0]) if dw_bias is None else np.asarray(dw_bias, np.float64)
    b = (b0 - np.asarray(running_mean, np.float64)) * g + np.asarray(bn_bias, np.float64)
    return np.ascontiguousarray((w * g[:, None]).T).astype(np.float32), b.astype(np.float32)


def rel_pos_attention(qkv, pos, pos_bias_u, pos_bias_v, heads: int, T: int | None = None, out=None):
    """qkv bf16 [B][T_rows][3 * heads * hd] (q | k | v), pos bf16 [2 T - 1][heads * hd] = linear_pos(rel_positions), pos_bias_u / _v fp32 [heads][hd],
    hd 64 or 128.  Returns bf16 [B][T_rows][heads * hd]; only the first T rows (default: all) are read and written."""
    import torch

    _want(qkv, "qkv", torch.bfloat16, 3)
    _want(pos, "pos", torch.bfloat16, 2)
    _want(pos_bias_u, "pos_bias_u", torch.float32, 2)
    _want(pos_bias_v, "pos_bias_v", torch.float32, 2)
    B, T_rows, ld = qkv.shape
    T = T_rows if T is None else T
    hs = ld // 3
    if ld != 3 * hs or hs % heads != 0:
        raise ValueError("qkv: the last axis must hold q | k | v of `heads` heads")
    hd = hs // heads
    if tuple(pos.shape) != (2 * T - 1, hs):
        raise ValueError(f"pos: need [2 T - 1 = {2 * T - 1}][{hs}], got {tuple(pos.shape)}")
    if tuple(pos_bias_u.shape) != (heads, hd) or tuple(pos_bias_v.shape) != (heads, hd):
        raise ValueError(f"pos_bias_u / pos_bias_v: need [{heads}][{hd}]")
    if out is None:
        out = torch.zeros((B, T_rows, hs), dtype=torch.bfloat16, device=qkv.device)
    else:
        _want(out, "out", torch.bfloat16, 3)
        if tuple(out.shape) != (B, T_rows, hs):
            raise ValueError(f"out: need {(B, T_rows, hs)}")
    lib = _lib.load()
    _lib.check(lib.kk_op_rel_pos_attention(_stream(), B, _p(qkv), ld, T_rows, T, heads, hd, _p(pos), hs, _p(pos_bias_u), _p(pos_bias_v), _p(out), hs),
               "kk_op_rel_pos_attention")
    return out


def conformer_dwconv(x, w, bias):
    """x bf16 [B][T][2 D] (pointwise_conv1's output), w fp32 [k][D] and bias fp32 [D] from fold_batch_norm -> bf16 [B][T][D]"""
    import torch

    _want(x, "x", torch.bfloat16, 3)
    _want(w, "w", torch.float32, 2)
    _want(bias, "bias", torch.float32, 1)
    B, T, D2 = x.shape
    k, D = w.shape
    if D2 != 2 * D or bias.shape[0] != D:
        raise ValueError(f"x has {D2} channels, w and bias are for D = {D}: need 2 D")
    out = torch.empty((B, T, D), dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    _lib.check(lib.kk_op_conformer_dwconv(_stream(), B, _p(x), D2, T, D, k, _p(w), _p(bias), _p(out), D), "kk_op_conformer_dwconv")
    return out


def conv2d_s2(x, w, bias, stem: bool):
    """stem: x fp32 [B][T][F] -> relu(conv) bf16 [B][T'][F'][C].  Otherwise x bf16 [B][T][F][C], depth-wise -> bf16 [B][T'][F'][C].  w fp32 [9][C]
    (tap ky * 3 + kx: a Conv2d weight [C][1][3][3] is w.reshape(C, 9).T), bias fp32 [C].  T' = (T - 1) // 2 + 1, F' likewise."""
    import torch

    _want(x, "x", torch.float32 if stem else torch.bfloat16, 3 if stem else 4)
    _want(w, "w", torch.float32, 2)
    _want(bias, "bias", torch.float32, 1)
    B, T, F = x.shape[:3]
    Cn = w.shape[1]
    if w.shape[0] != 9 or bias.shape[0] != Cn or (not stem and x.shape[3] != Cn):
        raise ValueError("w must be [9][C], bias [C] and a depth-wise input [B][T][F][C]")
    out = torch.empty((B, (T - 1) // 2 + 1, (F - 1) // 2 + 1, Cn), dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    _lib.check(lib.kk_op_conv2d_s2(_stream(), B, _p(x), 1 if stem else 0, T, F, Cn, _p(w), _p(bias), _p(out)), "kk_op_conv2d_s2")
    return out


# --------------------------------------------------------------------------------------------------------------------------------- features
@dataclass
class PreprocessArgs:
    """parakeet/audio.py:16-35"""
    sample_rate: int
    normalize: str
    window_size: float
    window_stride: float
    window: str
    features: int
    n_fft: int
    dither: float = 0.0  # unused by the reference's log_mel_spectrogram, and here
    pad_to: int = 0
    pad_value: float = 0

    @property
    def win_length(self) -> int:
        return int(self.window_size * self.sample_rate)

    @property
    def hop_length(self) -> int:
        return int(self.window_stride * self.sample_rate)

    @classmethod
    def from_dict(cls, d: dict):
        return cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})


def window_table(name: str, size: int) -> np.ndarray:
    """mlx_audio/utils.py:10-47 in float64; an unknown name is the Hann window, as audio.py:46-47 has it"""
    n = np.arange(size, dtype=np.float64)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(2 * math.pi * n / (size - 1))
    if name == "blackman":
        return 0.42 - 0.5 * np.cos(2 * math.pi * n / (size - 1)) + 0.08 * np.cos(4 * math.pi * n / (size - 1))
    if name == "bartlett":
        return 1 - 2 * np.abs(n - (size - 1) / 2) / (size - 1)
    return 0.5 * (1 - np.cos(2 * math.pi * n / (size - 1)))


def mel_filter_bank(sample_rate: int, n_fft: int, n_mels: int) -> np.ndarray:
    """The float64 (n_mels, n_fft / 2 + 1) bank that mel_filters(sample_rate, n_fft, n_mels, norm=args.normalize, mel_scale=None) produces
    (mlx_audio/utils.py:165-237): a mel_scale other than "htk" takes the Slaney branch, and a norm other than "slaney" -- "per_feature", say -- leaves
    the triangles un-normalised, with peaks of 1."""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    to_mel = lambda f: min_log_hz / f_sp + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp  # noqa: E731
    freqs = np.linspace(0.0, sample_rate // 2, n_fft // 2 + 1)
    mels = np.linspace(to_mel(0.0), to_mel(sample_rate / 2), n_mels + 2)
    pts = np.where(mels >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (mels - min_log_hz / f_sp)), f_sp * mels)
    diff, slopes = pts[1:] - pts[:-1], pts[None, :] - freqs[:, None]
    return np.maximum(0.0, np.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:])).T


_front_tables = {}


def log_mel_spectrogram(audio, args: PreprocessArgs):
    """audio.py:38-70 on the device (kk_op_parakeet_log_mel): audio [n] or [B][n] samples (numpy or torch, host or device) -> fp32 device
    [1 or B][1 + max(n, pad_to) // hop][features], every row normalised on its own."""
    import torch

    x = torch.as_tensor(audio, dtype=torch.float32).cuda()
    x = (x[None] if x.dim() == 1 else x).contiguous()
    B, n = x.shape
    key = (args.sample_rate, args.n_fft, args.features, args.window, args.win_length)
    if key not in _front_tables:
        j = 2 * math.pi * np.arange(args.n_fft, dtype=np.float64) / args.n_fft
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
        _front_tables[key] = (dev(window_table(args.window, args.win_length)), dev(np.stack([np.cos(j), np.sin(j)])),
                              dev(mel_filter_bank(args.sample_rate, args.n_fft, args.features).T))
    win, cs, fbT = _front_tables[key]
    F = 1 + max(n, args.pad_to) // args.hop_length
    out = torch.empty((B, F, args.features), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().kk_op_parakeet_log_mel(_stream(), B, _p(x), n, n, int(args.pad_to), float(args.pad_value), args.n_fft, args.hop_length,
                                                  args.win_length, args.features, 1 if args.normalize == "per_feature" else 0, _p(win), _p(cs), _p(fbT),
                                                  _p(out)), "kk_op_parakeet_log_mel")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- encoder
CONFORMER_KEYS = ("feat_in", "n_layers", "d_model", "n_heads", "ff_expansion_factor", "subsampling_factor", "conv_kernel_size", "subsampling_conv_channels")
TEXT_SIDE = "the text side (prediction network, joint, TDT / RNNT / CTC decoding, alignment, chunked generate) is not built: Model.encode gives the encoder states"


def is_parakeet_config(config: dict) -> bool:
    enc = config.get("encoder")
    return isinstance(enc, dict) and "preprocessor" in config and "subsampling" in enc and "self_attention_model" in enc


def check_conformer_args(enc: dict):
    """The Conformer variants that are served; anything else is refused by the name of its field."""
    if enc.get("subsampling", "dw_striding") != "dw_striding":
        raise NotImplementedError(f"subsampling = {enc['subsampling']!r}: only 'dw_striding' is built")
    if enc.get("causal_downsampling", False):
        raise NotImplementedError("causal_downsampling = True is not built")
    if enc.get("self_attention_model", "rel_pos") != "rel_pos":
        raise NotImplementedError(f"self_attention_model = {enc['self_attention_model']!r}: only 'rel_pos' is built")
    missing = [k for k in CONFORMER_KEYS if k not in enc]
    if missing:
        raise ValueError(f"encoder config lacks {missing}")


def canonical_tensors(enc: dict, w: dict) -> dict:
    """The reference's encoder parameters (names of conformer.py under `encoder.`, MLX or PyTorch conv layouts: every conv here has one input channel per
    group or a 1-wide kernel, so both flatten alike) -> the float32 tensors kk_parakeet_load_tensor takes, folded in float64:
    BatchNorm into the depth-wise taps, the 1/2 of `x += 0.5 ff(x)` into linear2, sqrt(d_model) of xscaling into pre_encode.out, the columns of
    pre_encode.out from (c, f) to (f, c), q | k | v stacked, absent biases as zeros."""
    D, Cc, n_sub = enc["d_model"], enc["subsampling_conv_channels"], int(math.log2(enc["subsampling_factor"]))
    f64 = lambda name: np.asarray(w[name], dtype=np.float64)  # noqa: E731
    bias = lambda name, n: f64(name) if name in w else np.zeros(n)  # noqa: E731
    out = {}

    def lin(dst, src, n, scale=1.0):
        m = f64(src + ".weight")
        out[dst + ".w"], out[dst + ".b"] = m.reshape(m.shape[0], -1) * scale, bias(src + ".bias", n) * scale

    pre = "encoder.pre_encode."
    out["pre.stem.w"], out["pre.stem.b"] = f64(pre + "conv.0.weight").reshape(Cc, 9).T, bias(pre + "conv.0.bias", Cc)
    for i in range(1, n_sub):
        out[f"pre.{i}.dw.w"], out[f"pre.{i}.dw.b"] = f64(pre + f"conv.{3 * i - 1}.weight").reshape(Cc, 9).T, bias(pre + f"conv.{3 * i - 1}.bias", Cc)
        lin(f"pre.{i}.pw", pre + f"conv.{3 * i}", Cc)
    xs = math.sqrt(D) if enc.get("xscaling", False) else 1.0
    wo = f64(pre + "out.weight")
    f_out = wo.shape[1] // Cc
    out["pre.out.w"], out["pre.out.b"] = wo.reshape(D, Cc, f_out).transpose(0, 2, 1).reshape(D, -1) * xs, bias(pre + "out.bias", D) * xs
    for li in range(enc["n_layers"]):
        s, d = f"encoder.layers.{li}.", f"L{li}."
        for dst, src in (("ff1.ln", "norm_feed_forward1"), ("att.ln", "norm_self_att"), ("conv.ln", "norm_conv"), ("ff2.ln", "norm_feed_forward2"),
                         ("out.ln", "norm_out")):
            out[d + dst + ".w"], out[d + dst + ".b"] = f64(s + src + ".weight"), f64(s + src + ".bias")
        for ff in ("1", "2"):
            lin(d + f"ff{ff}.a", s + f"feed_forward{ff}.linear1", D * enc["ff_expansion_factor"])
            lin(d + f"ff{ff}.b", s + f"feed_forward{ff}.linear2", D, 0.5)
        a = s + "self_attn."
        out[d + "qkv.w"] = np.concatenate([f64(a + f"linear_{n}.weight") for n in "qkv"])
        out[d + "qkv.b"] = np.concatenate([bias(a + f"linear_{n}.bias", D) for n in "qkv"])
        out[d + "pos.w"], out[d + "pos.b"] = f64(a + "linear_pos.weight"), np.zeros(D)
        lin(d + "o", a + "linear_out", D)
        out[d + "u"], out[d + "v"] = f64(a + "pos_bias_u").reshape(-1), f64(a + "pos_bias_v").reshape(-1)
        lin(d + "pw1", s + "conv.pointwise_conv1", 2 * D)
        lin(d + "pw2", s + "conv.pointwise_conv2", D)
        bn = s + "conv.batch_norm."
        out[d + "dw.w"], out[d + "dw.b"] = fold_batch_norm(f64(s + "conv.depthwise_conv.weight"), w.get(s + "conv.depthwise_conv.bias"), f64(bn + "weight"),
                                                           f64(bn + "bias"), f64(bn + "running_mean"), f64(bn + "running_var"))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


class Model:
    """parakeet.py's model, audio side: `encode(mel) -> (features, lengths)` on the device (kk_parakeet_*).  config: the checkpoint's config.json as a dict
    (its `encoder` block is ConformerArgs)."""

    def __init__(self, config: dict):
        self.config = config
        self.enc = dict(config["encoder"])
        check_conformer_args(self.enc)
        self.preprocessor = PreprocessArgs.from_dict(config["preprocessor"]) if config.get("preprocessor") else None
        self._h, self._pos, self._ws, self.text_side_weights = None, {}, {}, {}

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().kk_parakeet_destroy(self._h)

    def load_weights(self, weights: dict):
        """weights: name -> array (numpy, or anything np.asarray takes).  `decoder.*`, `joint.*` and `ctc.*` are kept aside for the text side."""
        import torch

        lib = _lib.load()
        w = {k: (v.float().cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in weights.items()}
        self.text_side_weights = {k: v for k, v in w.items() if k.split(".")[0] in ("decoder", "joint", "ctc")}
        h = C.c_void_p()
        _lib.check(lib.kk_parakeet_create(C.byref(_lib.KKParakeetConfig(*[int(self.enc[k]) for k in CONFORMER_KEYS])), C.byref(h)), "kk_parakeet_create")
        self._h = h
        for name, a in canonical_tensors(self.enc, w).items():
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _lib.check(lib.kk_parakeet_load_tensor(h, name.encode(), shape, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_parakeet_load_tensor")
        torch.cuda.init()
        _lib.check(lib.kk_parakeet_finalize(h, _stream()), "kk_parakeet_finalize")
        return self

    @classmethod
    def from_pretrained(cls, local_dir):
        """A local directory with config.json and *.safetensors"""
        import glob
        import json
        import os

        from safetensors import safe_open

        with open(os.path.join(local_dir, "config.json")) as f:
            model = cls(json.load(f))
        weights = {}
        for path in sorted(glob.glob(os.path.join(local_dir, "*.safetensors"))):
            with safe_open(path, framework="np") as f:
                weights.update({k: f.get_tensor(k) for k in f.keys()})
        if not weights:
            raise FileNotFoundError(f"No safetensors found in {local_dir}")
        return model.load_weights(weights)

    def encode(self, mel, cache=None):
        """mel [B][T_mel][feat_in] or [T_mel][feat_in] (torch or numpy; every item has T_mel frames, no mask is applied, as in the reference) ->
        (features fp32 device [B][T'][d_model], lengths int64 numpy [B])"""
        import torch

        if cache is not None:
            raise NotImplementedError("cache: streaming caches are not built")
        if self._h is None:
            raise RuntimeError("load_weights first")
        mel = torch.as_tensor(mel, dtype=torch.float32).cuda()
        mel = (mel[None] if mel.dim() == 2 else mel).contiguous()
        B, T_mel, F = mel.shape
        if F != self.enc["feat_in"]:
            raise ValueError(f"mel has {F} features, feat_in = {self.enc['feat_in']}")
        lib = _lib.load()
        T, D = lib.kk_parakeet_encode_frames(self._h, T_mel), self.enc["d_model"]
        if T not in self._pos:
            self._pos[T] = torch.from_numpy(rel_positions(T, D)).to(torch.float32).cuda().to(torch.bfloat16).contiguous()
        if (B, T_mel) not in self._ws:  # the workspace of the last shape is kept across calls
            self._ws = {(B, T_mel): torch.empty(lib.kk_parakeet_encode_workspace_bytes(self._h, B, T_mel), dtype=torch.uint8, device="cuda")}
        ws = self._ws[(B, T_mel)]
        nbytes = ws.numel()
        out = torch.empty((B, T, D), dtype=torch.float32, device="cuda")
        _lib.check(lib.kk_parakeet_encode(self._h, _stream(), B, T_mel, _p(mel), _p(self._pos[T]), _p(ws), nbytes, _p(out)), "kk_parakeet_encode")
        return out, subsampled_lengths([T_mel] * B, self.enc["subsampling_factor"])

    def encode_audio(self, audio):
        """samples [n] or [B][n] at preprocessor.sample_rate -> encode(log_mel_spectrogram(audio, preprocessor))"""
        if self.preprocessor is None:
            raise ValueError("the config has no preprocessor block")
        return self.encode(log_mel_spectrogram(audio, self.preprocessor))

    def decode(self, *a, **k):
        raise NotImplementedError(TEXT_SIDE)

    decode_chunk = generate = decode
