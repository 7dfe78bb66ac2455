"""Host mirror of the reference's Vocos vocoder (mlx_audio/codec/models/vocos/vocos.py): `Vocos(cfg, weights)`, `decode(features, bandwidth_id)`,
`from_pretrained` (a LOCAL directory only), and the two kernels on their own: `dwconv_layernorm` (ConvNeXtBlock's depth-wise conv -> LayerNorm /
AdaLayerNorm in one launch) and `istft_head` (ISTFTHead after its Linear, on an FFT).  The arithmetic runs in libkokoro_hip.so (kk_vocos_*,
kk_op_vocos_dwconv_ln, kk_op_vocos_istft; csrc/kk_vocos.hip); PyTorch allocates device memory, provides the stream and applies AdaLayerNorm's two
small Linears to the condition.

Not built (each refusal names what it is): `MelSpectrogramFeatures` and `Vocos.__call__(audio)` (a forward 1024-point transform); `EncodecFeatures`,
`get_encodec_codes` and `decode_from_codes` (EnCodec); the backbone inside Spark's codec; ragged batches; streaming; `padding="same"`."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import KokoroHipError, check

MAX_DIM = 1024  # the fused dwconv -> LayerNorm kernel's channel range is 1 .. 1024


@dataclass
class VocosConfig:
    """`init_args` of VocosBackbone and ISTFTHead in a Vocos config.yaml (vocos.py:120,211-220), with their defaults."""
    input_channels: int
    dim: int
    intermediate_dim: int
    num_layers: int
    n_fft: int
    hop_length: int
    adanorm_num_embeddings: Optional[int] = None
    bias: bool = True
    padding: str = "center"
    layer_scale_init_value: Optional[float] = None

    @classmethod
    def from_dict(cls, d: dict) -> "VocosConfig":
        """The hparams of a config.yaml ({"backbone": {"init_args": ...}, "head": {"init_args": ...}}), or the flat field names."""
        if "backbone" in d:
            flat = dict(d["backbone"]["init_args"])
            flat.update({k: v for k, v in d["head"]["init_args"].items() if k != "dim"})
            d = flat
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__})

    @classmethod
    def from_yaml(cls, path) -> "VocosConfig":
        import yaml

        with open(path, "r") as f:
            return cls.from_dict(yaml.safe_load(f))

    def to_dict(self) -> dict:
        """The backbone / head part of a config.yaml that `from_dict` reads back."""
        b = dict(input_channels=self.input_channels, dim=self.dim, intermediate_dim=self.intermediate_dim, num_layers=self.num_layers,
                 layer_scale_init_value=self.layer_scale_init_value, adanorm_num_embeddings=self.adanorm_num_embeddings, bias=self.bias)
        return {"backbone": {"class_path": "vocos.models.VocosBackbone", "init_args": b},
                "head": {"class_path": "vocos.heads.ISTFTHead", "init_args": dict(dim=self.dim, n_fft=self.n_fft, hop_length=self.hop_length, padding=self.padding)}}


def vocos_mel_24khz() -> VocosConfig:
    """config.yaml of the public `vocos-mel-24khz` checkpoint."""
    return VocosConfig(input_channels=100, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256)


def vocos_encodec_24khz() -> VocosConfig:
    """config.yaml of the public `vocos-encodec-24khz` checkpoint: AdaLayerNorm on four bandwidth embeddings."""
    return VocosConfig(input_channels=128, dim=384, intermediate_dim=1152, num_layers=8, n_fft=1280, hop_length=320, adanorm_num_embeddings=4)


def _refuse_istft(n_fft: int, hop: int, T: Optional[int] = None) -> None:
    n = int(n_fft)
    while n % 2 == 0 and n > 1:
        n //= 2
    if not 256 <= n_fft <= 2048 or n not in (1, 5):
        raise NotImplementedError(f"n_fft={n_fft} is not built: 2^a or 5 * 2^a with 256 <= n_fft <= 2048 (radix-4 / 2 / 5 passes only)")
    if hop * 4 != n_fft:
        raise NotImplementedError(f"hop_length={hop} is not built: the overlap-add is four-fold, hop_length = n_fft / 4 = {n_fft // 4}")
    if T is not None and T < 2:
        raise ValueError(f"T={T}: the centre cut leaves (T - 1) * hop_length samples, so at least 2 frames are needed")


def _refuse(cfg: VocosConfig) -> None:
    if cfg.padding != "center":
        raise NotImplementedError(f'padding="{cfg.padding}" is not built: the reference\'s ISTFTHead ignores the argument and always cuts the centre')
    _refuse_istft(cfg.n_fft, cfg.hop_length)
    if not 1 <= cfg.dim <= MAX_DIM:
        raise NotImplementedError(f"dim={cfg.dim} is outside the fused dwconv -> LayerNorm kernel's channel range 1 .. {MAX_DIM}")
    if not 1 <= cfg.num_layers <= 16:
        raise ValueError("num_layers must be 1 .. 16")


def param_shapes(cfg: VocosConfig) -> Dict[str, tuple]:
    """Every parameter of the backbone and the head, by name, with its MLX shape: what `load_weights` consumes.  An AdaLayerNorm's `.scale.bias` /
    `.shift.bias` are optional in a checkpoint (zeros when absent)."""
    _refuse(cfg)
    D, I, E, out = cfg.dim, cfg.intermediate_dim, cfg.adanorm_num_embeddings, {}

    def norm(p):
        if E:
            for s in ("scale", "shift"):
                out[f"{p}.{s}.weight"], out[f"{p}.{s}.bias"] = (D, E), (D,)
        else:
            out[p + ".weight"], out[p + ".bias"] = (D,), (D,)

    out["backbone.embed.weight"], out["backbone.embed.bias"] = (D, 7, cfg.input_channels), (D,)
    norm("backbone.norm")
    for i in range(cfg.num_layers):
        p = f"backbone.convnext.{i}"
        out[p + ".dwconv.weight"], out[p + ".dwconv.bias"] = (D, 7, 1), (D,)
        norm(p + ".norm")
        out[p + ".pwconv1.weight"], out[p + ".pwconv1.bias"] = (I, D), (I,)
        out[p + ".pwconv2.weight"], out[p + ".pwconv2.bias"] = (D, I), (D,)
        out[p + ".gamma"] = (D,)
    out["backbone.final_layer_norm.weight"] = (D,)
    if cfg.bias:
        out["backbone.final_layer_norm.bias"] = (D,)
    out["head.out.weight"], out["head.out.bias"] = (cfg.n_fft + 2, D), (cfg.n_fft + 2,)
    return out


def sanitize(cfg: VocosConfig, weights) -> Dict[str, np.ndarray]:
    """Vocos.from_pretrained's rules (vocos.py:316-332) restated for a PyTorch-layout state dict: the two stored windows are dropped,
    `backbone.embed.weight` and every `dwconv` weight get `moveaxis(1, 2)` (where the shape is not the MLX one already), and `feature_extractor.*` is
    dropped (the reference loads non-strictly to skip it).  Beyond the reference: an AdaLayerNorm matrix is accepted in either orientation when
    num_embeddings != dim ([num_embeddings][dim], an nn.Embedding's, is transposed to the Linear's [dim][num_embeddings]), and an absent AdaLayerNorm
    bias becomes zeros."""
    want, out = param_shapes(cfg), {}
    for key, value in weights.items():
        if key.startswith("feature_extractor.") or key == "head.istft.window":
            continue
        value = np.asarray(value)
        shape = want.get(key)
        if shape is not None and value.shape != tuple(shape):
            base, pname = key.rsplit(".", 1)
            if pname == "weight" and ("backbone.embed" in base or "dwconv" in base) and value.ndim == 3:
                value = np.moveaxis(value, 1, 2)
            elif pname == "weight" and base.endswith((".scale", ".shift")) and value.ndim == 2 and value.shape == tuple(shape)[::-1]:
                value = value.T
        out[key] = value
    for key, shape in want.items():
        if key not in out and key.endswith((".scale.bias", ".shift.bias")):
            out[key] = np.zeros(shape, np.float32)
    return out


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dwconv_rows(C_: int) -> int:
    """Time rows per workgroup `dwconv_layernorm` takes for C channels when `rows=0`."""
    return int(_lib.load().kk_op_vocos_dwconv_rows(int(C_)))


def dwconv_layernorm(x, w, b, ln_w, ln_b, eps: float = 1e-6, scale_shift=None, out_dtype=None, out=None, rows: int = 0):
    """ConvNeXtBlock's `dwconv` (k 7, padding 3, groups = C) followed by its LayerNorm, one launch: x [B][T][C] float32 on the device (unit stride
    along C; a view of a wider tensor keeps its pitch), w [C][7][1] / b [C] as a checkpoint holds them, ln_w / ln_b [C] (or None).
    scale_shift [B][2][C]: AdaLayerNorm's per-item pair instead of ln_w / ln_b.  Returns `out` ([B][T][C] float32 or bfloat16; allocated when None).
    rows: time rows per workgroup, 0 = chosen by shape."""
    if not isinstance(x, torch.Tensor) or x.ndim != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("x must be a float32 tensor [B][T][C] with unit stride along C")
    B, T, Cc = x.shape
    if not 1 <= Cc <= MAX_DIM:
        raise NotImplementedError(f"C={Cc} is outside the kernel's channel range 1 .. {MAX_DIM}")
    if not x.is_cuda:
        raise ValueError("x must be on the device")
    dev = x.device
    f32 = lambda t, n: None if t is None else torch.as_tensor(np.asarray(t, np.float32) if not isinstance(t, torch.Tensor) else t).to(dev, torch.float32).reshape(n).contiguous()
    wt, bt = f32(w, (Cc, 7)), f32(b, (Cc,))
    if scale_shift is not None:
        ss = f32(scale_shift, (B, 2, Cc))
        a_p, s_p, stride, keep = C.c_void_p(ss.data_ptr()), C.c_void_p(ss.data_ptr() + 4 * Cc), 2 * Cc, ss
    else:
        at, st = f32(ln_w, (Cc,)), f32(ln_b, (Cc,))
        a_p, s_p, stride, keep = _P(at), _P(st), 0, (at, st)
    if out is None:
        out = torch.empty((B, T, Cc), dtype=out_dtype or torch.float32, device=dev)
    if tuple(out.shape) != (B, T, Cc) or out.dtype not in (torch.float32, torch.bfloat16) or out.device != dev or out.stride(2) != 1:
        raise ValueError(f"out: need {(B, T, Cc)} float32 or bfloat16 on x's device with unit stride along C")
    with torch.cuda.device(dev):
        check(_lib.load().kk_op_vocos_dwconv_ln(_stream(dev), B, _P(x), x.stride(0) if B > 1 else T * x.stride(1), x.stride(1), T, Cc, _P(wt), _P(bt), a_p, s_p, stride,
                                                float(eps), _P(out), out.stride(0) if B > 1 else T * out.stride(1), out.stride(1),
                                                _lib.KK_BF16 if out.dtype == torch.bfloat16 else _lib.KK_F32, int(rows)), "kk_op_vocos_dwconv_ln")
    del keep
    return out


def istft_head(h, n_fft: int, hop: int, group: int = 0, padding: str = "center"):
    """ISTFTHead after its Linear (vocos.py:128-140): h [B][T][>= n_fft + 2] float32 on the device (unit stride along the last axis), log-magnitudes then
    phases of n_fft / 2 + 1 bins -> audio [B][(T - 1) hop] float32.  group: output hops per workgroup, 0 = chosen by shape."""
    if padding != "center":
        raise NotImplementedError(f'padding="{padding}" is not built: the reference\'s ISTFTHead ignores the argument and always cuts the centre')
    if not isinstance(h, torch.Tensor) or h.ndim != 3 or h.dtype != torch.float32 or h.stride(2) != 1 or h.shape[2] < n_fft + 2:
        raise ValueError(f"h must be a float32 tensor [B][T][>= {n_fft + 2}] with unit stride along the last axis")
    B, T, _ = h.shape
    _refuse_istft(n_fft, hop, T)
    if not h.is_cuda:
        raise ValueError("h must be on the device")
    out = torch.empty((B, (T - 1) * hop), dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        check(_lib.load().kk_op_vocos_istft(_stream(h.device), B, T, _P(h), h.stride(0) if B > 1 else T * h.stride(1), h.stride(1), int(n_fft), int(hop), _P(out),
                                            (T - 1) * hop, int(group)), "kk_op_vocos_istft")
    return out


class Vocos:
    def __init__(self, cfg: VocosConfig, weights=None, device: str = "cuda:0", compute_dtype: str = "float32"):
        _refuse(cfg)  # (on the host, before the library is touched)
        if compute_dtype not in ("float32", "bfloat16"):
            raise ValueError("compute_dtype must be float32 or bfloat16")
        self.cfg, self.compute_dtype, self.device = cfg, compute_dtype, torch.device(device)
        self.lib = _lib.load()
        kc = _lib.KKVocosConfig(int(cfg.input_channels), int(cfg.dim), int(cfg.intermediate_dim), int(cfg.num_layers), int(cfg.adanorm_num_embeddings or 0),
                                int(bool(cfg.bias)), int(cfg.n_fft), int(cfg.hop_length), 0, _lib.KK_BF16 if compute_dtype == "bfloat16" else _lib.KK_F32)
        h = C.c_void_p()
        check(self.lib.kk_vocos_create(C.byref(kc), C.byref(h)), "kk_vocos_create")
        self._h, self._final, self._ws, self._last_B, self._ada = h, False, None, 0, None
        if weights is not None:
            self.load_weights(weights)

    def share(self) -> "Vocos":
        """A second Vocos on the SAME kk_vocos (its weights are immutable after finalize; a forward takes a caller-owned workspace): own workspace,
        for another HIP stream / host thread in flight.  Keeps this one alive; only the original destroys the handle."""
        import copy

        other = copy.copy(self)
        other._parent, other._ws = self, None
        return other

    def __del__(self):
        try:
            if getattr(self, "_h", None) and getattr(self, "_parent", None) is None:
                self.lib.kk_vocos_destroy(self._h)
            self._h = None
        except Exception:
            pass

    @classmethod
    def from_pretrained(cls, local_dir, **kw) -> "Vocos":
        """A LOCAL directory with config.yaml + model.safetensors (PyTorch or MLX layout, see `sanitize`).  Nothing is fetched."""
        if not os.path.isdir(str(local_dir)):
            raise FileNotFoundError(f"{local_dir} is not a local directory (Vocos.from_pretrained never goes to the network)")
        cfg_path, st_path = os.path.join(local_dir, "config.yaml"), os.path.join(local_dir, "model.safetensors")
        for p in (cfg_path, st_path):
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        from safetensors.numpy import load_file

        model = cls(VocosConfig.from_yaml(cfg_path), **kw)
        return model.load_weights(sanitize(model.cfg, load_file(st_path)))

    def load_weights(self, weights) -> "Vocos":
        """The reference's parameter names in MLX layout (`param_shapes`).  A missing name or a wrong shape fails with the name; names the module tree
        does not have are ignored."""
        weights = dict(weights.items() if hasattr(weights, "items") else weights)
        want = param_shapes(self.cfg)
        for name, shape in want.items():
            if name not in weights:
                raise ValueError(f"Vocos.load_weights: missing parameter: {name}")
            if tuple(np.shape(weights[name])) != tuple(shape):
                raise ValueError(f"Vocos.load_weights: {name} has shape {tuple(np.shape(weights[name]))}, expected {tuple(shape)}")
        if not torch.cuda.is_available():
            raise KokoroHipError("Vocos needs a GPU: the vocoder has no CPU fallback")
        ada = {}
        for name in want:
            a = np.ascontiguousarray(np.asarray(weights[name], np.float32))
            if ".scale." in name or ".shift." in name:  # AdaLayerNorm's Linears are applied here (`_cond`), not in the library
                ada[name] = a
                continue
            shp = (C.c_int64 * a.ndim)(*a.shape)
            check(self.lib.kk_vocos_load_tensor(self._h, name.encode(), shp, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_vocos_load_tensor")
        if self.cfg.adanorm_num_embeddings:
            norms = ["backbone.norm"] + [f"backbone.convnext.{i}.norm" for i in range(self.cfg.num_layers)]
            # [E][n_norms * 2 * dim] and [n_norms * 2 * dim]: (scale, shift) of every norm side by side
            Wt = np.concatenate([ada[f"{p}.{s}.weight"].T for p in norms for s in ("scale", "shift")], axis=1)
            bt = np.concatenate([ada[f"{p}.{s}.bias"] for p in norms for s in ("scale", "shift")])
            self._ada = (torch.tensor(Wt, device=self.device), torch.tensor(bt, device=self.device))
        with torch.cuda.device(self.device):
            check(self.lib.kk_vocos_finalize(self._h, _stream(self.device)), "kk_vocos_finalize")
        self._final = True
        return self

    def _cond(self, bandwidth_id, B: int) -> torch.Tensor:
        """AdaLayerNorm's `scale(cond)` / `shift(cond)` (vocos.py:203-204) for every norm: [n_norms][B][2][dim].  As the reference does, the Linears
        are applied to whatever float vector [B][num_embeddings] is handed in (its own test passes [[3, 3, 3, 3]]).  The sum runs over the embedding
        axis in a fixed order per element, so an item's pair does not depend on B."""
        E, D, n = self.cfg.adanorm_num_embeddings, self.cfg.dim, self.cfg.num_layers + 1
        c = torch.as_tensor(bandwidth_id).to(self.device, torch.float32)
        if c.ndim == 1:
            c = c[None]
        if c.ndim != 2 or c.shape[1] != E or c.shape[0] not in (1, B):
            raise ValueError(f"bandwidth_id must be a float condition [B, {E}] (or [1, {E}]), got {tuple(c.shape)}")
        Wt, bt = self._ada
        acc = bt[None].expand(c.shape[0], -1).clone()
        for e in range(E):
            acc = acc + c[:, e, None] * Wt[e][None]
        return acc.expand(B, -1).reshape(B, n, 2, D).permute(1, 0, 2, 3).contiguous()

    def __call__(self, audio, **kw):
        raise NotImplementedError("Vocos.__call__(audio) is not built: MelSpectrogramFeatures needs a forward 1024-point transform and EncodecFeatures needs EnCodec; "
                                  "compute the features elsewhere and call decode(features)")

    def get_encodec_codes(self, audio, bandwidth_id):
        raise NotImplementedError("get_encodec_codes is not built: it needs EnCodec")

    def decode_from_codes(self, codes, **kw):
        raise NotImplementedError("decode_from_codes is not built: it needs EnCodec's codebooks")

    def decode(self, features, bandwidth_id=None) -> torch.Tensor:
        """features [B, T, input_channels], or channels-first [B, input_channels, T] (the reference's rule, vocos.py:245: the last axis is not
        input_channels), float -> audio [B, (T - 1) hop_length] float32 on the device.  bandwidth_id: the condition of an AdaLayerNorm model."""
        if bool(self.cfg.adanorm_num_embeddings) and bandwidth_id is None:
            raise ValueError("bandwidth_id is required: the model's norms are AdaLayerNorm (adanorm_num_embeddings is set)")
        if isinstance(features, (list, tuple)):
            if len({tuple(torch.as_tensor(f).shape) for f in features}) > 1:
                raise NotImplementedError("ragged batches are not built; run features of one length together")
            features = torch.stack([torch.as_tensor(f) for f in features])
        x = torch.as_tensor(features)
        if x.ndim != 3:
            raise ValueError(f"features must be [B, T, {self.cfg.input_channels}] or [B, {self.cfg.input_channels}, T], got {tuple(x.shape)}")
        if x.shape[-1] != self.cfg.input_channels:
            x = x.transpose(1, 2)
        if x.shape[-1] != self.cfg.input_channels:
            raise ValueError(f"features must be [B, T, {self.cfg.input_channels}] or [B, {self.cfg.input_channels}, T], got {tuple(torch.as_tensor(features).shape)}")
        B, T, _ = x.shape
        _refuse_istft(self.cfg.n_fft, self.cfg.hop_length, T)
        if not self._final:
            raise KokoroHipError("Vocos: load_weights first")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        cond = self._cond(bandwidth_id, B) if self.cfg.adanorm_num_embeddings else None
        self._last_B = B
        with torch.cuda.device(self.device):
            need = int(self.lib.kk_vocos_workspace_bytes(self._h, B, T))
            if need == 0:
                raise KokoroHipError(f"Vocos: the workspace could not be sized for B = {B}, T = {T}: {(self.lib.kk_last_error() or b'').decode()}")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            pcm = torch.empty((B, int(self.lib.kk_vocos_samples(self._h, T))), dtype=torch.float32, device=self.device)
            check(self.lib.kk_vocos_forward(self._h, _stream(self.device), B, T, _P(x), _P(cond), _P(self._ws), self._ws.numel(), _P(pcm)), "kk_vocos_forward")
        return pcm

    def debug_fetch(self, name: str) -> torch.Tensor:
        """An intermediate of the last call as float32 [B, rows, channels]: embed, block<i>, backbone, head."""
        rows, ch = C.c_int64(0), C.c_int64(0)
        check(self.lib.kk_vocos_debug_info(self._h, name.encode(), C.byref(rows), C.byref(ch)), "kk_vocos_debug_info")
        out = torch.empty((self._last_B, rows.value, ch.value), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kk_vocos_debug_fetch(self._h, _stream(self.device), name.encode(), C.c_void_p(out.data_ptr())), "kk_vocos_debug_fetch")
        return out
