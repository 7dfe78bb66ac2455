"""Host mirror of the reference's BigVGAN vocoder (mlx_audio/codec/models/bigvgan/bigvgan.py): `BigVGAN(cfg, weights)`, `model(mel)`,
`from_pretrained` (a LOCAL directory only), and `amp_act`, the fused anti-aliased Snake activation on its own.  The arithmetic runs in
libkokoro_hip.so (kk_bigvgan_*, kk_op_bigvgan_amp_act; csrc/kk_bigvgan.hip); PyTorch allocates device memory and provides the stream.

Not built (the refusal names the field): `activation="snake"`, a `resblock` other than "1" / "2", ragged batches (`lengths=`, or a list of mels of
different lengths), and any Activation1d other than up_ratio = down_ratio = 2 with 12 taps (the only form the reference instantiates)."""
from __future__ import annotations

import ctypes as C
import glob
import json
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import torch

from . import _lib
from ._lib import KokoroHipError, check


@dataclass
class BigVGANConfig:
    """The reference's BigVGANConfig (bigvgan.py:14-26), with its defaults."""
    num_mels: int
    upsample_rates: List[int]
    upsample_kernel_sizes: List[int]
    upsample_initial_channel: int
    resblock: str
    resblock_kernel_sizes: List[int]
    resblock_dilation_sizes: List[List[int]]
    activation: str
    snake_logscale: bool
    use_bias_at_final: bool = True
    use_tanh_at_final: bool = True

    @classmethod
    def from_dict(cls, d: dict) -> "BigVGANConfig":
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__})


def _v2(num_mels, rates, kernels, final) -> BigVGANConfig:
    return BigVGANConfig(num_mels=num_mels, upsample_rates=rates, upsample_kernel_sizes=kernels, upsample_initial_channel=1536, resblock="1",
                         resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation="snakebeta",
                         snake_logscale=True, use_bias_at_final=final, use_tanh_at_final=final)


def bigvgan_v2_24khz_100band_256x() -> BigVGANConfig:
    """config.json of the public `bigvgan_v2_24khz_100band_256x` checkpoint (the first reference test configuration, with 100 mel bands)."""
    return _v2(100, [4, 4, 2, 2, 2, 2], [8, 8, 4, 4, 4, 4], True)


def bigvgan_v2_44khz_128band_512x() -> BigVGANConfig:
    """The reference's second test configuration: no bias and a clip instead of tanh at the end."""
    return _v2(128, [8, 4, 2, 2, 2, 2], [16, 8, 4, 4, 4, 4], False)


def _refuse(cfg: BigVGANConfig) -> None:
    if cfg.activation == "snake":
        raise NotImplementedError('activation="snake" is not built: the reference\'s Snake indexes alpha along the TIME axis (activation.py:18, '
                                  "alpha[None, :, None] on a channels-last tensor), which does not broadcast for T != C")
    if cfg.activation != "snakebeta":
        raise ValueError(f"activation must be snakebeta, got {cfg.activation!r}")
    if str(cfg.resblock) not in ("1", "2"):
        raise NotImplementedError(f"resblock={cfg.resblock!r} is not built: only AMPBlock1 (\"1\") and AMPBlock2 (\"2\")")
    if len(cfg.upsample_rates) != len(cfg.upsample_kernel_sizes) or not 1 <= len(cfg.upsample_rates) <= 8:
        raise ValueError("upsample_rates and upsample_kernel_sizes must hold the same 1 .. 8 entries")
    if len(cfg.resblock_kernel_sizes) != len(cfg.resblock_dilation_sizes) or not 1 <= len(cfg.resblock_kernel_sizes) <= 4:
        raise ValueError("resblock_kernel_sizes and resblock_dilation_sizes must hold the same 1 .. 4 entries")
    if any(not 1 <= len(d) <= 4 for d in cfg.resblock_dilation_sizes):
        raise ValueError("every list of resblock_dilation_sizes must hold 1 .. 4 dilations")


FILTER_SHAPE = (1, 12, 1)  # kaiser_sinc_filter1d's result (resample.py:19)


def param_shapes(cfg: BigVGANConfig) -> Dict[str, tuple]:
    """Every parameter of the reference's module tree, by name, with its MLX shape: what `load_weights` consumes.  The `*.filter` entries are
    constants of the architecture: optional in a checkpoint, checked against the host-made taps when present."""
    _refuse(cfg)
    out: Dict[str, tuple] = {}

    def conv(p, o, k, i, bias=True):  # WNConv1d (conv.py:15-45)
        out[p + ".weight_g"], out[p + ".weight_v"] = (o, 1, 1), (o, k, i)
        if bias:
            out[p + ".bias"] = (o,)

    def act(p, c):  # Activation1d(SnakeBeta) (resample.py:157-171)
        out[p + ".act.alpha"], out[p + ".act.beta"] = (c,), (c,)
        out[p + ".upsample.filter"] = out[p + ".downsample.lowpass.filter"] = FILTER_SHAPE

    ch = cfg.upsample_initial_channel
    conv("conv_pre", ch, 7, cfg.num_mels)
    nk = len(cfg.resblock_kernel_sizes)
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        ci, co = ch // 2**i, ch // 2 ** (i + 1)
        p = f"ups.{i}.0"  # WNConvTranspose1d (conv.py:63-92): the norm keeps axis 2
        out[p + ".weight_g"], out[p + ".weight_v"], out[p + ".bias"] = (1, 1, ci), (co, k, ci), (co,)
        for j, (rk, dils) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
            p = f"resblocks.{i * nk + j}"
            for m in range(len(dils)):
                if str(cfg.resblock) == "1":
                    conv(f"{p}.convs1.{m}", co, rk, co)
                    conv(f"{p}.convs2.{m}", co, rk, co)
                    act(f"{p}.activations.{2 * m}", co)
                    act(f"{p}.activations.{2 * m + 1}", co)
                else:
                    conv(f"{p}.convs.{m}", co, rk, co)
                    act(f"{p}.activations.{m}", co)
    co = ch // 2 ** len(cfg.upsample_rates)
    act("activation_post", co)
    conv("conv_post", 1, 7, co, bias=cfg.use_bias_at_final)
    return out


def sanitize(cfg: BigVGANConfig, weights) -> Dict[str, np.ndarray]:
    """BigVGAN.sanitize (bigvgan.py:124-149) restated: PyTorch-layout tensors become MLX layout wherever a shape differs from `param_shapes`."""
    want, out = param_shapes(cfg), {}
    for key, value in weights.items():
        if "num_batches_tracked" in key:
            continue
        value = np.asarray(value)
        shape = want.get(key)
        if shape is not None and ("conv" in key or "lowpass.filter" in key or "upsample.filter" in key) and value.ndim == 3 and value.shape != tuple(shape):
            value = value.transpose(0, 2, 1)
        if shape is not None and "ups." in key and value.ndim == 3 and value.shape != tuple(shape):
            value = value.transpose(1, 2, 0)
        out[key] = value
    return out


def filter_taps() -> np.ndarray:
    """The 12 taps both filters of Activation1d share, as the library makes them (float64 on the host, rounded to float32 once)."""
    taps = (C.c_float * 12)()
    check(_lib.load().kk_op_bigvgan_filter(2, 2, 12, taps), "kk_op_bigvgan_filter")
    return np.array(taps, np.float32)


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def amp_act(x, alpha, beta, logscale: bool, out=None, seg: int = 0):
    """Activation1d(SnakeBeta(alpha, beta)) on its own: x [B][L][C] float32 or bfloat16 on the device (unit stride along C; a view of a wider
    tensor keeps its pitch), alpha / beta [C] as a checkpoint holds them.  Returns `out` (same shape and dtype; allocated when None).
    seg: rows per time segment of a lane, 0 = chosen by shape."""
    if x.ndim != 3 or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda or x.stride(2) != 1:
        raise ValueError("x must be a device tensor [B][L][C], float32 or bfloat16, with unit stride along C")
    B, L, Cc = x.shape
    a, b = (torch.as_tensor(t).detach().to("cpu", torch.float64).reshape(-1) for t in (alpha, beta))
    if a.numel() != Cc or b.numel() != Cc:
        raise ValueError(f"alpha and beta must hold {Cc} values")
    if logscale:
        a, b = a.exp(), b.exp()
    at, bt = a.to(torch.float32).to(x.device), (1.0 / (b + 1e-9)).to(torch.float32).to(x.device)
    if out is None:
        out = torch.empty((B, L, Cc), dtype=x.dtype, device=x.device)
    if tuple(out.shape) != (B, L, Cc) or out.dtype != x.dtype or out.device != x.device or out.stride(2) != 1:
        raise ValueError(f"out: need {(B, L, Cc)} of x's dtype on x's device with unit stride along C")
    with torch.cuda.device(x.device):
        check(_lib.load().kk_op_bigvgan_amp_act(_stream(x.device), B, C.c_void_p(x.data_ptr()), x.stride(0) if B > 1 else L * x.stride(1), x.stride(1),
                                                _lib.KK_BF16 if x.dtype == torch.bfloat16 else _lib.KK_F32, L, Cc, C.c_void_p(at.data_ptr()),
                                                C.c_void_p(bt.data_ptr()), C.c_void_p(out.data_ptr()), out.stride(0) if B > 1 else L * out.stride(1),
                                                out.stride(1), int(seg)), "kk_op_bigvgan_amp_act")
    return out


class BigVGAN:
    def __init__(self, cfg: BigVGANConfig, weights=None, device: str = "cuda:0", compute_dtype: str = "float32"):
        _refuse(cfg)  # (on the host, before the library is touched)
        if compute_dtype not in ("float32", "bfloat16"):
            raise ValueError("compute_dtype must be float32 or bfloat16")
        self.cfg, self.compute_dtype, self.device = cfg, compute_dtype, torch.device(device)
        self.lib = _lib.load()
        kc = _lib.KKBigVGANConfig()
        kc.num_mels, kc.upsample_initial_channel, kc.n_upsamples = int(cfg.num_mels), int(cfg.upsample_initial_channel), len(cfg.upsample_rates)
        for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            kc.upsample_rates[i], kc.upsample_kernel_sizes[i] = int(u), int(k)
        kc.resblock, kc.n_resblock_kernels = int(cfg.resblock), len(cfg.resblock_kernel_sizes)
        for j, (k, dils) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
            kc.resblock_kernel_sizes[j], kc.n_dilations[j] = int(k), len(dils)
            for m, d in enumerate(dils):
                kc.resblock_dilation_sizes[j][m] = int(d)
        kc.snake_logscale, kc.use_bias_at_final, kc.use_tanh_at_final = int(bool(cfg.snake_logscale)), int(bool(cfg.use_bias_at_final)), int(bool(cfg.use_tanh_at_final))
        kc.compute_dtype = _lib.KK_BF16 if compute_dtype == "bfloat16" else _lib.KK_F32
        h = C.c_void_p()
        check(self.lib.kk_bigvgan_create(C.byref(kc), C.byref(h)), "kk_bigvgan_create")
        self._h, self._final, self._ws, self._last_B = h, False, None, 0
        if weights is not None:
            self.load_weights(weights)

    def share(self) -> "BigVGAN":
        """A second BigVGAN on the SAME kk_bigvgan (its weights are immutable after finalize; a forward takes a caller-owned workspace): own
        workspace, for another HIP stream / host thread in flight.  Keeps this one alive; only the original destroys the handle."""
        import copy

        other = copy.copy(self)
        other._parent, other._ws = self, None
        return other

    def __del__(self):
        try:
            if getattr(self, "_h", None) and getattr(self, "_parent", None) is None:
                self.lib.kk_bigvgan_destroy(self._h)
            self._h = None
        except Exception:
            pass

    @property
    def hop_length(self) -> int:
        return int(np.prod(self.cfg.upsample_rates))

    @classmethod
    def from_pretrained(cls, local_dir, **kw) -> "BigVGAN":
        """A LOCAL directory with config.json + *.safetensors (MLX or PyTorch layout, see `sanitize`).  Nothing is fetched."""
        if not os.path.isdir(str(local_dir)):
            raise FileNotFoundError(f"{local_dir} is not a local directory (BigVGAN.from_pretrained never goes to the network)")
        cfg_path, files = os.path.join(local_dir, "config.json"), sorted(glob.glob(os.path.join(str(local_dir), "*.safetensors")))
        if not os.path.exists(cfg_path):
            raise FileNotFoundError(cfg_path)
        if not files:
            raise FileNotFoundError(os.path.join(str(local_dir), "*.safetensors"))
        from safetensors.numpy import load_file

        with open(cfg_path, "r") as f:
            model = cls(BigVGANConfig.from_dict(json.load(f)), **kw)
        weights = {}
        for p in files:
            weights.update(load_file(p))
        return model.load_weights(sanitize(model.cfg, weights))

    def load_weights(self, weights) -> "BigVGAN":
        """The reference's parameter names in MLX layout (`param_shapes`).  A missing name or a wrong shape fails with the name; names the module
        tree does not have are ignored.  Filter tensors, where present, must equal the host-made taps within 1e-6."""
        weights = dict(weights.items() if hasattr(weights, "items") else weights)
        want = param_shapes(self.cfg)
        taps = None
        for name, shape in want.items():
            if name.endswith(".filter"):
                if name in weights:
                    taps = filter_taps() if taps is None else taps
                    got = np.asarray(weights[name], np.float64).reshape(-1)
                    if got.size != 12 or np.abs(got - taps).max() > 1e-6:
                        raise ValueError(f"BigVGAN.load_weights: {name} is not kaiser_sinc_filter1d(0.25, 0.3, 12): only up_ratio = down_ratio = 2 with 12 taps is built")
                continue
            if name not in weights:
                raise ValueError(f"BigVGAN.load_weights: missing parameter: {name}")
            if tuple(np.shape(weights[name])) != tuple(shape):
                raise ValueError(f"BigVGAN.load_weights: {name} has shape {tuple(np.shape(weights[name]))}, expected {tuple(shape)}")
        for name in want:
            if name.endswith(".filter"):
                continue
            a = np.ascontiguousarray(np.asarray(weights[name], np.float32))
            shp = (C.c_int64 * a.ndim)(*a.shape)
            check(self.lib.kk_bigvgan_load_tensor(self._h, name.encode(), shp, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_bigvgan_load_tensor")
        if not torch.cuda.is_available():
            raise KokoroHipError("BigVGAN needs a GPU: the vocoder has no CPU fallback")
        with torch.cuda.device(self.device):
            check(self.lib.kk_bigvgan_finalize(self._h, _stream(self.device)), "kk_bigvgan_finalize")
        self._final = True
        return self

    def __call__(self, mel, lengths=None) -> torch.Tensor:
        """mel [B, num_mels, T] float -> audio [B, 1, T prod(upsample_rates)] float32 on the device (bigvgan.py:97-122)."""
        if lengths is not None or (isinstance(mel, (list, tuple)) and len({int(torch.as_tensor(m).shape[-1]) for m in mel}) > 1):
            raise NotImplementedError("lengths: the ragged-batch form is not built; run mels of one length together")
        if not self._final:
            raise KokoroHipError("BigVGAN: load_weights first")
        if isinstance(mel, (list, tuple)):
            mel = torch.stack([torch.as_tensor(m) for m in mel])
        x = torch.as_tensor(mel)
        if x.ndim != 3 or x.shape[1] != self.cfg.num_mels or x.shape[2] < 1:
            raise ValueError(f"mel must be [B, {self.cfg.num_mels}, T], got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).transpose(1, 2).contiguous()  # frames-major, the reference's first transpose
        B, T, _ = x.shape
        self._last_B = B
        with torch.cuda.device(self.device):
            n_out = int(self.lib.kk_bigvgan_samples(self._h, T))
            need = int(self.lib.kk_bigvgan_workspace_bytes(self._h, B, T))
            if need == 0:
                raise KokoroHipError(f"BigVGAN: the workspace could not be sized for B = {B}, T = {T}: {(self.lib.kk_last_error() or b'').decode()}")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            pcm = torch.empty((B, 1, n_out), dtype=torch.float32, device=self.device)
            check(self.lib.kk_bigvgan_forward(self._h, _stream(self.device), B, T, C.c_void_p(x.data_ptr()), C.c_void_p(self._ws.data_ptr()), self._ws.numel(),
                                              C.c_void_p(pcm.data_ptr())), "kk_bigvgan_forward")
        return pcm

    def debug_fetch(self, name: str) -> torch.Tensor:
        """An intermediate of the last call as float32 [B, rows, channels]: conv_pre, stage<i>, activation_post."""
        rows, ch = C.c_int64(0), C.c_int64(0)
        check(self.lib.kk_bigvgan_debug_info(self._h, name.encode(), C.byref(rows), C.byref(ch)), "kk_bigvgan_debug_info")
        out = torch.empty((self._last_B, rows.value, ch.value), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kk_bigvgan_debug_fetch(self._h, _stream(self.device), name.encode(), C.c_void_p(out.data_ptr())), "kk_bigvgan_debug_fetch")
        return out
