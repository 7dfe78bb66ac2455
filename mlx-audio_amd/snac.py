"""Host mirror of the reference's SNAC codec (mlx_audio/codec/models/snac/snac.py): `SNAC(cfg)`, `.encode(audio)`, `.decode(codes)`,
`.preprocess(audio)`, `from_config`, `from_pretrained` (a LOCAL directory only), and the two Orpheus helpers of
mlx_audio/tts/models/llama/llama.py.  The arithmetic runs in libkokoro_hip.so (kk_snac_*, csrc/kk_snac.hip); PyTorch allocates device memory
and provides the stream.

The reference's port is restated as written, not upstream PyTorch SNAC: transposed convs without output padding (an odd stride s gives
L s - 1 rows), NoiseBlock noise of shape [B, 1, C] (one normal per item and channel, constant over time), a no-op residual crop.
Not built (NotImplementedError names the field): `attn_window_size` (the LocalMHA of the 32 / 44 kHz checkpoints), `depthwise=False`, the
ragged-batch form (`lengths=`), and `__call__` (the encode -> decode round trip)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import KokoroHipError, check


@dataclass
class SNACConfig:
    """The constructor arguments of the reference's SNAC (snac.py:16-30), with its defaults."""
    sampling_rate: int = 44100
    encoder_dim: int = 64
    encoder_rates: List[int] = field(default_factory=lambda: [3, 3, 7, 7])
    latent_dim: Optional[int] = None
    decoder_dim: int = 1536
    decoder_rates: List[int] = field(default_factory=lambda: [7, 7, 3, 3])
    attn_window_size: Optional[int] = 32
    codebook_size: int = 4096
    codebook_dim: int = 8
    vq_strides: List[int] = field(default_factory=lambda: [8, 4, 2, 1])
    noise: bool = True
    depthwise: bool = True

    def __post_init__(self):
        if self.latent_dim is None:
            self.latent_dim = self.encoder_dim * (2 ** len(self.encoder_rates))  # snac.py:37-38

    @classmethod
    def from_dict(cls, d: dict) -> "SNACConfig":
        return cls(**{k: v for k, v in d.items() if k in cls.__dataclass_fields__})


def snac_24khz() -> SNACConfig:
    """config.json of the `snac_24khz` checkpoint the Llama TTS family decodes with (llama.py: 7 codes per coarse frame)."""
    return SNACConfig(sampling_rate=24000, encoder_dim=48, encoder_rates=[2, 4, 8, 8], latent_dim=None, decoder_dim=1024, decoder_rates=[8, 8, 4, 2],
                      attn_window_size=None, codebook_size=4096, codebook_dim=8, vq_strides=[4, 2, 1], noise=True, depthwise=True)


def _refuse(cfg: SNACConfig) -> None:
    if cfg.attn_window_size is not None:
        raise NotImplementedError("attn_window_size: LocalMHA (the 32 / 44 kHz checkpoints) is not built; only attn_window_size=None")
    if not cfg.depthwise:
        raise NotImplementedError("depthwise=False (dense residual convolutions) is not built")


def param_shapes(cfg: SNACConfig) -> Dict[str, tuple]:
    """Every parameter of the reference's module tree, by name, with its shape (layers.py, vq.py): what `load_weights` consumes."""
    _refuse(cfg)
    out: Dict[str, tuple] = {}

    def conv(p, o, k, i, bias=True):  # WNConv1d (layers.py:17-47)
        out[p + ".weight_g"], out[p + ".weight_v"] = (o, 1, 1), (o, k, i)
        if bias:
            out[p + ".bias"] = (o,)

    def convt(p, i, k, o):  # WNConvTranspose1d (layers.py:64-95)
        out[p + ".weight_g"], out[p + ".weight_v"], out[p + ".bias"] = (i, 1, 1), (i, k, o), (o,)

    def unit(p, c):  # ResidualUnit (layers.py:208-224), depth-wise
        out[p + ".block.layers.0.alpha"] = (1, c, 1)
        conv(p + ".block.layers.1", c, 7, 1)
        out[p + ".block.layers.2.alpha"] = (1, c, 1)
        conv(p + ".block.layers.3", c, 1, c)

    d = cfg.encoder_dim
    e = "encoder.block.layers."
    conv(e + "0", d, 7, 1)
    for l, s in enumerate(cfg.encoder_rates):  # EncoderBlock (layers.py:234-250)
        p = f"{e}{l + 1}.block.layers."
        for i in range(3):
            unit(p + str(i), d)
        out[p + "3.alpha"] = (1, d, 1)
        conv(p + "4", 2 * d, 2 * s, d)
        d *= 2
    conv(f"{e}{len(cfg.encoder_rates) + 1}", d, 7, 1)
    D = cfg.latent_dim
    for i in range(len(cfg.vq_strides)):  # VectorQuantize (vq.py:11-21)
        p = f"quantizer.quantizers.{i}"
        conv(p + ".in_proj", cfg.codebook_dim, 1, D)
        conv(p + ".out_proj", D, 1, cfg.codebook_dim)
        out[p + ".codebook.weight"] = (cfg.codebook_size, cfg.codebook_dim)
    m = "decoder.model.layers."
    conv(m + "0", D, 7, 1)
    conv(m + "1", cfg.decoder_dim, 1, D)
    co = cfg.decoder_dim
    for l, s in enumerate(cfg.decoder_rates):  # DecoderBlock (layers.py:270-294)
        ci, co = cfg.decoder_dim // 2**l, cfg.decoder_dim // 2 ** (l + 1)
        p = f"{m}{l + 2}.block.layers."
        out[p + "0.alpha"] = (1, ci, 1)
        convt(p + "1", ci, 2 * s, co)
        at = 2
        if cfg.noise:
            conv(f"{p}{at}.linear", co, 1, co, bias=False)
            at += 1
        for i in range(3):
            unit(p + str(at + i), co)
    n = len(cfg.decoder_rates)
    out[f"{m}{n + 2}.alpha"] = (1, co, 1)
    conv(f"{m}{n + 3}", 1, 7, co)
    return out


def codes_from_orpheus(code_list) -> List[torch.Tensor]:
    """llama.py:31-47 decode_audio_from_codes: a flat list of 7 n Orpheus audio codes, slot k of a frame carrying its `k * 4096` offset ->
    the three SNAC code tensors [1, n], [1, 2 n], [1, 4 n] (int32, host) that `SNAC.decode` takes."""
    c = torch.as_tensor(code_list, dtype=torch.int64).reshape(-1)
    n = c.numel() // 7
    f = c[: 7 * n].reshape(n, 7)
    l1 = f[:, 0]
    l2 = torch.stack([f[:, 1] - 4096, f[:, 4] - 4 * 4096], dim=1).reshape(-1)
    l3 = torch.stack([f[:, 2] - 2 * 4096, f[:, 3] - 3 * 4096, f[:, 5] - 5 * 4096, f[:, 6] - 6 * 4096], dim=1).reshape(-1)
    return [l1[None].to(torch.int32), l2[None].to(torch.int32), l3[None].to(torch.int32)]


def codes_to_orpheus(codes: Sequence) -> List[int]:
    """llama.py encode_audio_to_codes: SNAC codes of ONE item ([1, n], [1, 2 n], [1, 4 n]) -> the flat 7-slot interleave
    [L1, L2 + 4096, L3 + 2 * 4096, L3 + 3 * 4096, L2 + 4 * 4096, L3 + 5 * 4096, L3 + 6 * 4096] per coarse frame."""
    if len(codes) != 3:
        raise ValueError("the Orpheus layout has three code books (strides 4, 2, 1)")
    l1, l2, l3 = (torch.as_tensor(c).to("cpu", torch.int64) for c in codes)
    if l1.ndim != 2 or l1.shape[0] != 1 or l2.shape != (1, 2 * l1.shape[1]) or l3.shape != (1, 4 * l1.shape[1]):
        raise ValueError("codes must be [1, n], [1, 2 n], [1, 4 n]")
    n = l1.shape[1]
    l2, l3 = l2.reshape(n, 2), l3.reshape(n, 4)
    f = torch.stack([l1[0], l2[:, 0] + 4096, l3[:, 0] + 2 * 4096, l3[:, 1] + 3 * 4096, l2[:, 1] + 4 * 4096, l3[:, 2] + 5 * 4096, l3[:, 3] + 6 * 4096], dim=1)
    return f.reshape(-1).tolist()


class SNAC:
    def __init__(self, cfg: SNACConfig, weights: Dict[str, np.ndarray] | None = None, device: str = "cuda:0", compute_dtype: str = "float32"):
        _refuse(cfg)  # (on the host, before the library is touched)
        if compute_dtype not in ("float32", "bfloat16"):
            raise ValueError("compute_dtype must be float32 or bfloat16")
        self.cfg = cfg
        self.compute_dtype = compute_dtype
        self.device = torch.device(device)
        self.lib = _lib.load()
        kc = _lib.KKSnacConfig()
        for k in ("sampling_rate", "encoder_dim", "latent_dim", "decoder_dim", "codebook_size", "codebook_dim"):
            setattr(kc, k, int(getattr(cfg, k)))
        for name, vals in (("encoder_rates", cfg.encoder_rates), ("decoder_rates", cfg.decoder_rates), ("vq_strides", cfg.vq_strides)):
            if not 1 <= len(vals) <= 8:
                raise ValueError(f"{name} must hold 1 .. 8 entries")
            for i, v in enumerate(vals):
                getattr(kc, name)[i] = int(v)
        kc.n_encoder_rates, kc.n_decoder_rates, kc.n_vq = len(cfg.encoder_rates), len(cfg.decoder_rates), len(cfg.vq_strides)
        kc.attn_window_size, kc.noise, kc.depthwise = 0, int(bool(cfg.noise)), 1
        kc.compute_dtype = _lib.KK_BF16 if compute_dtype == "bfloat16" else _lib.KK_F32
        h = C.c_void_p()
        check(self.lib.kk_snac_create(C.byref(kc), C.byref(h)), "kk_snac_create")
        self._h = h
        self._final = False
        self._ws = None
        self._last_B = 0
        if weights is not None:
            self.load_weights(weights)

    def share(self) -> "SNAC":
        """A second SNAC on the SAME kk_snac (its weights are immutable after finalize; decode / encode take a caller-owned workspace): own
        workspace, for another HIP stream / host thread in flight.  Keeps this one alive; only the original destroys the codec."""
        import copy

        other = copy.copy(self)
        other._parent, other._ws = self, None
        return other

    def __del__(self):
        try:
            if getattr(self, "_h", None) and getattr(self, "_parent", None) is None:
                self.lib.kk_snac_destroy(self._h)
            self._h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the reference's attributes (snac.py:32-51)
    @property
    def sampling_rate(self) -> int:
        return self.cfg.sampling_rate

    @property
    def hop_length(self) -> int:
        return int(np.prod(self.cfg.encoder_rates))

    @property
    def n_codebooks(self) -> int:
        return len(self.cfg.vq_strides)

    @property
    def vq_strides(self) -> List[int]:
        return list(self.cfg.vq_strides)

    @property
    def noise_channels(self) -> List[int]:
        """Channels of each decoder block's NoiseBlock (empty without noise): `noise=` of decode holds one [B, 1, C] tensor per entry."""
        return [self.cfg.decoder_dim // 2 ** (l + 1) for l in range(len(self.cfg.decoder_rates))] if self.cfg.noise else []

    @classmethod
    def from_config(cls, config_path, **kw) -> "SNAC":
        with open(config_path, "r") as f:
            return cls(SNACConfig.from_dict(json.load(f)), **kw)

    @classmethod
    def from_pretrained(cls, local_dir, **kw) -> "SNAC":
        """snac.py:126-141 for a LOCAL directory with config.json + model.safetensors.  Nothing is fetched."""
        if not os.path.isdir(str(local_dir)):
            raise FileNotFoundError(f"{local_dir} is not a local directory (SNAC.from_pretrained never goes to the network)")
        cfg_path, w_path = os.path.join(local_dir, "config.json"), os.path.join(local_dir, "model.safetensors")
        for p in (cfg_path, w_path):
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        from safetensors.numpy import load_file

        model = cls.from_config(cfg_path, **kw)
        return model.load_weights(load_file(w_path))

    def load_weights(self, weights) -> "SNAC":
        """The reference's parameter names and layouts (`param_shapes`).  A missing name or a wrong shape fails with the name; names the
        module tree does not have are ignored the way `strict=False` would."""
        weights = dict(weights.items() if hasattr(weights, "items") else weights)
        want = param_shapes(self.cfg)
        for name, shape in want.items():
            if name not in weights:
                raise ValueError(f"SNAC.load_weights: missing parameter: {name}")
            if tuple(np.shape(weights[name])) != tuple(shape):
                raise ValueError(f"SNAC.load_weights: {name} has shape {tuple(np.shape(weights[name]))}, expected {tuple(shape)}")
        for name in want:
            a = np.ascontiguousarray(np.asarray(weights[name], np.float32))
            shp = (C.c_int64 * a.ndim)(*a.shape)
            check(self.lib.kk_snac_load_tensor(self._h, name.encode(), shp, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_snac_load_tensor")
        if not torch.cuda.is_available():
            raise KokoroHipError("SNAC needs a GPU: the codec has no CPU fallback")
        with torch.cuda.device(self.device):
            check(self.lib.kk_snac_finalize(self._h, self._stream()), "kk_snac_finalize")
        self._final = True
        return self

    def pad_to(self) -> int:
        lcm = 1
        for s in self.cfg.vq_strides:
            lcm = abs(lcm * s) // math.gcd(lcm, s)
        return self.hop_length * lcm

    def preprocess(self, audio):
        """snac.py:67-85: right zero-pad [B, 1, N] to a multiple of hop_length * lcm(vq_strides)."""
        audio = torch.as_tensor(audio)
        n = audio.shape[-1]
        unit = self.pad_to()
        return torch.nn.functional.pad(audio, (0, math.ceil(n / unit) * unit - n))

    def __call__(self, *a, **k):
        raise NotImplementedError("__call__ (the encode -> decode round trip of snac.py:87-93) is not built: call encode and decode")

    def _workspace(self, need: int):
        if need == 0:
            raise KokoroHipError(f"SNAC: the workspace could not be sized: {(self.lib.kk_last_error() or b'').decode()}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def encode(self, audio, lengths=None) -> List[torch.Tensor]:
        """audio [B, 1, N] float -> one int32 tensor [B, T / stride_i] per code book, on the device (snac.py:95-99).  Always fp32 kernels."""
        if lengths is not None or (isinstance(audio, (list, tuple)) and len({int(torch.as_tensor(a).shape[-1]) for a in audio}) > 1):
            raise NotImplementedError("lengths: the ragged-batch form is not built; pad the batch to one length")
        if not self._final:
            raise KokoroHipError("SNAC.encode: load_weights first")
        if isinstance(audio, (list, tuple)):
            audio = torch.stack([torch.as_tensor(a) for a in audio])
        x = torch.as_tensor(audio)
        if x.ndim != 3 or x.shape[1] != 1 or x.shape[2] < 1:
            raise ValueError(f"audio must be [B, 1, N], got {tuple(x.shape)}")
        x = self.preprocess(x).to(device=self.device, dtype=torch.float32).contiguous()
        B, _, N = x.shape
        self._last_B = B
        with torch.cuda.device(self.device):
            T = int(self.lib.kk_snac_encode_frames(self._h, N))
            ws = self._workspace(int(self.lib.kk_snac_encode_workspace_bytes(self._h, B, N)))
            codes = [torch.empty((B, T // s), dtype=torch.int32, device=self.device) for s in self.cfg.vq_strides]
            ptrs = (C.c_void_p * len(codes))(*[c.data_ptr() for c in codes])
            check(self.lib.kk_snac_encode(self._h, self._stream(), B, N, C.c_void_p(x.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), ptrs),
                  "kk_snac_encode")
        return codes

    def draw_noise(self, B: int, seed: int = 0) -> List[torch.Tensor]:
        """The NoiseBlocks' normals as decode(noise=None, seed=seed) draws them: one [B, 1, C] float32 tensor per decoder block; item b comes
        from a torch.Generator seeded with seed + b (blocks in order), so an item's audio does not depend on its batch."""
        chans = self.noise_channels
        out = [torch.empty((B, 1, c), dtype=torch.float32) for c in chans]
        for b in range(B):
            g = torch.Generator().manual_seed(int(seed) + b)
            for l, c in enumerate(chans):
                out[l][b, 0] = torch.randn(c, generator=g, dtype=torch.float32)
        return out

    def decode(self, codes, noise=None, seed: int = 0, lengths=None) -> torch.Tensor:
        """codes: one integer tensor [B, T / stride_i] per code book -> audio [B, N, 1] float32 on the device, the reference's channels-last
        result (snac.py:101-104).  noise: one [B, 1, C_i] float tensor per decoder block (`noise_channels`), or None to draw them
        (`draw_noise(B, seed)`)."""
        if lengths is not None:
            raise NotImplementedError("lengths: the ragged-batch form is not built; decode items of one length together")
        if not self._final:
            raise KokoroHipError("SNAC.decode: load_weights first")
        strides = self.cfg.vq_strides
        if len(codes) != len(strides):
            raise ValueError(f"codes must hold {len(strides)} tensors, got {len(codes)}")
        cs = [torch.as_tensor(c).to(device=self.device, dtype=torch.int32).contiguous() for c in codes]
        if any(c.ndim != 2 or c.shape[0] != cs[0].shape[0] or c.shape[1] < 1 for c in cs):
            raise ValueError("every code tensor must be [B, T / stride_i] with one B")
        B, T = int(cs[0].shape[0]), int(cs[0].shape[1]) * strides[0]
        if any(int(c.shape[1]) * s != T for c, s in zip(cs, strides)):
            raise ValueError(f"code lengths {[int(c.shape[1]) for c in cs]} do not describe one latent length under strides {list(strides)}")
        chans = self.noise_channels
        ns = []
        if chans:
            noise = self.draw_noise(B, seed) if noise is None else list(noise)
            if len(noise) != len(chans):
                raise ValueError(f"noise must hold {len(chans)} tensors, got {len(noise)}")
            for n, c in zip(noise, chans):
                n = torch.as_tensor(n)
                if tuple(n.shape) != (B, 1, c):
                    raise ValueError(f"a noise tensor has shape {tuple(n.shape)}, expected {(B, 1, c)}")
                ns.append(n.to(device=self.device, dtype=torch.float32).contiguous())
        self._last_B = B
        with torch.cuda.device(self.device):
            n_out = int(self.lib.kk_snac_decode_samples(self._h, T))
            ws = self._workspace(int(self.lib.kk_snac_decode_workspace_bytes(self._h, B, T)))
            pcm = torch.empty((B, n_out, 1), dtype=torch.float32, device=self.device)
            cp = (C.c_void_p * len(cs))(*[c.data_ptr() for c in cs])
            npp = (C.c_void_p * len(ns))(*[n.data_ptr() for n in ns]) if ns else None
            check(self.lib.kk_snac_decode(self._h, self._stream(), B, T, cp, npp, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(pcm.data_ptr())),
                  "kk_snac_decode")
        return pcm

    def debug_fetch(self, name: str) -> torch.Tensor:
        rows, ch = C.c_int64(0), C.c_int64(0)
        check(self.lib.kk_snac_debug_info(self._h, name.encode(), C.byref(rows), C.byref(ch)), "kk_snac_debug_info")
        out = torch.empty((self._last_B, rows.value, ch.value), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kk_snac_debug_fetch(self._h, self._stream(), name.encode(), C.c_void_p(out.data_ptr())), "kk_snac_debug_fetch")
        return out
