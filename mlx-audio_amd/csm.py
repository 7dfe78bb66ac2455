"""Host mirror of the reference's CSM frame generator surface (mlx_audio/tts/models/sesame/sesame.py:276-415): `SesameModel` with
`setup_caches`, `reset_caches`, `generate_frame(tokens, tokens_mask, input_pos, ...)`.  The arithmetic runs in libkokoro_hip.so
(kk_csm_*, csrc/kk_csm.hip).  The text tokenizer, prompt building and the generation loop (sesame.py:484-817) are host code of the
reference that can call this class unchanged; they need the Llama-3.2 tokenizer files, which are not available offline."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import KokoroHipError, check


def _llama_args(d: dict) -> _lib.KKLlamaArgs:
    a = _lib.KKLlamaArgs()
    for k in ("num_layers", "num_heads", "num_kv_heads", "head_dim", "hidden", "intermediate"):
        setattr(a, k, int(d[k]))
    a.rope_theta, a.rope_factor, a.rms_eps = float(d["rope_theta"]), float(d["rope_factor"]), float(d["rms_eps"])
    return a


def _sampler_struct(sampler) -> _lib.KKCsmSampler:
    """kk_csm_sampler of anything with temp / top_k (and optionally top_p / min_p / min_tokens_to_keep), e.g. sesame.Sampler; no seed, no device RNG"""
    return _lib.KKCsmSampler(float(sampler.temp), int(sampler.top_k), float(getattr(sampler, "top_p", 0.0)), float(getattr(sampler, "min_p", 0.0)),
                             int(getattr(sampler, "min_tokens_to_keep", 1)), 0, 0)


class Prefix:
    """kk_csm_prefix: the backbone K / V of a prompt's first `length` frames on the device, immutable, shared by every stream admitted on top of
    it (`SesameModel.admit(..., prefix=)`).  Usable from the generator it was made on and from its `share()`s.  Freed by `close()` / on collection."""

    def __init__(self, lib, handle, length: int, device, owner):
        self.lib, self._h, self.length, self.device = lib, handle, int(length), device
        self._owner = owner  # the weights outlive the prefix

    @property
    def nbytes(self) -> int:
        return int(self.lib.kk_csm_prefix_bytes(self._h)) if self._h else 0

    def save(self) -> torch.Tensor:
        """A copy of the buffer, [layers, 2 (K, V), length, kv_heads * head_dim] float32 as one flat device tensor."""
        if not self._h:
            raise ValueError("Prefix.save: the prefix is closed")
        out = torch.empty(self.nbytes // 4, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kk_csm_prefix_read(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.c_void_p(out.data_ptr()),
                                              out.numel() * 4), "kk_csm_prefix_read")
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.kk_csm_prefix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SesameModel:
    def __init__(self, cfg: dict, weights: Optional[Dict[str, np.ndarray]] = None, device: str = "cuda:0", weight_dtype: str = "float32",
                 quantization: Optional[dict] = None, weight_storage: str = "packed"):
        """quantization: config["quantization"] of an MLX affine-quantised checkpoint ({"group_size", "bits"} + per-layer overrides); `weights`
        then holds `{p}.weight` (uint32) / `{p}.scales` / `{p}.biases` triplets.  weight_storage "packed" (default): the Linears stay quantised
        in device memory and are decoded inside the matrix-core kernels (kk_csm_load_quantized) -- the bits of bf16 weight mode on the
        dequantised checkpoint; where the library cannot do that for the whole model it dequantises on the host (`weight_fallback` says
        why).  "dequantized": dequantise here and run bf16 weight mode."""
        if weight_storage not in ("packed", "dequantized"):
            raise ValueError(f"weight_storage must be 'packed' or 'dequantized', not {weight_storage!r}")
        self.quantization, self.weight_storage = quantization, weight_storage
        if quantization is not None:
            weight_dtype = "bfloat16"  # the arithmetic of a quantised checkpoint: fp32 on the bf16 rounding of scale * q + bias
        self.cfg = cfg
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise KokoroHipError("SesameModel needs a GPU: the frame generator has no CPU fallback")
        self.device = torch.device(device)
        kc = _lib.KKCsmConfig()
        kc.text_vocab_size, kc.audio_vocab_size = int(cfg["text_vocab_size"]), int(cfg["audio_vocab_size"])
        kc.audio_num_codebooks, kc.max_seq_len = int(cfg["audio_num_codebooks"]), int(cfg["max_seq_len"])
        kc.backbone, kc.decoder = _llama_args(cfg["backbone"]), _llama_args(cfg["decoder"])
        h = C.c_void_p()
        check(self.lib.kk_csm_create(C.byref(kc), C.byref(h)), "kk_csm_create")
        self._h = h
        # "bfloat16": what load_model does for a bf16 checkpoint (it keeps the checkpoint's dtype, tts/utils.py:217-262) -- the Linear
        # matrices are stored as bf16 and streamed as such by the single-token steps; arithmetic stays fp32
        self.weight_dtype = weight_dtype
        if weight_dtype != "float32":
            check(self.lib.kk_csm_set_weight_dtype(self._h, {"bfloat16": _lib.KK_BF16}[weight_dtype]), "kk_csm_set_weight_dtype")
        self._final = False
        self._ws = None
        self._enabled = False
        self.max_batch = 0
        self._graph = False
        self._gbuf = {}
        self._sid = {}
        self._ws_admit = None
        if weights is not None:
            self.load_weights(weights)

    def share(self) -> "SesameModel":
        """kk_csm_share: a second generator on the SAME device weights (own KV caches, positions, logits, graph cache) for another stream /
        thread in flight.  It keeps this one alive."""
        import copy

        if not self._final:
            raise KokoroHipError("SesameModel.share: load_weights first")
        other = copy.copy(self)
        h = C.c_void_p()
        check(self.lib.kk_csm_share(self._h, C.byref(h)), "kk_csm_share")
        other._h, other._parent = h, self
        other._ws, other._enabled, other.max_batch, other._graph, other._gbuf, other._sid = None, False, 0, False, {}, {}
        other._ws_admit = None
        return other

    def weights_root(self) -> "SesameModel":
        """The generator that owns the device weights this one runs on (itself, unless it came from `share()`)."""
        m = self
        while getattr(m, "_parent", None) is not None:
            m = m._parent
        return m

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.kk_csm_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def load_weights(self, weights: Dict[str, np.ndarray]) -> "SesameModel":
        triplets = {}
        if self.quantization is not None:
            from .quant import dequantize_affine, split_triplets

            q = self.quantization
            per_layer = {k: v for k, v in q.items() if k not in ("group_size", "bits")}
            weights, triplets = split_triplets(weights, int(q["group_size"]), int(q["bits"]), per_layer)
            if self.weight_storage == "dequantized":
                weights = dict(weights, **{k: dequantize_affine(*t) for k, t in triplets.items()})
                triplets = {}
        with torch.cuda.device(self.device):
            for name, (words, scales, biases, group, bits) in triplets.items():
                O, I = words.shape[0], words.shape[1] * (32 // bits)
                if scales.shape != (O, I // group) or biases.shape != scales.shape:
                    raise ValueError(f"{name}: scales / biases {scales.shape} do not match [{O}, {I}] at group size {group}")
                shp = (C.c_int64 * 2)(O, I)
                check(self.lib.kk_csm_load_quantized(self._h, name.encode(), shp, words.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p),
                                                     biases.ctypes.data_as(C.c_void_p), group, bits), "kk_csm_load_quantized")
            for name, arr in weights.items():
                a = np.ascontiguousarray(np.asarray(arr, np.float32))
                shp = (C.c_int64 * a.ndim)(*a.shape)
                check(self.lib.kk_csm_load_tensor(self._h, name.encode(), shp, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_csm_load_tensor")
            check(self.lib.kk_csm_finalize(self._h, self._stream()), "kk_csm_finalize")
        self._final = True
        return self

    @property
    def weight_format(self) -> str:
        """kk_csm_weight_format: "f32", "bf16", "q8", "q4" ("q8+q4": packed, per-layer overrides mix the two)."""
        f = int(self.lib.kk_csm_weight_format(self._h))
        if f < 0:
            check(1, "kk_csm_weight_format")
        return "q8+q4" if f & _lib.CSM_WEIGHTS_MIXED else _lib.CSM_WEIGHTS[f & 0xFF]

    @property
    def weight_fallback(self) -> Optional[str]:
        """None, or why a quantised checkpoint was dequantised on the host instead of staying packed."""
        f = int(self.lib.kk_csm_weight_format(self._h))
        if f < 0 or not f & _lib.CSM_WEIGHTS_DEQUANTIZED:
            return None
        return (self.lib.kk_csm_weight_fallback_reason(self._h) or b"").decode() or "fell back to dequantised"

    @property
    def weight_bytes(self) -> Dict[str, int]:
        """kk_csm_weight_bytes: device bytes held for the Linear matrices / for all weights."""
        lin, tot = C.c_size_t(0), C.c_size_t(0)
        check(self.lib.kk_csm_weight_bytes(self._h, C.byref(lin), C.byref(tot)), "kk_csm_weight_bytes")
        return {"linear": int(lin.value), "total": int(tot.value)}

    # ---- sesame.py:320-345
    def setup_caches(self, max_batch_size: int) -> None:
        with torch.cuda.device(self.device):
            check(self.lib.kk_csm_setup_caches(self._h, int(max_batch_size)), "kk_csm_setup_caches")
        self._gbuf = {}  # the library dropped its captured graphs with the old caches; their staging buffers go with them
        self._enabled = True
        self.max_batch = int(max_batch_size)

    def set_padding(self, pads) -> None:
        """kk_csm_set_padding: left padding (in frames) of every stream's prompt, for batches whose prompts differ in length.  Call on an
        empty cache, before the prompt block; reset_caches clears it."""
        arr = (C.c_int32 * len(pads))(*[int(p) for p in pads])
        check(self.lib.kk_csm_set_padding(self._h, len(pads), arr), "kk_csm_set_padding")

    def caches_are_enabled(self) -> bool:
        return self._enabled

    def reset_caches(self) -> None:
        check(self.lib.kk_csm_reset_caches(self._h), "kk_csm_reset_caches")

    def set_graph_mode(self, on: bool = True) -> None:
        """kk_csm_set_graph_mode: single-token frames are replayed as one hipGraph.  Inputs are staged in buffers that persist across
        calls (a graph is keyed on its pointers); the returned codes are a view that the next frame overwrites."""
        check(self.lib.kk_csm_set_graph_mode(self._h, 1 if on else 0), "kk_csm_set_graph_mode")
        self._graph = bool(on)

    @property
    def position(self) -> int:
        return int(self.lib.kk_csm_position(self._h))

    # ---- sesame.py:349-395
    def generate_frame(self, tokens, tokens_mask, input_pos=None, temperature: float = 0.0, top_k: int = 50, uniforms=None, sampler=None,
                       seed: Optional[int] = None, stream_ids=None, device_rng: bool = False) -> torch.Tensor:
        """tokens [B, S, n_cb+1] int, tokens_mask same shape; `input_pos` (the reference's argument) is checked against the cache position.
        `sampler` (anything with temp / top_k / top_p / min_p / min_tokens_to_keep, e.g. sesame.Sampler) replaces `temperature` / `top_k` and
        brings the top-p / min-p filters (the rule: kk_csm_sampler in kokoro_hip.h).  `uniforms` [B, n_cb] are the injected draws; without them
        and with `seed`, the kernels draw from Philox on (seed, stream id, position, code book) -- `stream_ids` [B] int, default the batch
        index.  Neither: arg-max.  Returns codes [B, n_cb] int32 on the device.
        `sampler="rows"` (kk_csm_generate_frame_rows): item b samples with the settings `set_row_sampler(b, ...)` stored for cache row b -- one
        launch per code book whatever the mix, and a replayed graph that never re-captures when a row's settings change.  `temperature`, `top_k`
        and `seed` are not read then: with `device_rng=True` (and no `uniforms`) every row draws on the seed of ITS entry."""
        assert self.caches_are_enabled(), "backbone caches are not enabled"
        tokens = torch.as_tensor(tokens).to(device=self.device, dtype=torch.int32).contiguous()
        mask = torch.as_tensor(tokens_mask).to(device=self.device, dtype=torch.float32).contiguous()
        B, S, W = tokens.shape
        ncb = self.cfg["audio_num_codebooks"]
        if W != ncb + 1 or tuple(mask.shape) != (B, S, W):
            raise ValueError(f"tokens / tokens_mask must be [B, S, {ncb + 1}]")
        if input_pos is not None:
            ip = np.array(input_pos.cpu() if isinstance(input_pos, torch.Tensor) else input_pos)
            if ip.shape != (B, S) or not np.array_equal(ip, np.broadcast_to(self.position + np.arange(S), (B, S))):
                raise ValueError("input_pos must continue the cache: position + arange(S) for every item")
        u = None
        if uniforms is not None:
            u = torch.as_tensor(uniforms).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(u.shape) != (B, ncb):
                raise ValueError(f"uniforms must be [B, {ncb}]")
        rows = isinstance(sampler, str)
        if rows and sampler != "rows":
            raise ValueError('sampler must be a sampler object or "rows"')
        if rows and seed is not None:
            raise ValueError('sampler="rows": the seeds are those of set_row_sampler; pass device_rng=True to draw on them')
        if device_rng and not rows:
            raise ValueError('device_rng belongs to sampler="rows"; pass `seed` otherwise')
        sp = _lib.KKCsmSampler(float(temperature), int(top_k), 0.0, 0.0, 1, 0, 0)
        if sampler is not None and not rows:
            sp = _sampler_struct(sampler)
        sid = None
        if u is None and (seed is not None or (rows and device_rng)):
            if not rows:
                sp.seed, sp.use_device_rng = int(seed) & 0xFFFFFFFFFFFFFFFF, 1
            if stream_ids is not None:
                sid = self._sid.get(B)  # one persistent buffer per batch size: a replayed graph reads it through the same pointer
                if sid is None:
                    sid = self._sid[B] = torch.empty(B, dtype=torch.int32, device=self.device)
                ids = torch.as_tensor(stream_ids).to(dtype=torch.int32).reshape(-1)
                if ids.numel() != B:
                    raise ValueError(f"stream_ids must hold {B} entries")
                sid.copy_(ids)
        if self._graph and S == 1:
            key = (B, u is not None)
            if key not in self._gbuf:
                self._gbuf[key] = (torch.empty_like(tokens), torch.empty_like(mask), torch.empty((B, ncb), dtype=torch.float32, device=self.device),
                                   torch.empty((B, ncb), dtype=torch.int32, device=self.device))
            gt, gm, gu, gc = self._gbuf[key]
            gt.copy_(tokens)
            gm.copy_(mask)
            if u is not None:
                gu.copy_(u)
                u = gu
            tokens, mask = gt, gm
        with torch.cuda.device(self.device):
            need = int(self.lib.kk_csm_workspace_bytes(self._h, B, S))
            if need == 0:
                raise KokoroHipError("kk_csm_workspace_bytes failed")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            codes = self._gbuf[(B, u is not None)][3] if (self._graph and S == 1) else torch.empty((B, ncb), dtype=torch.int32, device=self.device)
            if rows:
                check(self.lib.kk_csm_generate_frame_rows(self._h, self._stream(), B, S, C.c_void_p(tokens.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                          1 if device_rng else 0, C.c_void_p(u.data_ptr()) if u is not None else None,
                                                          C.c_void_p(sid.data_ptr()) if sid is not None else None,
                                                          C.c_void_p(self._ws.data_ptr()), need, C.c_void_p(codes.data_ptr())), "kk_csm_generate_frame_rows")
            else:
                check(self.lib.kk_csm_generate_frame_ex(self._h, self._stream(), B, S, C.c_void_p(tokens.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                        C.byref(sp), C.c_void_p(u.data_ptr()) if u is not None else None,
                                                        C.c_void_p(sid.data_ptr()) if sid is not None else None,
                                                        C.c_void_p(self._ws.data_ptr()), need, C.c_void_p(codes.data_ptr())), "kk_csm_generate_frame")
        self._last_B = B
        return codes

    def set_row_sampler(self, row: int, sampler, seed: Optional[int] = None) -> None:
        """kk_csm_set_row_sampler: cache row `row` samples with `sampler` (temp / top_k / top_p / min_p / min_tokens_to_keep) in every later
        `generate_frame(..., sampler="rows")`, a replayed graph included; `seed` is the row's Philox seed for frames that draw on the device.
        Written in stream order.  setup_caches and reset_caches_parked zero every entry (arg-max).  ValueError for a row out of range or a
        sampler out of range, before anything is launched."""
        assert self.caches_are_enabled(), "backbone caches are not enabled"
        if not 0 <= int(row) < self.max_batch:
            raise ValueError(f"set_row_sampler: row {row} out of range [0, {self.max_batch})")
        sp = _sampler_struct(sampler)
        if not (sp.temperature >= 0.0 and 0.0 <= sp.top_p <= 1.0 and 0.0 <= sp.min_p <= 1.0 and sp.min_tokens_to_keep >= 1 and sp.top_k >= -1):
            raise ValueError("set_row_sampler: sampler out of range (temp >= 0, top_p and min_p in [0, 1], min_tokens_to_keep >= 1, top_k >= -1)")
        if seed is not None:
            sp.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        with torch.cuda.device(self.device):
            check(self.lib.kk_csm_set_row_sampler(self._h, self._stream(), int(row), C.byref(sp)), "kk_csm_set_row_sampler")

    # ---- continuous batching (kk_csm_admit / park_row / shift_caches / row_state)
    def reset_caches_parked(self) -> None:
        """reset_caches with every row parked: the start of a serving session (streams enter through `admit`)."""
        check(self.lib.kk_csm_reset_caches_parked(self._h), "kk_csm_reset_caches_parked")

    def park(self, row: int) -> None:
        """Retire cache row `row`: from the next frame on it sees no key and appends nothing; `admit` may reuse it."""
        if not 0 <= int(row) < self.max_batch:
            raise ValueError(f"park: row {row} out of range [0, {self.max_batch})")
        check(self.lib.kk_csm_park_row(self._h, int(row)), "kk_csm_park_row")

    def row_state(self):
        """(pad [max_batch] as a list -- max_seq_len marks a parked row --, P): what the next frame will see."""
        assert self.caches_are_enabled(), "backbone caches are not enabled"
        pad, pos = (C.c_int32 * self.max_batch)(), C.c_int32(0)
        check(self.lib.kk_csm_row_state(self._h, pad, C.byref(pos)), "kk_csm_row_state")
        return list(pad), int(pos.value)

    def shift(self, delta: int) -> None:
        """Move every live row's window, and the shared position, by `delta` cache slots (exact: keys carry their stream's own position).
        ValueError if the position or a live window would leave the cache."""
        pad, P = self.row_state()
        mp = int(self.cfg["max_seq_len"])
        delta = int(delta)
        if not 0 <= P + delta <= mp or any(p < mp and p + delta < 0 for p in pad):
            raise ValueError(f"shift by {delta}: a live window would leave the cache [0, {mp}) (position {P}, pad {pad})")
        with torch.cuda.device(self.device):
            check(self.lib.kk_csm_shift_caches(self._h, self._stream(), delta, None, 0), "kk_csm_shift_caches")

    def _admit_workspace(self, S: int):
        need = int(self.lib.kk_csm_workspace_bytes(self._h, 1, max(2, S)))
        if need == 0:
            raise KokoroHipError("kk_csm_workspace_bytes failed")
        # a workspace of its own: the captured frame step of the running batch is keyed on ITS workspace pointer
        if self._ws_admit is None or self._ws_admit.numel() < need:
            self._ws_admit = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws_admit, need

    def make_prefix(self, tokens, tokens_mask) -> Prefix:
        """kk_csm_prefix_create: the backbone K / V of the frames tokens / tokens_mask [n, n_cb+1] at positions 0 .. n-1 as a `Prefix`.  No cache
        row, position or captured graph is touched: legal while a batch runs.  No depth decoder, no sampling."""
        tokens = torch.as_tensor(tokens).to(device=self.device, dtype=torch.int32).contiguous()
        mask = torch.as_tensor(tokens_mask).to(device=self.device, dtype=torch.float32).contiguous()
        ncb = self.cfg["audio_num_codebooks"]
        if tokens.dim() != 2 or tokens.shape[1] != ncb + 1 or mask.shape != tokens.shape:
            raise ValueError(f"tokens / tokens_mask must be [n, {ncb + 1}]")
        n = int(tokens.shape[0])
        if not 1 <= n < int(self.cfg["max_seq_len"]):
            raise ValueError(f"make_prefix: {n} frames; a prefix holds 1 .. max_seq_len - 1 frames")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            ws, need = self._admit_workspace(n)
            check(self.lib.kk_csm_prefix_create(self._h, self._stream(), n, C.c_void_p(tokens.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), need, C.byref(h)), "kk_csm_prefix_create")
        return Prefix(self.lib, h, n, self.device, self)

    def capture_prefix(self, row: int, n: int) -> Prefix:
        """kk_csm_prefix_capture: a copy of the first `n` positions of LIVE cache row `row` (every backbone layer's K and V) as a `Prefix`, the
        class `make_prefix` returns -- `admit(prefix=)` takes it unchanged.  It reads that row's window and writes its own buffer only: the
        position, the paddings and the captured frame step are untouched, so it is legal between two frames of a running batch.  ValueError for
        a row out of range, a parked row, or n outside [1, positions the row holds]."""
        assert self.caches_are_enabled(), "backbone caches are not enabled"
        row, n = int(row), int(n)
        if not 0 <= row < self.max_batch:
            raise ValueError(f"capture_prefix: row {row} out of range [0, {self.max_batch})")
        pad, P = self.row_state()
        if pad[row] >= int(self.cfg["max_seq_len"]):
            raise ValueError(f"capture_prefix: row {row} is parked")
        if not 1 <= n <= P - pad[row]:
            raise ValueError(f"capture_prefix: row {row} holds {P - pad[row]} positions, {n} were asked for")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.kk_csm_prefix_capture(self._h, self._stream(), row, n, C.byref(h)), "kk_csm_prefix_capture")
        return Prefix(self.lib, h, n, self.device, self)

    def admit(self, row: int, tokens, tokens_mask, temperature: float = 0.0, top_k: int = 50, uniforms=None, sampler=None, seed: Optional[int] = None,
              stream_id: int = 0, prefix: Optional[Prefix] = None) -> torch.Tensor:
        """The prompt frame of ONE new stream (tokens / tokens_mask [S, n_cb+1]) into the parked cache row `row` of a running batch; the
        other rows keep their state and the shared position does not move.  Sampling as in generate_frame (`uniforms` [n_cb]; or `seed`
        with `stream_id`: the device generator at the stream's own position S).  Returns codes [n_cb] int32 -- the bits of
        generate_frame on the prompt alone.  ValueError for a live row, a row out of range, or a prompt longer than the position
        (`shift(S - P)` first).
        `prefix` (make_prefix): the stream's prompt is the prefix followed by `tokens`; the prefix's K / V are copied under the suffix instead of
        being computed, the result is, bit for bit, that of the whole prompt.  Then the prompt length that must fit is prefix.length + S; a
        closed prefix or one of another weight set is a ValueError."""
        assert self.caches_are_enabled(), "backbone caches are not enabled"
        tokens = torch.as_tensor(tokens).to(device=self.device, dtype=torch.int32).contiguous()
        mask = torch.as_tensor(tokens_mask).to(device=self.device, dtype=torch.float32).contiguous()
        ncb = self.cfg["audio_num_codebooks"]
        if tokens.dim() != 2 or tokens.shape[1] != ncb + 1 or mask.shape != tokens.shape:
            raise ValueError(f"tokens / tokens_mask must be [S, {ncb + 1}]")
        S = int(tokens.shape[0])
        if not 0 <= int(row) < self.max_batch:
            raise ValueError(f"admit: row {row} out of range [0, {self.max_batch})")
        pad, P = self.row_state()
        if pad[int(row)] < int(self.cfg["max_seq_len"]):
            raise ValueError(f"admit: row {row} is live (park it first)")
        n = 0
        if prefix is not None:
            if not isinstance(prefix, Prefix) or not prefix._h:
                raise ValueError("admit: prefix must be an open Prefix (make_prefix)")
            n = prefix.length
        if S < 1 or n + S > P:
            raise ValueError(f"admit: a prompt of {n + S} frames does not fit below position {P} (shift by {n + S - P} first)")
        u = None
        if uniforms is not None:
            u = torch.as_tensor(uniforms).to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
            if u.numel() != ncb:
                raise ValueError(f"uniforms must hold {ncb} entries")
        sp = _lib.KKCsmSampler(float(temperature), int(top_k), 0.0, 0.0, 1, 0, 0)
        if sampler is not None:
            sp = _sampler_struct(sampler)
        if u is None and seed is not None:
            sp.seed, sp.use_device_rng = int(seed) & 0xFFFFFFFFFFFFFFFF, 1
        with torch.cuda.device(self.device):
            ws, need = self._admit_workspace(S)
            codes = torch.empty(ncb, dtype=torch.int32, device=self.device)
            if prefix is not None:
                rc = self.lib.kk_csm_admit_prefixed(self._h, self._stream(), int(row), prefix._h, S, C.c_void_p(tokens.data_ptr()),
                                                    C.c_void_p(mask.data_ptr()), C.byref(sp), C.c_void_p(u.data_ptr()) if u is not None else None,
                                                    int(stream_id) & 0x7FFFFFFF, C.c_void_p(ws.data_ptr()), need, C.c_void_p(codes.data_ptr()))
                if rc != 0 and b"another weight set" in (self.lib.kk_last_error() or b""):
                    raise ValueError("admit: the prefix was computed with another weight set")
                check(rc, "kk_csm_admit_prefixed")
                return codes
            check(self.lib.kk_csm_admit(self._h, self._stream(), int(row), S, C.c_void_p(tokens.data_ptr()), C.c_void_p(mask.data_ptr()), C.byref(sp),
                                        C.c_void_p(u.data_ptr()) if u is not None else None, int(stream_id) & 0x7FFFFFFF,
                                        C.c_void_p(ws.data_ptr()), need, C.c_void_p(codes.data_ptr())), "kk_csm_admit")
        return codes

    def admit_transfer(self, row: int, src: "SesameModel", src_row: int = 0, src_stream=None) -> None:
        """kk_csm_admit_transfer: the finished admission in live row `src_row` of `src` -- another generator on the same weights (`share()`),
        which ran `admit` on `src_stream` (a torch.cuda.Stream; None: the current one) -- enters the parked row `row` of this one: its window
        is copied below the position, in every layer's K and V, on the current stream.  One copy launch; the position, the other rows and the
        captured frame step are untouched.  The entry orders the two streams (this one waits for the admission, `src_stream` waits for the copy);
        `src_row` stays live: park it.  ValueError for what the library refuses on the host (the same generator, a row out of range, a live
        `row`, a parked `src_row`, a window longer than the position -- `shift` first --, other weights); nothing is changed then."""
        assert self.caches_are_enabled(), "backbone caches are not enabled"
        if not isinstance(src, SesameModel) or not src.caches_are_enabled():
            raise ValueError("admit_transfer: src must be a SesameModel with caches")
        with torch.cuda.device(self.device):
            sst = C.c_void_p((src_stream if src_stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)
            rc = self.lib.kk_csm_admit_transfer(self._h, self._stream(), int(row), src._h, sst, int(src_row))
        if rc != 0:
            raise ValueError((self.lib.kk_last_error() or b"kk_csm_admit_transfer failed").decode())

    def debug_logits(self) -> torch.Tensor:
        B, ncb, V = self._last_B, self.cfg["audio_num_codebooks"], self.cfg["audio_vocab_size"]
        out = torch.empty((ncb, B, V), dtype=torch.float32, device=self.device)
        check(self.lib.kk_csm_debug_logits(self._h, self._stream(), B, C.c_void_p(out.data_ptr())), "kk_csm_debug_logits")
        return out
