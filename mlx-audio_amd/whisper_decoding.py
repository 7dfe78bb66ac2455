"""Host mirror of the TEXT side of the reference's Whisper at token level: the decoder's weight table, the special-token ids, `DecodingOptions` /
`DecodingResult`, `detect_language` and the greedy `DecodingTask` of mlx_audio/stt/models/whisper/decoding.py:20-129, 398-742.  The arithmetic runs
in libkokoro_hip.so (kk_whisper_text_*, kk_op_whisper_*; the handle in csrc/kk_whisper_text.hip, its kernels in csrc/kk_whisper_text_kernels.hip): the decoder forward with its K/V caches, and ONE pick
launch per step that applies the logit filters, takes the arg-maximum and the log-probability and updates the rows' state on the device.  The host
looks at a device counter of unfinished rows every `eos_check_interval` steps.

There is no tokenizer here (the vocabulary files are not part of this repository): tokens go in and come out as ids, `DecodingResult.text` stays "".
`TextRuntime.forward_qk` is the forward that also hands out raw cross-attention scores; the token timestamps made from them live in whisper_timing.py.
`RowRuntime` is the handle's row mode (kk_whisper_text_rows_*): rows with their own window, position, options and lifetime, and groups of
rows on one window (beam search and best_of); the batcher on top of it lives in whisper_serve.py.  Sampling at temperature > 0, `best_of` and the temperature fallback live in whisper_sampling.py, on
`TextRuntime.set_audio_groups` / `sample_setup`; `decode` and `verify_options` here stay greedy and keep refusing a temperature.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace
from typing import Dict, Iterable, List, NamedTuple, Optional, Tuple, Union

import numpy as np

NOT_BUILT = "text decoder: not built"
CHUNK_LENGTH = 30
BLANK_TOKEN = 220  # " " in both the GPT-2 and the multilingual vocabulary (SuppressBlank, decoding.py:306)


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
def decoder_shapes(dims) -> Dict[str, tuple]:
    """name -> shape of every decoder parameter by the MLX checkpoint's names (whisper.py:202-224, 140-155, 90-97); the keys have no bias."""
    D, V = dims.n_text_state, dims.n_vocab
    s = {"decoder.token_embedding.weight": (V, D), "decoder.positional_embedding": (dims.n_text_ctx, D),
         "decoder.ln.weight": (D,), "decoder.ln.bias": (D,)}
    for i in range(dims.n_text_layer):
        p = f"decoder.blocks.{i}."
        for att in ("attn", "cross_attn"):
            for lin in ("query", "value", "out"):
                s[p + f"{att}.{lin}.weight"] = (D, D)
                s[p + f"{att}.{lin}.bias"] = (D,)
            s[p + f"{att}.key.weight"] = (D, D)
        s[p + "mlp1.weight"], s[p + "mlp1.bias"] = (4 * D, D), (4 * D,)
        s[p + "mlp2.weight"], s[p + "mlp2.bias"] = (D, 4 * D), (D,)
        for ln in ("attn_ln", "cross_attn_ln", "mlp_ln"):
            s[p + ln + ".weight"] = s[p + ln + ".bias"] = (D,)
    return s


def _as_f32(v) -> np.ndarray:
    if type(v).__module__.split(".")[0] == "torch":
        v = v.detach().float().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype=np.float32)


def decoder_tensors(dims, rest: dict, quantized: Optional[dict] = None) -> Optional[Dict[str, np.ndarray]]:
    """The complete decoder set of a checkpoint's non-encoder tensors as fp32 numpy, or None when a name of `decoder_shapes` is absent (an encoder-only
    checkpoint: the text side stays unbuilt).  With the complete set present, a misshapen tensor is a ValueError that names it.  `quantized`: matrices
    that arrive as (words, scales, biases, group_size, bits) instead (quant.split_triplets); they count as present, are checked and are left out."""
    quantized = quantized or {}
    want = decoder_shapes(dims)
    if any(k not in rest and k not in quantized for k in want):
        return None
    out = {}
    for k, shape in want.items():
        if k in quantized:
            words, scales, biases, group, bits = quantized[k]
            got = (words.shape[0], words.shape[-1] * (32 // bits)) if words.ndim == 2 else tuple(words.shape)
            if got != shape:
                raise ValueError(f"decoder tensor {k} has shape {got}, expected {shape}")
            if got[1] % group != 0 or scales.shape != (got[0], got[1] // group) or biases.shape != scales.shape:
                raise ValueError(f"decoder tensor {k}: scales / biases {tuple(scales.shape)} do not match {shape} at group size {group}")
            continue
        try:
            a = _as_f32(rest[k])
        except Exception as e:  # not an array at all
            raise ValueError(f"decoder tensor {k} is not a numeric array") from e
        if a.shape != shape:
            raise ValueError(f"decoder tensor {k} has shape {tuple(a.shape)}, expected {shape}")
        out[k] = a
    return out


def check_decoder_tensors(dims, tensors: dict) -> Dict[str, np.ndarray]:
    """Like decoder_tensors for a set that is MEANT to be complete: a missing name is a ValueError that names it too."""
    for k in decoder_shapes(dims):
        if k not in tensors:
            raise ValueError(f"missing decoder tensor: {k}")
    return decoder_tensors(dims, tensors)


# ---- tokens -------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SpecialTokens:
    """The ids tokenizer.py derives from the vocabulary, by arithmetic from n_vocab."""
    eot: int
    sot: int
    language_tokens: Tuple[int, ...]
    translate: int
    transcribe: int
    sot_lm: int
    sot_prev: int
    no_speech: int
    no_timestamps: int
    timestamp_begin: int
    multilingual: bool


def special_tokens(dims) -> SpecialTokens:
    multilingual = dims.n_vocab >= 51865
    num_languages = dims.n_vocab - 51765 - int(multilingual)
    base = 50257 if multilingual else 50256
    sot = base + 1
    t = sot + num_languages
    return SpecialTokens(eot=base, sot=sot, language_tokens=tuple(range(sot + 1, sot + 1 + num_languages)), translate=t + 1, transcribe=t + 2, sot_lm=t + 3,
                         sot_prev=t + 4, no_speech=t + 5, no_timestamps=t + 6, timestamp_begin=t + 7, multilingual=multilingual)


# ---- options ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class DecodingOptions:
    """decoding.py:82-116 with token ids where the reference takes text.  `language`: a language-token id, or an index into the language tokens, or None
    to detect.  `prompt` / `prefix`: lists of token ids.  `suppress_tokens`: an iterable of ids or "-1"; without a tokenizer "-1" cannot name the
    non-speech symbols of tokenizer.non_speech_tokens, so it contributes ONLY the special tokens of decoding.py:522-533 (transcribe, translate, sot,
    sot_prev, sot_lm, no_speech) -- pass the symbol ids yourself to suppress them."""
    task: str = "transcribe"
    language: Optional[int] = None
    temperature: float = 0.0
    sample_len: Optional[int] = None
    best_of: Optional[int] = None
    beam_size: Optional[int] = None
    patience: Optional[float] = None
    length_penalty: Optional[float] = None
    prompt: Optional[List[int]] = None
    prefix: Optional[List[int]] = None
    suppress_tokens: Optional[Union[str, Iterable[int]]] = "-1"
    suppress_blank: bool = True
    without_timestamps: bool = False
    max_initial_timestamp: Optional[float] = 1.0
    fp16: bool = True  # kept for the reference's signature; the decoder runs bf16 weights with fp32 activations whatever it says


@dataclass(frozen=True)
class DecodingResult:
    """decoding.py:119-129.  `language` is the language-token id (None for an English-only model), `language_probs` is keyed by language-token id,
    `text` stays "" and `compression_ratio` nan (no tokenizer)."""
    audio_features: object
    language: Optional[int]
    language_probs: Optional[Dict[int, float]] = None
    tokens: List[int] = field(default_factory=list)
    text: str = ""
    avg_logprob: float = np.nan
    no_speech_prob: float = np.nan
    temperature: float = np.nan
    compression_ratio: float = np.nan


def verify_options(options: DecodingOptions) -> DecodingOptions:
    """_verify_options (decoding.py:465-478) word for word, then what this build leaves out, each with its own message."""
    if options.beam_size is not None and options.best_of is not None:
        raise ValueError("beam_size and best_of can't be given together")
    if options.temperature == 0:
        if options.best_of is not None:
            raise ValueError("best_of with greedy sampling (T=0) is not compatible")
    if options.patience is not None and options.beam_size is None:
        raise ValueError("patience requires beam_size to be given")
    if options.length_penalty is not None and not (0 <= options.length_penalty <= 1):
        raise ValueError("length_penalty (alpha) should be a value between 0 and 1")
    if options.patience is not None:
        raise NotImplementedError("patience belongs to beam search, which is not yet implemented")
    if options.beam_size is not None:
        raise NotImplementedError("Beam search decoder is not yet implemented")
    if options.best_of is not None:
        raise NotImplementedError("best_of needs sampling at temperature > 0, which is not yet implemented")
    if options.temperature != 0:
        raise NotImplementedError("sampling at temperature > 0 is not yet implemented (greedy decoding only)")
    for name in ("prompt", "prefix"):
        v = getattr(options, name)
        if isinstance(v, str):
            raise ValueError(f"{name} must be a list of token ids: the tokenizer is not built")
    if isinstance(options.language, str):
        raise ValueError("language must be a language-token id or index: the tokenizer is not built")
    if options.task not in ("transcribe", "translate", "lang_id"):
        raise ValueError(f"unknown task {options.task!r}")
    return options


def language_token(tok: SpecialTokens, language: int) -> int:
    n = len(tok.language_tokens)
    if 0 <= language < n:
        return tok.language_tokens[language]
    if n and tok.language_tokens[0] <= language <= tok.language_tokens[-1]:
        return int(language)
    raise ValueError(f"language {language} is neither an index below {n} nor a language-token id")


def sot_sequence(tok: SpecialTokens, language: Optional[int], task: str, without_timestamps: bool) -> Tuple[int, ...]:
    """tokenizer.py's sot_sequence: sot, then language and task for a multilingual vocabulary; `language` None stands for the first language
    (the reference builds its tokenizer with "en") until detection overwrites it."""
    seq = [tok.sot]
    if tok.multilingual:
        seq.append(language_token(tok, 0 if language is None else language))
        seq.append(tok.translate if task == "translate" else tok.transcribe)
    if without_timestamps:
        seq.append(tok.no_timestamps)
    return tuple(seq)


def initial_tokens(tok: SpecialTokens, options: DecodingOptions, n_ctx: int, sample_len: int) -> Tuple[int, ...]:
    """_get_initial_tokens (decoding.py:480-506)"""
    tokens = list(sot_sequence(tok, options.language, options.task, options.without_timestamps))
    if options.prefix:
        prefix = list(options.prefix)
        max_prefix_len = n_ctx // 2 - sample_len
        prefix = prefix[-max_prefix_len:]
        tokens = tokens + prefix
    if options.prompt:
        tokens = [tok.sot_prev] + list(options.prompt)[-(n_ctx // 2 - 1):] + tokens
    return tuple(int(t) for t in tokens)


def suppress_list(tok: SpecialTokens, options: DecodingOptions) -> Tuple[int, ...]:
    """_get_suppress_tokens (decoding.py:508-535) without tokenizer.non_speech_tokens, see DecodingOptions"""
    st = options.suppress_tokens
    if isinstance(st, str):
        st = [int(t) for t in st.split(",")] if st else []
    st = list(st) if st is not None else []
    st = [int(t) for t in st if int(t) >= 0]
    st += [tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm, tok.no_speech]
    return tuple(sorted(set(st)))


def suppress_bitmask(n_vocab: int, ids: Iterable[int]) -> np.ndarray:
    bits = np.zeros((n_vocab + 31) // 32, np.uint32)
    for t in ids:
        if not 0 <= t < n_vocab:
            raise ValueError(f"suppress token {t} is outside the vocabulary")
        bits[t >> 5] |= np.uint32(1 << (t & 31))
    return bits


# ---- the runtime behind Model -----------------------------------------------------------------------------------------------------------------
class TextRuntime:
    """The text handle of one Model plus the PyTorch memory it runs in."""

    def __init__(self, lib, dims, tensors: Dict[str, np.ndarray], device, stream, quantized: Optional[dict] = None):
        from . import _lib

        self._lib, self.dims, self.device = lib, dims, device
        kc = _lib.KKWhisperTextConfig()
        for k in ("n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer", "n_audio_ctx", "n_audio_state"):
            setattr(kc, k, int(getattr(dims, k)))
        h = C.c_void_p()
        _lib.check(lib.kk_whisper_text_create(C.byref(kc), C.byref(h)), "kk_whisper_text_create")
        self._h = h
        try:
            for name, a in tensors.items():
                shp = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(lib.kk_whisper_text_load_tensor(h, name.encode(), shp, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_whisper_text_load_tensor")
            for name, (words, scales, biases, group, bits) in (quantized or {}).items():
                if name in decoder_shapes(dims):  # (checked by decoder_tensors)
                    shp = (C.c_int64 * 2)(words.shape[0], words.shape[1] * (32 // bits))
                    _lib.check(lib.kk_whisper_text_load_quantized(h, name.encode(), shp, words.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p),
                                                                  biases.ctypes.data_as(C.c_void_p), group, bits), "kk_whisper_text_load_quantized")
            _lib.check(lib.kk_whisper_text_finalize(h, stream), "kk_whisper_text_finalize")
        except Exception:
            self.release()
            raise
        self._state = self._ws = self._step_logits = None
        self.B = 0

    def release(self):
        if getattr(self, "_h", None) is not None:
            self._lib.kk_whisper_text_destroy(self._h)
        self._h = None

    def weight_report(self) -> dict:
        """kk_whisper_text_weight_info / _fallback, see whisper.Model.weight_report"""
        from . import _lib

        mb, tb = C.c_size_t(), C.c_size_t()
        n_packed, n_bf16, n_fb = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.kk_whisper_text_weight_info(self._h, C.byref(mb), C.byref(tb), C.byref(n_packed), C.byref(n_bf16), C.byref(n_fb)),
                   "kk_whisper_text_weight_info")
        fallbacks = dict((self._lib.kk_whisper_text_weight_fallback(self._h, i) or b"\t").decode().split("\t", 1) for i in range(n_fb.value))
        return {"matrix_bytes": mb.value, "resident_bytes": tb.value, "packed": n_packed.value, "bf16": n_bf16.value, "fallbacks": fallbacks}

    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, B, S):
        import torch

        need = int(self._lib.kk_whisper_text_workspace_bytes(self._h, B, S))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._ws.data_ptr()), self._ws.numel()

    def set_audio(self, features):
        """features: fp32 device (B, n_audio_ctx, n_audio_state), contiguous"""
        import torch

        from . import _lib

        B = features.shape[0]
        need = int(self._lib.kk_whisper_text_state_bytes(self._h, B))
        if self._state is None or self._state.numel() < need:
            self._state = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws, wsn = self._workspace(B, 1)
        _lib.check(self._lib.kk_whisper_text_set_audio(self._h, self._stream(), B, C.c_void_p(features.data_ptr()), C.c_void_p(self._state.data_ptr()),
                                                       self._state.numel(), ws, wsn), "kk_whisper_text_set_audio")
        self.B = B

    def set_audio_groups(self, features, n_group: int):
        """features: fp32 device (n_audio, n_audio_ctx, n_audio_state), contiguous.  B = n_audio * n_group rows, row b on the cross K/V of window
        b // n_group, which is projected and kept once per window."""
        import torch

        from . import _lib

        n_audio = features.shape[0]
        B = n_audio * n_group
        need = int(self._lib.kk_whisper_text_state_bytes_groups(self._h, n_audio, n_group))
        if need == 0:
            raise ValueError(f"n_group must be in 1 .. {_lib.WHISPER_MAX_GROUP}")
        if self._state is None or self._state.numel() < need:
            self._state = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws, wsn = self._workspace(B, 1)
        _lib.check(self._lib.kk_whisper_text_set_audio_groups(self._h, self._stream(), n_audio, n_group, C.c_void_p(features.data_ptr()),
                                                              C.c_void_p(self._state.data_ptr()), self._state.numel(), ws, wsn), "kk_whisper_text_set_audio_groups")
        self.B = B

    def sample_setup(self, temperature: float, seed: int, streams):
        """after pick_setup: the picks draw at `temperature` on the Philox key `seed`, row b on stream id streams[b], until the next pick_setup"""
        from . import _lib

        ids = np.ascontiguousarray(np.asarray(streams, np.uint32))
        if ids.shape != (self.B,):
            raise ValueError(f"streams must hold one id per row ({self.B})")
        _lib.check(self._lib.kk_whisper_text_sample_setup(self._h, self._stream(), float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, ids.ctypes.data_as(C.c_void_p)),
                   "kk_whisper_text_sample_setup")

    def beam_setup(self, beam_size: int, max_candidates: int):
        """after set_audio_groups(features, beam_size) and pick_setup: `pick` runs the beam's top-k and select, `step` reads the self K/V through the
        owner table, until the next pick_setup.  The beam state lives in memory of its own beside the window state."""
        import torch

        from . import _lib

        n_audio = self.B // beam_size
        need = int(self._lib.kk_whisper_text_beam_state_bytes(self._h, n_audio, beam_size, max_candidates))
        if need == 0:
            raise ValueError(f"beam_size must be in 1 .. {_lib.WHISPER_MAX_GROUP} and max_candidates in 1 .. {2 * _lib.WHISPER_MAX_GROUP}")
        if getattr(self, "_beam_state", None) is None or self._beam_state.numel() < need:
            self._beam_state = torch.empty(need, dtype=torch.uint8, device=self.device)
        _lib.check(self._lib.kk_whisper_text_beam_setup(self._h, self._stream(), beam_size, max_candidates, C.c_void_p(self._beam_state.data_ptr()),
                                                        self._beam_state.numel()), "kk_whisper_text_beam_setup")
        self._beam = (n_audio, beam_size, max_candidates)

    def beam_not_complete(self) -> int:
        from . import _lib

        n = C.c_int32()
        _lib.check(self._lib.kk_whisper_text_beam_not_complete(self._h, self._stream(), C.byref(n)), "kk_whisper_text_beam_not_complete")
        return int(n.value)

    def beam_read(self):
        """-> per window its finished sequences [(tokens, sum_logprob)] in the order they finished, and its live prefixes [(tokens, sum_logprob)] by slot
        (a dead slot's sum is -inf)"""
        from . import _lib

        n_audio, K, mc = self._beam
        cap = self.dims.n_text_ctx
        fc, fs, fl = np.zeros(n_audio, np.int32), np.zeros((n_audio, mc), np.float32), np.zeros((n_audio, mc), np.int32)
        ft, lt = np.zeros((n_audio, mc, cap), np.int32), np.zeros((self.B, cap), np.int32)
        ls, ll = np.zeros(self.B, np.float32), np.zeros(self.B, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _lib.check(self._lib.kk_whisper_text_beam_read(self._h, self._stream(), cap, p(fc), p(fs), p(fl), p(ft), p(lt), p(ls), p(ll)), "kk_whisper_text_beam_read")
        finished = [[([int(t) for t in ft[a, f, : fl[a, f]]], float(fs[a, f])) for f in range(fc[a])] for a in range(n_audio)]
        live = [[([int(t) for t in lt[a * K + k, : ll[a * K + k]]], float(ls[a * K + k])) for k in range(K)] for a in range(n_audio)]
        return finished, live

    def rewind(self, position: int = 0):
        from . import _lib

        _lib.check(self._lib.kk_whisper_text_rewind(self._h, position), "kk_whisper_text_rewind")

    def forward(self, tokens, all_positions: bool):
        """tokens: int32 device (B, S) -> fp32 (B, S, V) or (B, V)"""
        import torch

        from . import _lib

        B, S = tokens.shape
        V = self.dims.n_vocab
        out = torch.empty((B, S, V) if all_positions else (B, V), dtype=torch.float32, device=self.device)
        ws, wsn = self._workspace(B, S)
        _lib.check(self._lib.kk_whisper_text_forward(self._h, self._stream(), B, S, C.c_void_p(tokens.data_ptr()), C.c_void_p(out.data_ptr()), int(all_positions),
                                                     ws, wsn), "kk_whisper_text_forward")
        self._last = out  # the pick that follows reads it
        return out

    def forward_qk(self, tokens, pairs, n_keys: int):
        """the capturing forward: tokens int32 device (B, S), pairs an int array (n, 2) of (layer, head) -> (logits fp32 (B, S, V), the raw cross-attention
        scores 64^-0.5 q k of the pairs, fp32 (B, n, S, n_keys)); the logits are the bits of forward(tokens, True)"""
        import torch

        from . import _lib

        B, S = tokens.shape
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        n = int(pairs.shape[0])
        out = torch.empty((B, S, self.dims.n_vocab), dtype=torch.float32, device=self.device)
        qk = torch.empty((B, n, S, n_keys), dtype=torch.float32, device=self.device)
        ws, wsn = self._workspace(B, S)
        _lib.check(self._lib.kk_whisper_text_forward_qk(self._h, self._stream(), B, S, C.c_void_p(tokens.data_ptr()), C.c_void_p(out.data_ptr()),
                                                        pairs.ctypes.data_as(C.c_void_p), n, int(n_keys), C.c_void_p(qk.data_ptr()), qk.numel() * 4, ws, wsn),
                   "kk_whisper_text_forward_qk")
        self._last = out
        return out, qk

    def step(self):
        """one position on the tokens the last pick chose; the logits stay in a buffer the runtime keeps"""
        import torch

        from . import _lib

        if self._step_logits is None or self._step_logits.shape[0] != self.B:
            self._step_logits = torch.empty((self.B, self.dims.n_vocab), dtype=torch.float32, device=self.device)
        ws, wsn = self._workspace(self.B, 1)
        _lib.check(self._lib.kk_whisper_text_forward(self._h, self._stream(), self.B, 1, None, C.c_void_p(self._step_logits.data_ptr()), 0, ws, wsn),
                   "kk_whisper_text_forward")

    def pick_setup(self, params, suppress_bits: Optional[np.ndarray]):
        from . import _lib

        sp = None if suppress_bits is None else suppress_bits.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.kk_whisper_text_pick_setup(self._h, self._stream(), C.byref(params), sp), "kk_whisper_text_pick_setup")

    def pick(self):
        from . import _lib

        _lib.check(self._lib.kk_whisper_text_pick(self._h, self._stream()), "kk_whisper_text_pick")

    def not_ended(self) -> int:
        from . import _lib

        n = C.c_int32()
        _lib.check(self._lib.kk_whisper_text_not_ended(self._h, self._stream(), C.byref(n)), "kk_whisper_text_not_ended")
        return int(n.value)

    def read(self):
        """-> (tokens int32 [B][n_text_ctx], list of pick states)"""
        from . import _lib

        cap = self.dims.n_text_ctx
        toks = np.zeros((self.B, cap), np.int32)
        rows = (_lib.KKWhisperPickState * self.B)()
        _lib.check(self._lib.kk_whisper_text_read(self._h, self._stream(), toks.ctypes.data_as(C.c_void_p), cap, C.cast(rows, C.c_void_p)), "kk_whisper_text_read")
        return toks, list(rows)


# ---- detect_language / decode (called by whisper.Model) -------------------------------------------------------------------------------------
def _features(model, x):
    """mel (.., 2 n_audio_ctx, n_mels) or features (.., n_audio_ctx, n_audio_state) -> fp32 device (B, n_audio_ctx, n_audio_state), was it 2-D"""
    import torch

    d = model.dims
    shape = tuple(x.shape)
    if len(shape) not in (2, 3):
        raise ValueError("expected a 2-D or 3-D mel spectrogram or audio features")
    single = len(shape) == 2
    if shape[-2:] != (d.n_audio_ctx, d.n_audio_state):  # (decoding.py:52, 541) already-encoded features skip the encoder
        x = model.embed_audio(x)
    x = torch.as_tensor(x).to(device=model.device, dtype=torch.float32)
    if single:
        x = x[None]
    return x.contiguous(), single


def detect_language(model, mel_or_features):
    """decoding.py:20-79 -> (language-token ids: an int, or an int64 device tensor (B,); probabilities: {language-token id: p}, or a list of them)"""
    import torch

    rt = model._text
    tok = special_tokens(model.dims)
    if not tok.multilingual:
        raise ValueError("This model doesn't have language tokens so it can't perform lang id")
    feats, single = _features(model, mel_or_features)
    with torch.cuda.device(model.device):
        rt.set_audio(feats)
        x = torch.full((feats.shape[0], 1), tok.sot, dtype=torch.int32, device=model.device)
        logits = rt.forward(x, True)[:, 0]
        lo, hi = tok.language_tokens[0], tok.language_tokens[-1] + 1
        lang = logits[:, lo:hi]  # everything but the language tokens is masked: the softmax runs over them alone
        ids = lang.argmax(dim=-1) + lo
        probs = torch.softmax(lang, dim=-1).cpu().numpy()
    out = [{t: float(probs[i, t - lo]) for t in tok.language_tokens} for i in range(feats.shape[0])]
    if single:
        return int(ids[0]), out[0]
    return ids, out


class Windows(NamedTuple):
    """what DecodingTask.run knows of a batch of windows before its loop (`window_prologue`)"""
    tokens: np.ndarray  # int32 (rows, S): every row's initial tokens, the detected language written in
    sample_len: int
    sample_begin: int
    sot_index: int
    feats: object       # fp32 device (n_audio, n_audio_ctx, n_audio_state)
    single: bool        # the input was 2-D
    languages: List[Optional[int]]
    lang_probs: List[Optional[Dict[int, float]]]  # per window; None where nothing was detected


def window_prologue(model, mel_or_features, options: DecodingOptions, n_group: int = 1) -> Windows:
    """DecodingTask.run up to its loop, behind the caller's option checks, for `n_group` decoder rows per window: the initial tokens (decoding.py:480-506),
    the room check, the features, and _detect_language (:557-570) written into the tokens of every row of its window."""
    d = model.dims
    tok = special_tokens(d)
    n_ctx = d.n_text_ctx
    sample_len = options.sample_len or n_ctx // 2
    init = initial_tokens(tok, options, n_ctx, sample_len)
    sample_begin, sot_index = len(init), init.index(tok.sot)
    if sample_begin >= n_ctx:
        raise ValueError(f"{sample_begin} initial tokens leave no room in n_text_ctx = {n_ctx}")
    feats, single = _features(model, mel_or_features)
    n_audio = feats.shape[0]
    tokens = np.tile(np.asarray(init, np.int32), (n_audio * n_group, 1))
    languages: List[Optional[int]] = [None if not tok.multilingual else init[sot_index + 1]] * n_audio
    lang_probs: List[Optional[Dict[int, float]]] = [None] * n_audio
    if options.language is None or options.task == "lang_id":
        ids, lang_probs = detect_language(model, feats)
        languages = [max(p, key=p.get) for p in lang_probs]
        if options.language is None:
            tokens[:, sot_index + 1] = np.repeat(ids.cpu().numpy(), n_group)
    return Windows(tokens, sample_len, sample_begin, sot_index, feats, single, languages, lang_probs)


def window_loop(model, w: Windows, options: DecodingOptions, n_group: int, eos_check_interval: int, setup, done, audio_is_set: bool = False):
    """The main loop of DecodingTask.run (:590-616, 641-669) on `n_group` rows per window: pick_setup and, behind it, the caller's `setup()` (None: greedy
    picks); the prefill; then step and pick until `done()` -- asked every eos_check_interval steps --, sample_len or the text context ends it.  Called with
    the model's device current.  audio_is_set: the windows' cross K/V is the state's already.  -> no_speech_prob per window, on the device"""
    import torch

    d, rt = model.dims, model._text
    tok = special_tokens(d)
    params, bits = pick_params(d, tok, options)
    if audio_is_set:
        rt.rewind(0)
    else:
        rt.set_audio_groups(w.feats, n_group)
    rt.pick_setup(params, bits)
    if setup is not None:
        setup()
    pre = rt.forward(torch.from_numpy(w.tokens).to(model.device), True)  # the prefill, (B, S, V)
    no_speech = torch.softmax(pre[::n_group, w.sot_index], dim=-1)[:, tok.no_speech]  # the rows of a window share their prefill
    rt.pick()
    for i in range(1, w.sample_len):
        if w.sample_begin + i > d.n_text_ctx:  # (:604)
            break
        rt.step()
        rt.pick()
        if i % eos_check_interval == 0 and done():
            break
    return no_speech


def cut_at_eot(tokens, eot: int) -> List[int]:
    seq = [int(t) for t in tokens]
    return seq[: seq.index(eot)] if eot in seq else seq


def decode(model, mel_or_features, options: DecodingOptions = DecodingOptions(), eos_check_interval: int = 8, **kwargs):
    """decoding.py:710-742 -> DecodingTask.run (:618-707), greedy at temperature 0"""
    import torch

    if kwargs:
        options = replace(options, **kwargs)
    options = verify_options(options)
    if eos_check_interval < 1:
        raise ValueError("eos_check_interval must be >= 1")
    rt = model._text
    w = window_prologue(model, mel_or_features, options)
    B = w.feats.shape[0]
    if options.task == "lang_id":
        res = [DecodingResult(audio_features=w.feats[b], language=w.languages[b], language_probs=w.lang_probs[b]) for b in range(B)]
        return res[0] if w.single else res
    with torch.cuda.device(model.device):
        # (detection has made these windows' cross K/V already)
        no_speech = window_loop(model, w, options, 1, eos_check_interval, None, lambda: rt.not_ended() == 0, audio_is_set=options.language is None)
        toks, rows = rt.read()
        no_speech = no_speech.cpu().numpy()
    eot = special_tokens(model.dims).eot
    out = []
    for b in range(B):
        seq = cut_at_eot(toks[b, : rows[b].count], eot)
        out.append(DecodingResult(audio_features=w.feats[b], language=w.languages[b], tokens=seq,
                                  avg_logprob=float(rows[b].sum_logprob) / (len(seq) + 1), no_speech_prob=float(no_speech[b]), temperature=options.temperature))
    return out[0] if w.single else out


# ---- row mode: decoder rows that join and leave one running batch (kk_whisper_text_rows_*) ------------------------------------------
def pick_params(dims, tok: SpecialTokens, options: DecodingOptions):
    """-> (kk_whisper_pick_params, suppress bitmask or None) of `options`, as decode sets them up"""
    from . import _lib

    params = _lib.KKWhisperPickParams(n_vocab=dims.n_vocab, eot=tok.eot, blank=BLANK_TOKEN, no_timestamps=tok.no_timestamps, timestamp_begin=tok.timestamp_begin,
                                      max_initial_timestamp_index=-1, without_timestamps=int(options.without_timestamps), suppress_blank=int(options.suppress_blank))
    if not options.without_timestamps and options.max_initial_timestamp:
        precision = CHUNK_LENGTH / dims.n_audio_ctx  # usually 0.02 seconds
        params.max_initial_timestamp_index = round(options.max_initial_timestamp / precision)
    bits = suppress_bitmask(dims.n_vocab, suppress_list(tok, options)) if options.suppress_tokens else None
    return params, bits


class RowRuntime:
    """Row mode of a TextRuntime's handle: thin ctypes plumbing over kk_whisper_text_rows_* that owns the PyTorch memory (the row state, a workspace
    that grows with the largest round, the last round's logits).  The window state of the TextRuntime is not touched."""

    def __init__(self, text: TextRuntime, max_rows: int):
        import torch

        from . import _lib

        if not 1 <= max_rows <= _lib.WHISPER_MAX_ROWS:
            raise ValueError(f"max_rows must be in 1 .. {_lib.WHISPER_MAX_ROWS}")
        self._t, self._lib, self.dims, self.device, self.max_rows = text, text._lib, text.dims, text.device, max_rows
        self._h = text._h
        with torch.cuda.device(self.device):
            need = int(self._lib.kk_whisper_text_rows_state_bytes(self._h, max_rows))
            self._state = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws = None
            _lib.check(self._lib.kk_whisper_text_rows_open(self._h, self._stream(), max_rows, C.c_void_p(self._state.data_ptr()), need),
                       "kk_whisper_text_rows_open")
            need = int(self._lib.kk_whisper_text_rows_groups_state_bytes(self._h, max_rows))  # what groups keep beside the row state
            self._gstate = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.check(self._lib.kk_whisper_text_rows_groups_bind(self._h, self._stream(), C.c_void_p(self._gstate.data_ptr()), need), "kk_whisper_text_rows_groups_bind")
        self._logits = None

    def _stream(self):
        return self._t._stream()

    def _workspace(self, R: int, n_items: int):
        import torch

        need = int(self._lib.kk_whisper_text_rows_workspace_bytes(self._h, R, n_items))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._ws.data_ptr()), self._ws.numel()

    def _admission(self, features, tokens, params, suppress_bits: Optional[np.ndarray]):
        """what both admission entries take of a window -- features: fp32 device (n_audio_ctx, n_audio_state), contiguous; tokens: the initial ids --
        and, behind it, the workspace"""
        toks = np.ascontiguousarray(np.asarray(tokens, np.int32))
        sp = None if suppress_bits is None else suppress_bits.ctypes.data_as(C.c_void_p)
        return (C.c_void_p(features.data_ptr()), toks.ctypes.data_as(C.c_void_p), len(toks), C.byref(params), sp), self._workspace(1, 1)

    def admit_group(self, rows, beam: bool, features, tokens, params, suppress_bits: Optional[np.ndarray], max_candidates: int = 1):
        """rows: the group's decoder rows, the leader first, on ONE projection of the window's cross K/V; beam: a beam group of len(rows) =
        beam_size, else a plain one (every row picks for itself; a single row is the plain group of one).  Read with group_read, left with group_release."""
        from . import _lib

        r = np.ascontiguousarray(np.asarray(rows, np.int32))
        window, ws = self._admission(features, tokens, params, suppress_bits)
        _lib.check(self._lib.kk_whisper_text_rows_admit_group(self._h, self._stream(), r.ctypes.data_as(C.c_void_p), len(r),
                                                              _lib.WHISPER_GROUP_BEAM if beam else _lib.WHISPER_GROUP_PLAIN, *window, int(max_candidates), *ws),
                   "kk_whisper_text_rows_admit_group")

    def admit(self, row: int, features, tokens, params, suppress_bits: Optional[np.ndarray]):
        """the one-row form on the raw entry: the row is in no group, is read with `read` and is admitted over without a release"""
        from . import _lib

        window, ws = self._admission(features, tokens, params, suppress_bits)
        _lib.check(self._lib.kk_whisper_text_rows_admit(self._h, self._stream(), row, *window, *ws), "kk_whisper_text_rows_admit")

    def set_draw(self, row: int, temperature: float, seed: int, stream: int):
        """after admit (which leaves the row greedy): the row's picks draw at `temperature` on the Philox key `seed` and the stream id `stream`"""
        from . import _lib

        _lib.check(self._lib.kk_whisper_text_rows_set_draw(self._h, self._stream(), row, float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF),
                   "kk_whisper_text_rows_set_draw")

    def forward(self, items, out_rows):
        """items: (row, pos, count, from, keep, slot) tuples; out_rows: flat rows -> fp32 device (len(out_rows), V), alive until the next forward"""
        import torch

        from . import _lib

        n = len(items)
        arr = (_lib.KKWhisperRowsItem * max(n, 1))(*[_lib.KKWhisperRowsItem(*it) for it in items])
        out = np.ascontiguousarray(np.asarray(out_rows, np.int32))
        R = sum(max(int(it[2]), 0) for it in items)
        logits = torch.empty((max(len(out), 1), self.dims.n_vocab), dtype=torch.float32, device=self.device)
        ws, wsn = self._workspace(max(R, 1), max(min(n, _lib.WHISPER_MAX_ROWS), 1))
        _lib.check(self._lib.kk_whisper_text_rows_forward(self._h, self._stream(), C.cast(arr, C.c_void_p), n, out.ctypes.data_as(C.c_void_p), len(out),
                                                          C.c_void_p(logits.data_ptr()), ws, wsn), "kk_whisper_text_rows_forward")
        self._logits = logits  # the pick that follows reads it
        return logits

    def pick(self, rows):
        from . import _lib

        r = np.ascontiguousarray(np.asarray(rows, np.int32))
        _lib.check(self._lib.kk_whisper_text_rows_pick(self._h, self._stream(), r.ctypes.data_as(C.c_void_p), len(r)), "kk_whisper_text_rows_pick")

    def flags(self) -> List[bool]:
        from . import _lib

        out = np.zeros(self.max_rows, np.int32)
        _lib.check(self._lib.kk_whisper_text_rows_flags(self._h, self._stream(), out.ctypes.data_as(C.c_void_p)), "kk_whisper_text_rows_flags")
        return [bool(v) for v in out]

    def read(self, row: int, kept: bool = True):
        """-> (sampled tokens int32 [n_text_ctx], pick state, the two kept logits rows fp32 device (2, V) or None)"""
        import torch

        from . import _lib

        cap = self.dims.n_text_ctx
        toks = np.zeros(cap, np.int32)
        st = _lib.KKWhisperPickState()
        k = torch.empty((2, self.dims.n_vocab), dtype=torch.float32, device=self.device) if kept else None
        _lib.check(self._lib.kk_whisper_text_rows_read(self._h, self._stream(), row, toks.ctypes.data_as(C.c_void_p), cap, C.byref(st),
                                                       None if k is None else C.c_void_p(k.data_ptr())), "kk_whisper_text_rows_read")
        return toks, st, k

    def set_token(self, row: int, index: int, token):
        """token: an int32 device tensor of one element"""
        from . import _lib

        _lib.check(self._lib.kk_whisper_text_rows_set_token(self._h, self._stream(), row, index, C.c_void_p(token.data_ptr())), "kk_whisper_text_rows_set_token")

    def group_read(self, leader: int, n_rows: int, kept: bool = True):
        """-> (finished [(tokens, sum)] in the order they finished, live [(tokens, sum)] by slot -- TextRuntime.beam_read for one window -- and the
        leader's two kept logits rows fp32 device (2, V) or None)"""
        import torch

        from . import _lib

        cap, F = self.dims.n_text_ctx, 2 * _lib.WHISPER_MAX_GROUP
        fc, fs, fl = np.zeros(1, np.int32), np.zeros(F, np.float32), np.zeros(F, np.int32)
        ft, lt = np.zeros((F, cap), np.int32), np.zeros((n_rows, cap), np.int32)
        ls, ll = np.zeros(n_rows, np.float32), np.zeros(n_rows, np.int32)
        k = torch.empty((2, self.dims.n_vocab), dtype=torch.float32, device=self.device) if kept else None
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _lib.check(self._lib.kk_whisper_text_rows_group_read(self._h, self._stream(), leader, cap, p(fc), p(fs), p(fl), p(ft), p(lt), p(ls), p(ll),
                                                             None if k is None else C.c_void_p(k.data_ptr())), "kk_whisper_text_rows_group_read")
        finished = [([int(t) for t in ft[f, : fl[f]]], float(fs[f])) for f in range(fc[0])]
        live = [([int(t) for t in lt[g, : ll[g]]], float(ls[g])) for g in range(n_rows)]
        return finished, live, k

    def group_release(self, leader: int):
        from . import _lib

        _lib.check(self._lib.kk_whisper_text_rows_group_release(self._h, leader), "kk_whisper_text_rows_group_release")
