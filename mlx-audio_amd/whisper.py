"""Host mirror of the reference's Whisper (mlx_audio/stt/models/whisper): the constants, `pad_or_trim` and `log_mel_spectrogram` of
audio.py:12-82, `ModelDimensions`, and `Model` with `embed_audio` / `load_weights` / `from_pretrained` (whisper.py:67-78, 251-353) and, at token
level, `logits`, `detect_language` and `decode` (whisper.py:298, decoding.py; the options, results and special tokens live in whisper_decoding.py
and are re-exported here).  The arithmetic runs in libkokoro_hip.so (kk_op_log_mel, kk_whisper_*, csrc/kk_whisper.hip; kk_whisper_text_*,
kk_op_whisper_*, csrc/kk_whisper_text.hip with the kernels of csrc/kk_whisper_text_kernels.hip); PyTorch allocates device memory and provides the stream.

The text side is built when a checkpoint holds the COMPLETE `decoder.*` set; otherwise the model is encoder-only and `logits`, `decode`,
`detect_language`, `forward_with_cross_qk` and the alignment heads raise NotImplementedError("text decoder: not built").  `generate` keeps raising;
transcription of long audio is `Model.transcribe` (whisper_transcribe.py), with `mel_windows` here cutting a round's windows on the device.
`Model.decoder_weights` keeps the non-encoder tensors of a checkpoint on the host, untouched, either way -- an `alignment_heads` entry included: the heads are set with `set_alignment_heads`, never parsed from a checkpoint.

Token timestamps (`Model.alignment_heads`, `set_alignment_heads`, `forward_with_cross_qk`, whisper.py:272-303; `find_alignment`, `dtw`, `median_filter`,
`TokenTiming`, `WordTiming` of whisper_timing.py, re-exported here) run on kk_op_whisper_qk_rows / align_matrix / dtw and kk_whisper_text_forward_qk
(csrc/kk_whisper_align.hip).

`span_windows(spans, W, n_mels, src_rate)` (kk_op_log_mel_spans) turns spans of sample buffers at another rate -- flat, or rings at 64-bit stream
positions -- into windows in one launch pair, bit-equal to `resample`, `log_mel_spectrogram` and `mel_windows` in turn: how a CSM listener's utterance gets here.

`Model.serve(...)` returns a `whisper_serve.WhisperBatcher`: windows with their own options join and leave one running decoder batch (the row mode of the
text handle, kk_whisper_text_rows_*), each with the result `decode` gives it alone."""
from __future__ import annotations

import base64
import ctypes as C
import gzip
import json
import math
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Dict, NamedTuple, Optional

import numpy as np

# hard-coded audio hyper-parameters (audio.py:12-21)
SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE  # 480000 samples in a 30-second chunk
N_FRAMES = N_SAMPLES // HOP_LENGTH  # 3000 frames in a mel spectrogram input
N_SAMPLES_PER_TOKEN = HOP_LENGTH * 2  # the stem's second convolution has stride 2
FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH  # 10 ms per audio frame
TOKENS_PER_SECOND = SAMPLE_RATE // N_SAMPLES_PER_TOKEN  # 20 ms per audio token

from .whisper_decoding import (NOT_BUILT as _NOT_BUILT, DecodingOptions, DecodingResult, SpecialTokens, decoder_shapes,  # noqa: E402,F401
                               decoder_tensors, special_tokens)
from .whisper_timing import TokenTiming, WordTiming, dtw, find_alignment, median_filter  # noqa: E402,F401


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def pad_or_trim(array, length: int = N_SAMPLES, *, axis: int = -1):
    """audio.py:24-38: cut `axis` at `length`, or append zeros up to it.  numpy arrays and torch tensors (any device) keep their kind."""
    n = array.shape[axis]
    if n > length:
        sl = [slice(None)] * array.ndim
        sl[axis] = slice(0, length)
        array = array[tuple(sl)]
    elif n < length:
        ax = axis % array.ndim
        if _is_torch(array):
            import torch

            shape = list(array.shape)
            shape[ax] = length - n
            array = torch.cat([array, torch.zeros(shape, dtype=array.dtype, device=array.device)], dim=ax)
        else:
            widths = [(0, 0)] * array.ndim
            widths[ax] = (0, length - n)
            array = np.pad(array, widths)
    return array


def _hz_to_mel(f: float) -> float:
    """Slaney's scale: linear (200/3 Hz per mel) below 1 kHz, logarithmic (27 mels per factor 6.4) above."""
    return 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4) if f >= 1000.0 else 3.0 * f / 200.0


def mel_filters(n_mels: int) -> np.ndarray:
    """The (n_mels, 201) float64 filter bank the reference builds with mel_filters(16000, 400, n_mels, norm="slaney", mel_scale=None)
    (audio.py:76; mlx_audio/utils.py:165-237, where a mel_scale other than "htk" takes the Slaney branch): triangles between n_mels + 2
    points equally spaced on Slaney's scale from 0 to 8 kHz, each scaled by 2 / (its width in Hz)."""
    freqs = np.linspace(0.0, SAMPLE_RATE // 2, N_FFT // 2 + 1)
    mels = np.linspace(_hz_to_mel(0.0), _hz_to_mel(SAMPLE_RATE / 2), n_mels + 2)
    pts = np.where(mels >= 15.0, 1000.0 * np.exp(math.log(6.4) / 27.0 * (mels - 15.0)), 200.0 / 3 * mels)
    width = np.diff(pts)
    rel = pts[None, :] - freqs[:, None]  # (201, n_mels + 2)
    bank = np.maximum(0.0, np.minimum(-rel[:, :-2] / width[:-1], rel[:, 2:] / width[1:]))
    bank = bank * (2.0 / (pts[2:] - pts[:-2]))[None, :]
    return np.ascontiguousarray(bank.T)


_tables: Dict[tuple, tuple] = {}


def _logmel_tables(device, n_mels: int):
    """window [400] (symmetric Hann, mlx_audio/utils.py:11-14), cos | sin [2][400] of 2 pi j / 400, bank transposed [201][n_mels]: float64 on the
    host, fp32 on the device, once per (device, n_mels)."""
    import torch

    key = (str(device), n_mels)
    if key not in _tables:
        j = np.arange(N_FFT, dtype=np.float64)
        window = 0.5 * (1.0 - np.cos(2.0 * np.pi * j / (N_FFT - 1)))
        cs = np.stack([np.cos(2.0 * np.pi * j / N_FFT), np.sin(2.0 * np.pi * j / N_FFT)])
        _tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(device)
                             for t in (window, cs, mel_filters(n_mels).T))
    return _tables[key]


def check_log_mel_lengths(lengths, padding: int) -> None:
    """The reflect padding of the STFT needs 201 samples (mlx_audio/utils.py:82-84)."""
    for n in lengths:
        if n + padding < N_FFT // 2 + 1:
            raise ValueError(f"log_mel_spectrogram: {n} samples + {padding} padding is shorter than the {N_FFT // 2 + 1} the reflect padding needs")


def log_mel_spectrogram(audio, n_mels: int = 80, padding: int = 0, device: str = "cuda:0"):
    """audio.py:41-82 on the device.  audio: a 1-D numpy array or torch tensor (CPU or device) of 16 kHz samples -> fp32 device tensor
    (n_frames, n_mels), n_frames = (len + padding) // 160; or a list of them (a ragged batch, one launch) -> a list of such tensors."""
    if n_mels not in (80, 128):
        raise ValueError("n_mels must be 80 or 128")
    if padding < 0:
        raise ValueError("padding must be >= 0")
    single = not isinstance(audio, (list, tuple))
    clips = [audio] if single else list(audio)
    if not clips:
        return []
    lengths = []
    for a in clips:
        if a.ndim != 1:
            raise ValueError("log_mel_spectrogram takes 1-D audio")
        lengths.append(int(a.shape[0]))
    check_log_mel_lengths(lengths, padding)
    import torch

    for a in clips:
        if _is_torch(a) and a.is_cuda:
            device = a.device
            break
    dev = torch.device(device)
    with torch.cuda.device(dev):
        B, ldx = len(clips), max(lengths)
        if B == 1:
            x = torch.as_tensor(clips[0]).to(device=dev, dtype=torch.float32).contiguous().view(1, -1)
        else:
            x = torch.zeros((B, ldx), dtype=torch.float32, device=dev)
            for b, a in enumerate(clips):
                x[b, : lengths[b]] = torch.as_tensor(a).to(device=dev, dtype=torch.float32)
        out = log_mel_rows(x, lengths, n_mels, padding)
    res = [out[b, : (lengths[b] + padding) // HOP_LENGTH] for b in range(B)]
    return res[0] if single else res


def log_mel_rows(x, lengths, n_mels: int = 80, padding: int = 0):
    """The kernel call itself: x fp32 device [B][ldx] (row b holds lengths[b] samples; what lies behind them is never read) ->
    fp32 [B][max frames][n_mels], rows past a clip's frame count zero."""
    import torch

    from . import _lib

    lib = _lib.load()
    check_log_mel_lengths(lengths, padding)
    B, ldx = x.shape
    if len(lengths) != B or max(lengths) > ldx or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("log_mel_rows: x must be contiguous fp32 [B][ldx] with lengths[b] <= ldx")
    dev = x.device
    with torch.cuda.device(dev):
        window, cs, fbT = _logmel_tables(dev, n_mels)
        F_rows = max((n + padding) // HOP_LENGTH for n in lengths)
        n_dev = torch.tensor(lengths, dtype=torch.int32).to(dev)
        partial = torch.empty((B, F_rows), dtype=torch.float32, device=dev)
        out = torch.empty((B, F_rows, n_mels), dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.kk_op_log_mel(st, B, C.c_void_p(x.data_ptr()), ldx, C.c_void_p(n_dev.data_ptr()), padding, n_mels,
                                     C.c_void_p(window.data_ptr()), C.c_void_p(cs.data_ptr()), C.c_void_p(fbT.data_ptr()),
                                     C.c_void_p(partial.data_ptr()), C.c_void_p(out.data_ptr()), F_rows), "kk_op_log_mel")
    return out


def mel_windows(mels, seeks, sizes, W: int):
    """The windows of a transcription round in ONE launch (kk_op_mel_windows): row r is `pad_or_trim(mels[r][seeks[r] : seeks[r] + sizes[r]], W,
    axis=-2)` (whisper.py:592-596).  mels: fp32 device tensors (frames, n_mels), one per row -- views of different allocations are fine, the same
    tensor may serve several rows; 0 <= sizes[r] <= W and seeks[r] + sizes[r] <= frames of row r.  -> fp32 device (R, W, n_mels)."""
    import torch

    from . import _lib

    lib = _lib.load()
    R = len(mels)
    if not 1 <= R <= _lib.WHISPER_MAX_ROWS or len(seeks) != R or len(sizes) != R:
        raise ValueError(f"mel_windows takes 1 .. {_lib.WHISPER_MAX_ROWS} spectrograms with one seek and one size each")
    if W < 1:
        raise ValueError("W must be >= 1")
    n_mels = int(mels[0].shape[-1])
    for m in mels:
        if not _is_torch(m) or not m.is_cuda or m.dtype != torch.float32 or m.ndim != 2 or m.shape[1] != n_mels or not m.is_contiguous() or m.device != mels[0].device:
            raise ValueError("mel_windows: every spectrogram must be a contiguous fp32 (frames, n_mels) tensor on one device")
    for r in range(R):
        if not 0 <= sizes[r] <= W or seeks[r] < 0 or seeks[r] + sizes[r] > mels[r].shape[0]:
            raise ValueError(f"mel_windows: row {r}: frames {seeks[r]} .. {seeks[r] + sizes[r]} of {mels[r].shape[0]}, W = {W}")
    dev = mels[0].device
    src = (C.c_void_p * R)(*[m.data_ptr() for m in mels])
    arr = lambda v: (C.c_int32 * R)(*[int(x) for x in v])  # noqa: E731
    with torch.cuda.device(dev):
        out = torch.empty((R, W, n_mels), dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.kk_op_mel_windows(st, R, src, arr([m.shape[0] for m in mels]), arr(seeks), arr(sizes), W, n_mels, C.c_void_p(out.data_ptr())),
                   "kk_op_mel_windows")
    return out


class Span(NamedTuple):
    """A row of `span_windows`: `n` >= 1 samples of the 1-D fp32 device tensor `buf`, from element `start` on when `ring_len` is 0, else samples
    (start + i) % ring_len of a ring (`ring.py`; `start` is a 64-bit stream position)."""
    buf: object
    ring_len: int
    start: int
    n: int


SPAN_LDS_WINDOW, SPAN_LDS_TABLE = 1536, 512  # floats of a frame's source samples and of the phase table that kk_op_log_mel_spans keeps in LDS

_span_tabs: Dict[tuple, object] = {}


def span_ratio(src_rate: int):
    """(L, M) of `src_rate` -> 16 kHz, or ValueError naming a ratio that `span_windows` does not serve (`resample.ratio`'s bound, and a frame's
    source samples and phase table must fit the kernel's LDS: 8, 12, 16, 24, 32 and 48 kHz do)."""
    from . import resample as RS

    L, M = RS.ratio(src_rate, SAMPLE_RATE)
    if L != M:
        T = RS.taps_per_output(L, M)
        if L * (T | 1) > SPAN_LDS_TABLE or (N_FFT - 1) * M // L + T + 2 > SPAN_LDS_WINDOW:
            raise ValueError(f"span_windows: {src_rate} -> {SAMPLE_RATE} Hz is {L} / {M}: a frame of that ratio does not fit the kernel's LDS "
                             f"(phase table {L * (T | 1)} of {SPAN_LDS_TABLE} floats, source samples {(N_FFT - 1) * M // L + T + 2} of {SPAN_LDS_WINDOW})")
    return L, M


def span_len16(n: int, L: int, M: int) -> int:
    """16 kHz samples of an n-sample span: `resample.out_len`."""
    return -(-int(n) * int(L) // int(M))


def check_spans(spans, W: int, src_rate: int = 24000):
    """The host checks of `span_windows` without a device: -> (L, M).  ValueError names the row whose span is longer than one window."""
    L, M = span_ratio(src_rate)
    if W < 3:
        raise ValueError("W must be >= 3")
    for r, sp in enumerate(spans):
        ring_len, start, n = int(sp[1]), int(sp[2]), int(sp[3])
        if n < 1 or start < 0 or ring_len < 0 or (ring_len and n > ring_len):
            raise ValueError(f"span_windows: row {r}: span [{start}, + {n}) of ring {ring_len}")
        if span_len16(n, L, M) > W * HOP_LENGTH:
            raise ValueError(f"span_windows: row {r}: {n} samples at {src_rate} Hz are {span_len16(n, L, M)} at 16 kHz, more than the "
                             f"{W * HOP_LENGTH} of a window of {W} frames")
    return L, M


def span_windows(spans, W: int, n_mels: int = 80, src_rate: int = 24000):
    """Utterances that lie on the device become Whisper windows in ONE launch pair (kk_op_log_mel_spans).  spans: 1 ..
    WHISPER_MAX_ROWS `Span`s (or such tuples) at `src_rate`; the rows may name different allocations or the same one.  Row r is, bit for bit,
    `mel_windows([log_mel_spectrogram(resample.resample(x, src_rate, 16000), n_mels, padding=W * 160)], [0], [W], W)[0]` for the span's samples
    x; what lies outside a span is never read.  -> fp32 device (R, W, n_mels).  ValueError for a span longer than a window (it names the row)
    and for a ratio that is not served (`span_ratio`)."""
    import torch

    from . import _lib
    from . import resample as RS

    if n_mels not in (80, 128):
        raise ValueError("n_mels must be 80 or 128")
    spans = [Span(*sp) for sp in spans]
    R = len(spans)
    if not 1 <= R <= _lib.WHISPER_MAX_ROWS:
        raise ValueError(f"span_windows takes 1 .. {_lib.WHISPER_MAX_ROWS} spans")
    L, M = check_spans(spans, W, src_rate)
    dev = spans[0].buf.device
    for r, sp in enumerate(spans):
        b = sp.buf
        if not _is_torch(b) or not b.is_cuda or b.dtype != torch.float32 or b.ndim != 1 or not b.is_contiguous() or b.device != dev:
            raise ValueError("span_windows: every buffer must be a contiguous 1-D fp32 tensor on one device")
        if (sp.ring_len > b.shape[0]) if sp.ring_len else (sp.start + sp.n > b.shape[0]):
            raise ValueError(f"span_windows: row {r}: span [{sp.start}, + {sp.n}) of ring {sp.ring_len} does not lie in its buffer of {b.shape[0]}")
    lib = _lib.load()
    with torch.cuda.device(dev):
        window, cs, fbT = _logmel_tables(dev, n_mels)
        tab, T = None, 0
        if L != M:
            key = (str(dev), L, M)
            if key not in _span_tabs:
                _span_tabs[key] = torch.from_numpy(np.array(RS.phase_table(L, M))).to(dev)
            tab = _span_tabs[key]
            T = int(tab.shape[1])
        partial = torch.empty((R, W + 2), dtype=torch.float32, device=dev)
        out = torch.empty((R, W, n_mels), dtype=torch.float32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        i32 = lambda v: (C.c_int32 * R)(*[int(x) for x in v])  # noqa: E731
        i64 = lambda v: (C.c_int64 * R)(*[int(x) for x in v])  # noqa: E731
        _lib.check(lib.kk_op_log_mel_spans(st, R, (C.c_void_p * R)(*[sp.buf.data_ptr() for sp in spans]), i64([sp.buf.shape[0] for sp in spans]),
                                           i32([sp.ring_len for sp in spans]), i64([sp.start for sp in spans]), i32([sp.n for sp in spans]), W, L, M,
                                           C.c_void_p(tab.data_ptr() if tab is not None else None), T, n_mels, C.c_void_p(window.data_ptr()),
                                           C.c_void_p(cs.data_ptr()), C.c_void_p(fbT.data_ptr()), C.c_void_p(partial.data_ptr()),
                                           C.c_void_p(out.data_ptr())), "kk_op_log_mel_spans")
    return out


@dataclass
class ModelDimensions:
    """whisper.py:67-78."""
    n_mels: int
    n_audio_ctx: int
    n_audio_state: int
    n_audio_head: int
    n_audio_layer: int
    n_vocab: int
    n_text_ctx: int
    n_text_state: int
    n_text_head: int
    n_text_layer: int


DIMENSION_KEYS = tuple(f.name for f in fields(ModelDimensions))


def is_whisper_config(config: dict) -> bool:
    return config.get("model_type") == "whisper" or all(k in config for k in DIMENSION_KEYS)


def _as_f32(v) -> np.ndarray:
    if _is_torch(v):
        v = v.detach().float().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype=np.float32)


def encoder_shapes(dims: ModelDimensions) -> Dict[str, tuple]:
    """name -> shape of every encoder parameter, by the MLX checkpoint's names and layouts (conv weights [O, K, I]); whisper.py:171-187."""
    D, M = dims.n_audio_state, dims.n_mels
    s = {"encoder.conv1.weight": (D, 3, M), "encoder.conv1.bias": (D,), "encoder.conv2.weight": (D, 3, D), "encoder.conv2.bias": (D,),
         "encoder.ln_post.weight": (D,), "encoder.ln_post.bias": (D,)}
    for i in range(dims.n_audio_layer):
        p = f"encoder.blocks.{i}."
        for lin in ("query", "value", "out"):
            s[p + f"attn.{lin}.weight"] = (D, D)
            s[p + f"attn.{lin}.bias"] = (D,)
        s[p + "attn.key.weight"] = (D, D)  # no bias (whisper.py:95)
        s[p + "mlp1.weight"], s[p + "mlp1.bias"] = (4 * D, D), (4 * D,)
        s[p + "mlp2.weight"], s[p + "mlp2.bias"] = (D, 4 * D), (D,)
        for ln in ("attn_ln", "mlp_ln"):
            s[p + ln + ".weight"] = s[p + ln + ".bias"] = (D,)
    return s


def split_weights(dims: ModelDimensions, weights: dict):
    """-> (encoder tensors as fp32 numpy in the MLX layouts, everything else untouched).  A conv weight in the PyTorch layout [O, I, K] is told
    apart by its shape and transposed.  A missing or misshapen encoder tensor is a ValueError that names it."""
    want = encoder_shapes(dims)
    enc, rest = {}, {}
    for k, v in weights.items():
        if k in want:
            enc[k] = v
        elif k.startswith("encoder.") and k != "encoder._positional_embedding" and k != "encoder.positional_embedding":
            raise ValueError(f"unexpected encoder tensor: {k}")
        else:
            rest[k] = v
    out = {}
    for k, shape in want.items():
        if k not in enc:
            raise ValueError(f"missing encoder tensor: {k}")
        a = _as_f32(enc[k])
        if len(shape) == 3 and a.shape != shape and a.shape == (shape[0], shape[2], shape[1]):
            a = np.ascontiguousarray(a.transpose(0, 2, 1))  # [O, I, K] -> [O, K, I]
        if a.shape != shape:
            raise ValueError(f"encoder tensor {k} has shape {tuple(a.shape)}, expected {shape}")
        out[k] = a
    return out, rest


class Model:
    """whisper.py:251-353, audio side.  The weights are held as bf16 on the device (fp16 / fp32 checkpoints are rounded to nearest even)."""

    def __init__(self, dims: ModelDimensions, dtype: str = "bfloat16", device: str = "cuda:0"):
        if str(dtype).replace("torch.", "") != "bfloat16":
            raise ValueError("the encoder runs on bf16 matrix cores: dtype must be 'bfloat16' (an f16 mode is not built)")
        self.dims = dims
        self.dtype = "bfloat16"
        self.device_name = device
        self.decoder_weights: Dict[str, object] = {}
        self._h = None
        self._ws = None
        self._lib = None
        self._text = None
        self._server = None  # the open WhisperBatcher, if any (serve)
        self._alignment_heads = None  # the default is made on first use

    # ---- weights ---------------------------------------------------------------------------------------------------------------------
    def load_weights(self, weights: dict, quantization: Optional[dict] = None, weight_storage: str = "packed") -> "Model":
        """`quantization`: config["quantization"] of an MLX 4- / 8-bit checkpoint (group_size, bits, per-layer entries), whose `weights` hold
        `{p}.weight` (uint32) / `{p}.scales` / `{p}.biases` triplets.  weight_storage "packed": the decoder's quantised matrices and the token embedding
        stay the checkpoint's integers in device memory, matrix by matrix where the format allows (quant.whisper_weight_route; `weight_report()` says
        what became of each); "dequantized": everything is dequantised here and runs as bf16.  Both compute the same bits.  The encoder's
        Linears are dequantised either way."""
        check_weight_storage(weight_storage)
        packed = {}
        if quantization is not None:
            weights, packed = split_quantised(weights, quantization, weight_storage)
        enc, rest = split_weights(self.dims, weights)
        self.decoder_weights = rest  # decoder.* (and alignment data): kept for the text side, not touched
        import torch

        from . import _lib

        lib = self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.KokoroHipError("whisper.Model needs a GPU: the encoder has no CPU fallback")
        self.device = torch.device(self.device_name)
        kc = _lib.KKWhisperConfig()
        for k in ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer"):
            setattr(kc, k, int(getattr(self.dims, k)))
        self._release()
        h = C.c_void_p()
        _lib.check(lib.kk_whisper_create(C.byref(kc), C.byref(h)), "kk_whisper_create")
        self._h = h
        with torch.cuda.device(self.device):
            for name, a in enc.items():
                shp = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(lib.kk_whisper_load_tensor(h, name.encode(), shp, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_whisper_load_tensor")
            _lib.check(lib.kk_whisper_finalize(h, self._stream()), "kk_whisper_finalize")
            dec = decoder_tensors(self.dims, rest, packed)  # None: no complete decoder set, the model stays encoder-only
            if dec is not None:
                from .whisper_decoding import TextRuntime

                self._text = TextRuntime(lib, self.dims, dec, self.device, self._stream(), quantized=packed)
        return self

    def weight_report(self) -> dict:
        """What the decoder's weights occupy on the device and how its matrices are stored: `matrix_bytes` (the Linears and the token embedding),
        `resident_bytes` (those plus biases, LayerNorms and positions), `packed` / `bf16` (matrix counts; the stacked cross key | value counts once)
        and `fallbacks`: name -> reason for every quantised tensor that was dequantised into a bf16 matrix."""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        return self._text.weight_report()

    @classmethod
    def from_pretrained(cls, path: str, dtype: str = "bfloat16", device: str = "cuda:0", weight_storage: Optional[str] = None) -> "Model":
        """whisper.py:320-353 for a LOCAL directory: config.json + weights.safetensors or weights.npz.  Never goes to the network.
        weight_storage: None refuses a checkpoint with config["quantization"]; "packed" / "dequantized" load it (`load_weights`).  A checkpoint
        that is not quantised ignores it."""
        check_weight_storage(weight_storage, allow_none=True)
        model_path = Path(path)
        if not model_path.is_dir():
            raise FileNotFoundError(f"{path} is not a local directory (checkpoints are not downloaded)")
        with open(model_path / "config.json", encoding="utf-8") as f:
            config = json.load(f)
        dims = dimensions_from_config(config, weight_storage)
        wf = model_path / "weights.safetensors"
        if wf.exists():
            from safetensors import safe_open

            weights = {}
            with safe_open(str(wf), framework="pt") as f:
                for k in f.keys():
                    weights[k] = f.get_tensor(k)
        else:
            wf = model_path / "weights.npz"
            if not wf.exists():
                raise FileNotFoundError(f"no weights.safetensors or weights.npz in {path}")
            with np.load(str(wf)) as z:
                weights = {k: z[k] for k in z.files}
        if config.get("quantization") is None:
            return cls(dims, dtype, device).load_weights(weights)
        return cls(dims, dtype, device).load_weights(weights, config["quantization"], weight_storage)

    # ---- the encoder -----------------------------------------------------------------------------------------------------------------
    def embed_audio(self, mel):
        """whisper.py:295 -> AudioEncoder.__call__: mel (2 * n_audio_ctx, n_mels) or (B, 2 * n_audio_ctx, n_mels) -> fp32 device tensor
        (n_audio_ctx, n_audio_state) or (B, ...)."""
        d = self.dims
        shape = tuple(mel.shape)
        assert len(shape) in (2, 3) and shape[-2:] == (2 * d.n_audio_ctx, d.n_mels), "incorrect audio shape"
        if self._h is None:
            raise RuntimeError("whisper.Model.embed_audio: load_weights first")
        import torch

        from . import _lib

        lib = self._lib
        x = torch.as_tensor(mel).to(device=self.device, dtype=torch.float32).contiguous()
        B = 1 if x.ndim == 2 else x.shape[0]
        with torch.cuda.device(self.device):
            need = int(lib.kk_whisper_encode_workspace_bytes(self._h, B))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            out = torch.empty((B, d.n_audio_ctx, d.n_audio_state), dtype=torch.float32, device=self.device)
            _lib.check(lib.kk_whisper_encode(self._h, self._stream(), B, C.c_void_p(x.data_ptr()), C.c_void_p(self._ws.data_ptr()), need,
                                             C.c_void_p(out.data_ptr())), "kk_whisper_encode")
        return out[0] if x.ndim == 2 else out

    # ---- the text side -----------------------------------------------------------------------------------------------------------------
    @property
    def has_text_decoder(self) -> bool:
        return self._text is not None

    def logits(self, tokens=None, audio_features=None, *a, **kw):
        """whisper.py:298: tokens (B, S) ints, audio_features (B, n_audio_ctx, n_audio_state) -> fp32 device (B, S, n_vocab).  No cache is carried
        over between calls."""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        import torch

        d = self.dims
        tokens = torch.as_tensor(tokens)
        feats = torch.as_tensor(audio_features)
        if tokens.ndim != 2 or feats.ndim != 3 or tokens.shape[0] != feats.shape[0] or tuple(feats.shape[1:]) != (d.n_audio_ctx, d.n_audio_state):
            raise ValueError("logits takes tokens (B, S) and audio features (B, n_audio_ctx, n_audio_state)")
        if not 1 <= tokens.shape[1] <= d.n_text_ctx:
            raise ValueError(f"1 <= S <= n_text_ctx = {d.n_text_ctx}")
        with torch.cuda.device(self.device):
            self._text.set_audio(feats.to(device=self.device, dtype=torch.float32).contiguous())
            return self._text.forward(tokens.to(device=self.device, dtype=torch.int32).contiguous(), True)

    # ---- token timestamps (whisper.py:272-303) ------------------------------------------------------------------------------------------
    @property
    def alignment_heads(self) -> np.ndarray:
        """int array (n, 2) of (layer, head); by default every head of the upper half of the decoder's layers (whisper.py:274-278)"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        if self._alignment_heads is None:
            all_heads = np.zeros((self.dims.n_text_layer, self.dims.n_text_head), dtype=bool)
            all_heads[self.dims.n_text_layer // 2:] = True
            self._alignment_heads = np.asarray(all_heads.nonzero()).T.astype(np.int64)
        return self._alignment_heads

    def set_alignment_heads(self, dump):
        """whisper.py:280-293: an int array (n, 2), or the base85-encoded gzip of a boolean (n_text_layer, n_text_head) mask"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        d = self.dims
        if isinstance(dump, np.ndarray):
            heads = np.asarray(dump)
            if heads.ndim != 2 or heads.shape[1] != 2 or heads.shape[0] < 1 or heads.dtype.kind not in "iu":
                raise ValueError("alignment heads must be a non-empty integer array of shape (n, 2)")
            heads = heads.astype(np.int64)
        elif isinstance(dump, bytes):
            array = np.frombuffer(gzip.decompress(base64.b85decode(dump)), dtype=bool).copy()
            if array.size != d.n_text_layer * d.n_text_head:
                raise ValueError(f"the alignment-head mask holds {array.size} entries, the decoder has {d.n_text_layer} x {d.n_text_head} heads")
            heads = np.asarray(array.reshape(d.n_text_layer, d.n_text_head).nonzero()).T.astype(np.int64)
            if heads.shape[0] < 1:
                raise ValueError("the alignment-head mask selects no head")
        else:
            raise ValueError(f"Invalid type for `dump`: {type(dump)}. Expected a np.ndarray or base85-encoded bytes containing"
                             " alignment_head information")
        if (heads < 0).any() or (heads[:, 0] >= d.n_text_layer).any() or (heads[:, 1] >= d.n_text_head).any():
            raise ValueError(f"alignment heads outside the decoder's {d.n_text_layer} layers of {d.n_text_head} heads")
        self._alignment_heads = heads

    def forward_with_cross_qk(self, mel_or_features, tokens):
        """whisper.py:301-303: a mel (B, 2 n_audio_ctx, n_mels) or audio features (B, n_audio_ctx, n_audio_state), tokens (B, S) ints ->
        (logits fp32 device (B, S, n_vocab), [per layer: the raw cross-attention scores, fp32 device (B, n_text_head, S, n_audio_ctx)])"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        import torch

        from .whisper_decoding import _features

        d = self.dims
        tokens = torch.as_tensor(tokens)
        if tokens.ndim != 2 or not 1 <= tokens.shape[1] <= d.n_text_ctx:
            raise ValueError(f"forward_with_cross_qk takes tokens (B, S) with 1 <= S <= n_text_ctx = {d.n_text_ctx}")
        feats, _ = _features(self, mel_or_features)
        if feats.shape[0] != tokens.shape[0]:
            raise ValueError("forward_with_cross_qk: the batch sizes of the audio and of the tokens differ")
        pairs = np.asarray([(l, h) for l in range(d.n_text_layer) for h in range(d.n_text_head)], np.int32)
        with torch.cuda.device(self.device):
            self._text.set_audio(feats)
            logits, qk = self._text.forward_qk(tokens.to(device=self.device, dtype=torch.int32).contiguous(), pairs, d.n_audio_ctx)
        qk = qk.view(tokens.shape[0], d.n_text_layer, d.n_text_head, tokens.shape[1], d.n_audio_ctx)
        return logits, [qk[:, l] for l in range(d.n_text_layer)]

    def decode(self, *a, **kw):
        """decoding.py:710-742 at token level, see whisper_decoding.decode"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_decoding import decode

        return decode(self, *a, **kw)

    def sample(self, *a, **kw):
        """`decode` at temperature > 0 with `best_of` candidates and the maximum-likelihood ranker, see whisper_sampling.sample"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_sampling import sample

        return sample(self, *a, **kw)

    def sample_candidates(self, *a, **kw):
        """every sampled candidate of every window, before the ranker, see whisper_sampling.sample_candidates"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_sampling import sample_candidates

        return sample_candidates(self, *a, **kw)

    def decode_with_fallback(self, *a, **kw):
        """whisper.py:503-541 for a batch of windows, see whisper_sampling.decode_with_fallback"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_sampling import decode_with_fallback

        return decode_with_fallback(self, *a, **kw)

    def beam_search(self, *a, **kw):
        """`decode` by beam search (`beam_size`, `patience`) at temperature 0, see whisper_beam.beam_search"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_beam import beam_search

        return beam_search(self, *a, **kw)

    def beam_candidates(self, *a, **kw):
        """every window's `beam_size` candidates after the beam's finalize, before the ranker, see whisper_beam.beam_candidates"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_beam import beam_candidates

        return beam_candidates(self, *a, **kw)

    def beam_decode_with_fallback(self, *a, **kw):
        """the temperature fallback with beam search as its temperature-0 pass, see whisper_beam.decode_with_fallback"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_beam import decode_with_fallback

        return decode_with_fallback(self, *a, **kw)

    def serve(self, max_rows: int = 8, eos_check_interval: int = 8, max_round_tokens: int = 256):
        """A running decoder batch that windows join and leave (whisper_serve.WhisperBatcher): `submit(window, options)` returns a Future of
        the DecodingResult `decode` would return for that window alone.  `decode`, `logits`, `detect_language` and `find_alignment` keep working on this
        model between the batcher's rounds.  One batcher per model at a time: close() it before asking for another."""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_serve import WhisperBatcher

        if self._server is not None and not self._server.closed:
            raise RuntimeError("this model's WhisperBatcher is still open: close() it first")
        self._server = WhisperBatcher(self, max_rows=max_rows, eos_check_interval=eos_check_interval, max_round_tokens=max_round_tokens)
        return self._server

    def generate(self, *a, **kw):
        raise NotImplementedError(_NOT_BUILT)

    def transcribe(self, audio, **kw):
        """whisper.py:355-866, the reference's `generate`, under OpenAI's name for it: one recording (1-D samples at 16 kHz) -> TranscribeResult, a list of
        recordings -> a list, all of them on one running decoder batch; see whisper_transcribe.transcribe"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_transcribe import transcribe

        return transcribe(self, audio, **kw)

    def beam_transcribe(self, audio, **kw):
        """`transcribe` with beam search at temperature 0 and `best_of` samples above it, every window a group of rows of the one running decoder
        batch; see whisper_transcribe.beam_transcribe"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_transcribe import beam_transcribe

        return beam_transcribe(self, audio, **kw)

    def detect_language(self, *a, **kw):
        """decoding.py:20-79, see whisper_decoding.detect_language"""
        if self._text is None:
            raise NotImplementedError(_NOT_BUILT)
        from .whisper_decoding import detect_language

        return detect_language(self, *a, **kw)

    @property
    def is_multilingual(self) -> bool:
        return self.dims.n_vocab >= 51865

    @property
    def num_languages(self) -> int:
        return self.dims.n_vocab - 51765 - int(self.is_multilingual)

    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _release(self):
        if getattr(self, "_server", None) is not None:
            self._server.close()  # its rows live in the text handle's memory
        self._server = None
        if getattr(self, "_h", None) is not None and self._lib is not None:
            self._lib.kk_whisper_destroy(self._h)
        self._h = None
        if getattr(self, "_text", None) is not None:
            self._text.release()
        self._text = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


WEIGHT_STORAGES = ("packed", "dequantized")


def check_weight_storage(weight_storage, allow_none: bool = False) -> None:
    if not (weight_storage in WEIGHT_STORAGES or (allow_none and weight_storage is None)):
        raise ValueError(f"weight_storage must be 'packed' or 'dequantized', not {weight_storage!r}")


def split_quantised(weights: dict, quantization: dict, weight_storage: str):
    """(weights with every quantised tensor that does not stay packed dequantised to fp32, {name: (words, scales, biases, group_size, bits)} of the
    ones that go to the text handle as they are).  A layer is quantised iff `{p}.scales` and `{p}.biases` come with `{p}.weight`; per-layer entries
    of `quantization` are honoured as quant.split_triplets does.  Under "packed" every `decoder.*` triplet is handed on -- the handle decides per
    matrix and dequantises by the same rule what it cannot keep packed -- and everything else (the encoder's Linears) is dequantised here."""
    from .quant import dequantize_affine, split_triplets

    as_np = {k: (v.float().numpy() if _is_torch(v) and v.dtype.is_floating_point else (v.numpy() if _is_torch(v) else np.asarray(v))) for k, v in weights.items()}
    per_layer = {k: v for k, v in quantization.items() if k not in ("group_size", "bits")}
    plain, triplets = split_triplets(as_np, int(quantization["group_size"]), int(quantization["bits"]), per_layer)
    packed = {}
    for k, t in triplets.items():
        if weight_storage == "packed" and k.startswith("decoder."):
            packed[k] = t
        else:
            plain[k] = dequantize_affine(*t)
    return plain, packed


def dimensions_from_config(config: dict, weight_storage: Optional[str] = None) -> ModelDimensions:
    """whisper.py:329-334.  A quantised checkpoint is refused unless the caller says how its weights are to be stored (`Model.from_pretrained`)."""
    if config.get("quantization") is not None and weight_storage is None:
        raise ValueError("quantised Whisper checkpoints are not supported yet without a weight_storage: pass weight_storage='packed' (the decoder's "
                         "matrices stay quantised in device memory) or 'dequantized'")
    missing = [k for k in DIMENSION_KEYS if k not in config]
    if missing:
        raise ValueError(f"config.json lacks the Whisper dimensions {missing}")
    return ModelDimensions(**{k: int(config[k]) for k in DIMENSION_KEYS})


def load_model(model_path, dtype: Optional[str] = None, **kwargs) -> Model:
    """What utils.load_model routes a Whisper checkpoint to."""
    return Model.from_pretrained(str(model_path), dtype or "bfloat16", **{k: v for k, v in kwargs.items() if k in ("device", "weight_storage")})
