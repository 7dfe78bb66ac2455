"""Host mirror of the reference's mlx_audio/stt/models/whisper/timing.py at token level: `median_filter`, `dtw`, `WordTiming` and `find_alignment`
("when was each token spoken", from the cross-attention of the alignment heads).  Where the reference leaves the accelerator -- scipy's median filter
on the host, a numba loop for the warping -- everything up to the per-token frames runs in libkokoro_hip.so (kk_whisper_text_forward_qk,
kk_op_whisper_align_matrix, kk_op_whisper_dtw, kk_op_whisper_median_filter; csrc/kk_whisper_align.hip), and a batch of windows runs in one pass.

There is no tokenizer here, so ids go in and times come out: `find_alignment` returns one `TokenTiming` per text token, or, when the caller that owns
a tokenizer passes `words` (the token lists of its words), `WordTiming`s by the reference's boundary arithmetic with `word=""`.  `merge_punctuations` and
`add_word_timestamps` need the text of the words and are not built."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np


@dataclass
class TokenTiming:
    token: int
    start: float
    end: float
    probability: float


@dataclass
class WordTiming:
    """timing.py:103-109"""
    word: str
    tokens: List[int]
    start: float
    end: float
    probability: float


@dataclass
class Alignment:
    """What `find_alignment` is made from, for one window: `matrix` the fp32 device view (rows, frames) that was warped (the rows of no_timestamps and
    of every text token), the path as two int arrays, `first_frames` (rows,) the path's first frame of every row (the reference's
    `time_indices[jumps]`), `probabilities` (n_tokens,) and the tokens themselves."""
    tokens: List[int]
    matrix: object
    text_indices: np.ndarray
    time_indices: np.ndarray
    first_frames: np.ndarray
    probabilities: np.ndarray


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device_f32(x):
    import torch

    if not (type(x).__module__.split(".")[0] == "torch" and x.is_cuda):
        raise ValueError("expected a tensor on the device")
    return x.to(torch.float32).contiguous()


def median_filter(x, filter_width: int):
    """timing.py:19-44 on the device: a median filter of odd width along the last dimension with reflect padding; an input no longer than
    filter_width // 2 is returned as it is.  x: a device tensor of any rank -> fp32 device tensor of the same shape."""
    import torch

    from . import _lib

    if not (filter_width > 0 and filter_width % 2 == 1):
        raise ValueError("`filter_width` should be an odd number")
    x = _device_f32(x)
    n = x.shape[-1]
    if n <= filter_width // 2 or x.numel() == 0:
        return x
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().kk_op_whisper_median_filter(_stream(x.device), x.numel() // n, n, _ptr(x), n, int(filter_width), _ptr(out), n),
                   "kk_op_whisper_median_filter")
    return out


def dtw_rows(x, n_rows: Sequence[int], n_cols: Sequence[int], negate: bool = False):
    """The kernel call itself: x fp32 device (B, rows_max, ld), item b is its first n_rows[b] x n_cols[b] (what lies behind is never read) ->
    (text_indices (B, cap), time_indices (B, cap), lengths (B,), first_cols (B, rows_max)) as int32 device tensors, cap = rows_max + ld"""
    import torch

    from . import _lib

    lib = _lib.load()
    if x.ndim != 3 or x.dtype != torch.float32 or not x.is_contiguous() or len(n_rows) != x.shape[0] or len(n_cols) != x.shape[0]:
        raise ValueError("dtw_rows: x must be contiguous fp32 (B, rows_max, ld) with one row and column count per item")
    B, rows_max, ld = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        nr = torch.tensor(list(n_rows), dtype=torch.int32).to(dev)
        nc = torch.tensor(list(n_cols), dtype=torch.int32).to(dev)
        cap = rows_max + ld
        ti = torch.zeros((B, cap), dtype=torch.int32, device=dev)
        tj = torch.zeros((B, cap), dtype=torch.int32, device=dev)
        ln = torch.zeros((B,), dtype=torch.int32, device=dev)
        first = torch.zeros((B, rows_max), dtype=torch.int32, device=dev)
        need = int(lib.kk_op_whisper_dtw_workspace_bytes(B, rows_max, ld))
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        _lib.check(lib.kk_op_whisper_dtw(_stream(dev), B, _ptr(x), rows_max * ld, ld, _ptr(nr), rows_max, _ptr(nc), ld, int(bool(negate)), _ptr(ti), _ptr(tj),
                                         _ptr(ln), _ptr(first), _ptr(ws), ws.numel()), "kk_op_whisper_dtw")
    return ti, tj, ln, first


def dtw(x) -> np.ndarray:
    """timing.py:98-100 on the device: x a 2-D device tensor (N, M) -> the (2, L) integer array of (text_indices, time_indices)"""
    x = _device_f32(x)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("dtw takes a 2-D cost matrix with at least one row and one column")
    ti, tj, ln, _ = dtw_rows(x[None], [x.shape[0]], [x.shape[1]])
    L = int(ln[0])
    return np.stack([ti[0, :L].cpu().numpy(), tj[0, :L].cpu().numpy()]).astype(np.int64)


def align_matrix_rows(qk, n_rows: Sequence[int], n_frames: Sequence[int], medfilt_width: int = 7, qk_scale: float = 1.0, group: int = 0):
    """The kernel call itself (timing.py:147-155): qk fp32 device (B, heads, rows_max, ld) -> fp32 device (B, rows_max, ld) whose item b holds, in its
    first n_rows[b] x n_frames[b], the heads' mean of the median-filtered, column-standardised softmax; the cells behind stay zero."""
    import torch

    from . import _lib

    lib = _lib.load()
    if qk.ndim != 4 or qk.dtype != torch.float32 or not qk.is_contiguous() or len(n_rows) != qk.shape[0] or len(n_frames) != qk.shape[0]:
        raise ValueError("align_matrix_rows: qk must be contiguous fp32 (B, heads, rows_max, ld) with one row and frame count per item")
    B, H, rows_max, ld = qk.shape
    dev = qk.device
    with torch.cuda.device(dev):
        nr = torch.tensor(list(n_rows), dtype=torch.int32).to(dev)
        nf = torch.tensor(list(n_frames), dtype=torch.int32).to(dev)
        out = torch.zeros((B, rows_max, ld), dtype=torch.float32, device=dev)
        need = int(lib.kk_op_whisper_align_matrix_workspace_bytes(B, H, rows_max, ld, int(group)))
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        _lib.check(lib.kk_op_whisper_align_matrix(_stream(dev), B, H, _ptr(qk), H * rows_max * ld, rows_max * ld, ld, _ptr(nr), rows_max, _ptr(nf), ld,
                                                  float(qk_scale), int(medfilt_width), int(group), _ptr(out), ld, _ptr(ws), ws.numel()),
                   "kk_op_whisper_align_matrix")
    return out


def alignment_tokens(dims, text_tokens: Sequence[int], language: Optional[int] = None, task: str = "transcribe") -> Tuple[List[int], int, int]:
    """timing.py:125-132, 156 -> (the sequence [*sot_sequence, no_timestamps, *text_tokens, eot], the first and the end of the rows that are warped:
    len(sot_sequence) and len - 1, i.e. the no_timestamps row and every text token's row)"""
    from .whisper_decoding import sot_sequence, special_tokens

    tok = special_tokens(dims)
    if isinstance(language, str):
        raise ValueError("language must be a language-token id or index: the tokenizer is not built")
    sot = sot_sequence(tok, language, task, False)
    seq = [*sot, tok.no_timestamps, *(int(t) for t in text_tokens), tok.eot]
    return seq, len(sot), len(seq) - 1


def jump_frames(text_indices: np.ndarray, time_indices: np.ndarray) -> np.ndarray:
    """timing.py:169-170 without the division: the frame at which the path enters each row"""
    jumps = np.pad(np.diff(np.asarray(text_indices)), (1, 0), constant_values=1).astype(bool)
    return np.asarray(time_indices)[jumps]


def word_timings(words: Sequence[Sequence[int]], first_frames: np.ndarray, probabilities: np.ndarray) -> List[WordTiming]:
    """timing.py:167-183 for words given as token lists (the eot "word" the reference appends is implied): word w starts where its first token's row is
    entered and ends where the next word's is; its probability is the mean of its tokens'."""
    from .whisper import TOKENS_PER_SECOND

    if len(words) == 0:
        return []
    bounds = np.pad(np.cumsum([len(t) for t in words]), (1, 0))
    times = np.asarray(first_frames) / TOKENS_PER_SECOND
    if bounds[-1] + 1 != len(times):
        raise ValueError("`words` must concatenate to text_tokens")
    return [WordTiming("", [int(t) for t in w], float(times[i]), float(times[j]), float(np.mean(probabilities[i:j])))
            for w, i, j in zip(words, bounds[:-1], bounds[1:])]


def alignment_details(model, text_tokens, mel_or_features, num_frames, *, medfilt_width: int = 7, qk_scale: float = 1.0, language: Optional[int] = None,
                      task: str = "transcribe") -> List[Optional[Alignment]]:
    """One `Alignment` per item of a batch (None for an item without text tokens): text_tokens a list of token lists, the audio (B, ...),
    num_frames an int or a list.  Rows shorter than the longest are padded with eot behind their own eot (the decoder is causal: the positions
    before are unaffected), and every item is aligned over its own rows and its own num_frames // 2 frames."""
    import torch

    from .whisper_decoding import NOT_BUILT, _features, special_tokens

    if model._text is None:
        raise NotImplementedError(NOT_BUILT)
    d = model.dims
    tok = special_tokens(d)
    feats, _ = _features(model, mel_or_features)
    B = feats.shape[0]
    if len(text_tokens) != B:
        raise ValueError(f"{len(text_tokens)} token lists for {B} windows of audio")
    frames = [int(num_frames)] * B if np.isscalar(num_frames) else [int(n) for n in num_frames]
    if len(frames) != B or any(not 1 <= n // 2 <= d.n_audio_ctx for n in frames):
        raise ValueError(f"num_frames: one value per window, each with 1 <= num_frames // 2 <= n_audio_ctx = {d.n_audio_ctx}")
    if not (medfilt_width > 0 and medfilt_width % 2 == 1):
        raise ValueError("`medfilt_width` should be an odd number")
    live = [b for b in range(B) if len(text_tokens[b]) > 0]
    out: List[Optional[Alignment]] = [None] * B
    if not live:
        return out
    plans = [alignment_tokens(d, text_tokens[b], language, task) for b in live]
    n0 = plans[0][1]
    S = max(len(p[0]) for p in plans)
    if S > d.n_text_ctx:
        raise ValueError(f"{S} tokens exceed n_text_ctx = {d.n_text_ctx}")
    for b in live:
        if any(not 0 <= int(t) < tok.eot for t in text_tokens[b]):
            raise ValueError("text_tokens must be ids below eot")
    toks = np.full((len(live), S), tok.eot, np.int32)
    for i, (seq, _, _) in enumerate(plans):
        toks[i, : len(seq)] = seq
    n_frames = [frames[b] // 2 for b in live]
    n_keys = max(n_frames)
    heads = model.alignment_heads
    dev = model.device
    with torch.cuda.device(dev):
        rt = model._text
        rt.set_audio(feats[live].contiguous() if len(live) != B else feats)
        logits, qk = rt.forward_qk(torch.from_numpy(toks).to(dev), heads, n_keys)
        mat = align_matrix_rows(qk, [len(p[0]) for p in plans], n_frames, medfilt_width, qk_scale)
        warped = mat[:, n0: S - 1]  # the rows of no_timestamps and of the text tokens; the eot row of the longest item is dropped, shorter items end earlier
        rows = [p[2] - n0 for p in plans]
        ti, tj, ln, first = dtw_rows(warped.contiguous(), rows, n_frames, negate=True)
        ti, tj, ln, first = ti.cpu().numpy(), tj.cpu().numpy(), ln.cpu().numpy(), first.cpu().numpy()
        for i, b in enumerate(live):
            T = len(text_tokens[b])
            # timing.py:136-141: the softmax over the ids below eot at the positions that predict the text tokens, one item at a time
            p = torch.softmax(logits[i, n0: n0 + T, : tok.eot], dim=-1)
            ids = torch.as_tensor([int(t) for t in text_tokens[b]], dtype=torch.int64, device=dev)
            probs = p.gather(1, ids[:, None])[:, 0].cpu().numpy()
            L = int(ln[i])
            out[b] = Alignment(tokens=[int(t) for t in text_tokens[b]], matrix=warped[i, : rows[i], : n_frames[i]], text_indices=ti[i, :L].astype(np.int64),
                               time_indices=tj[i, :L].astype(np.int64), first_frames=first[i, : rows[i]].astype(np.int64), probabilities=probs)
    return out


def find_alignment(model, text_tokens, mel_or_features, num_frames, *, medfilt_width: int = 7, qk_scale: float = 1.0, language: Optional[int] = None,
                   task: str = "transcribe", words=None):
    """timing.py:112-183 at token level.  text_tokens: a list of ids (one window: the audio is 2-D or has B = 1) or a list of such lists (a batch; then
    `num_frames` may be a list and `words` is a list per item).  -> a list of `TokenTiming` (start / end: the first frame of the token's row and of the
    next row, over TOKENS_PER_SECOND), or of `WordTiming` when `words` is given; for a batch, a list of those.  No text tokens: []."""
    from .whisper import TOKENS_PER_SECOND

    batched = len(text_tokens) > 0 and isinstance(text_tokens[0], (list, tuple, np.ndarray))
    if not batched:
        if len(text_tokens) == 0:
            return []
        shape = tuple(mel_or_features.shape)
        if len(shape) == 2:
            mel_or_features = mel_or_features[None]
        elif len(shape) != 3 or shape[0] != 1:
            raise ValueError("one list of text tokens takes one window of audio")
        return find_alignment(model, [list(text_tokens)], mel_or_features, [int(num_frames)], medfilt_width=medfilt_width, qk_scale=qk_scale, language=language,
                              task=task, words=None if words is None else [words])[0]
    if words is not None and len(words) != len(text_tokens):
        raise ValueError("`words`: one list of token lists per item")
    res = []
    for b, al in enumerate(alignment_details(model, text_tokens, mel_or_features, num_frames, medfilt_width=medfilt_width, qk_scale=qk_scale, language=language,
                                             task=task)):
        if al is None:
            res.append([])
        elif words is not None:
            if [int(t) for w in words[b] for t in w] != al.tokens:
                raise ValueError("`words` must concatenate to text_tokens")
            res.append(word_timings(words[b], al.first_frames, al.probabilities))
        else:
            times = al.first_frames / TOKENS_PER_SECOND
            res.append([TokenTiming(t, float(times[i]), float(times[i + 1]), float(al.probabilities[i])) for i, t in enumerate(al.tokens)])
    return res
