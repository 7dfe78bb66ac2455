"""Sampling on the Whisper text side: decoding at temperature > 0 with `best_of` candidates per window, the maximum-likelihood ranker and
the temperature fallback of the reference's transcription loop, at token level.  Restates `GreedyDecoder` at temperature > 0, `MaximumLikelihoodRanker`
and `DecodingTask.run` (mlx_audio/stt/models/whisper/decoding.py:165-188, 250-283, 618-707) and `decode_with_fallback` (whisper.py:503-541).

The arithmetic runs in libkokoro_hip.so: the decoder forward of whisper_decoding.TextRuntime, the sampled pick (kk_op_whisper_pick_sampled: Gumbel-max
on Philox uniforms in the pass that takes the log-probability) and a state whose `best_of` rows per window read ONE cross K/V slice
(kk_whisper_text_set_audio_groups) where the reference repeats the audio features (decoding.py:641-655).

`decode`, `verify_options` and the batcher keep refusing a temperature: sampling is reached through the names of this module and the thin methods
`Model.sample`, `Model.sample_candidates` and `Model.decode_with_fallback`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .whisper_decoding import DecodingOptions, DecodingResult, _features, cut_at_eot, special_tokens, window_loop, window_prologue

MAX_GROUP = 8  # KK_WHISPER_MAX_GROUP


def verify_sampling_options(options: DecodingOptions) -> DecodingOptions:
    """_verify_options (decoding.py:465-478) word for word, then what sampling needs and what this build leaves out."""
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
    t = options.temperature
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or not t > 0:
        raise ValueError("sampling needs a finite temperature > 0; temperature 0 is greedy decoding: call decode")
    if options.best_of is not None and not 1 <= options.best_of <= MAX_GROUP:
        raise ValueError(f"best_of must be in 1 .. {MAX_GROUP} (KK_WHISPER_MAX_GROUP)")
    for name in ("prompt", "prefix"):
        v = getattr(options, name)
        if isinstance(v, str):
            raise ValueError(f"{name} must be a list of token ids: the tokenizer is not built")
    if isinstance(options.language, str):
        raise ValueError("language must be a language-token id or index: the tokenizer is not built")
    if options.task == "lang_id":
        raise ValueError("lang_id samples nothing: call decode")
    if options.task not in ("transcribe", "translate"):
        raise ValueError(f"unknown task {options.task!r}")
    return options


@dataclass
class SampledWindows:
    """What `sample_candidates` returns: per window, its `n_group` candidates (tokens cut at eot, sum_logprob) and what DecodingTask.run knows of it
    before the ranker (language-token id, language probabilities or None, no_speech_prob, its audio features)."""
    candidates: List[List[Tuple[List[int], float]]]
    languages: List[Optional[int]]
    language_probs: List[Optional[Dict[int, float]]]
    no_speech_probs: List[float]
    audio_features: object
    single: bool
    temperature: float


def _row_streams(streams, n_audio: int, n_group: int) -> np.ndarray:
    ids = list(range(n_audio)) if streams is None else [int(s) for s in streams]
    if len(ids) != n_audio:
        raise ValueError(f"streams must give one id per window ({n_audio})")
    rows = [s * n_group + g for s in ids for g in range(n_group)]  # a window sampled alone with its id draws what its rows of a batch draw
    if any(not 0 <= r <= 0xFFFFFFFF for r in rows):
        raise ValueError("a stream id times best_of must fit 32 bits")
    return np.asarray(rows, np.uint32)


def sample_candidates(model, mel_or_features, options: DecodingOptions = DecodingOptions(temperature=1.0), seed: int = 0, streams: Optional[Sequence[int]] = None,
                      eos_check_interval: int = 8, **kwargs) -> SampledWindows:
    """DecodingTask.run (decoding.py:618-707) up to the ranker at temperature > 0: `best_of or 1` sampled sequences per window.  `streams`: one id per
    window (default 0, 1, ...); row g of window a draws on the stream id streams[a] * n_group + g, so what a row samples depends on `seed`, its id and its
    own history -- not on the batch it runs in.  Language detection, where asked for, runs on the plain window state first; the grouped state then
    projects the windows' cross K/V once more."""
    import torch

    if kwargs:
        options = replace(options, **kwargs)
    options = verify_sampling_options(options)
    if eos_check_interval < 1:
        raise ValueError("eos_check_interval must be >= 1")
    rt = model._text
    n_group = options.best_of or 1
    w = window_prologue(model, mel_or_features, options, n_group)
    n_audio = w.feats.shape[0]
    ids = _row_streams(streams, n_audio, n_group)
    with torch.cuda.device(model.device):
        no_speech = window_loop(model, w, options, n_group, eos_check_interval, lambda: rt.sample_setup(options.temperature, seed, ids),
                                lambda: rt.not_ended() == 0)
        toks, rows = rt.read()
        no_speech = no_speech.cpu().numpy()
    eot = special_tokens(model.dims).eot
    cands = [[(cut_at_eot(toks[b, : rows[b].count], eot), float(rows[b].sum_logprob)) for b in range(a * n_group, (a + 1) * n_group)] for a in range(n_audio)]
    return SampledWindows(candidates=cands, languages=w.languages, language_probs=w.lang_probs, no_speech_probs=[float(p) for p in no_speech],
                          audio_features=w.feats, single=w.single, temperature=float(options.temperature))


def rank(candidates: Sequence[Tuple[Sequence[int], float]], length_penalty: Optional[float]) -> int:
    """MaximumLikelihoodRanker.rank (decoding.py:165-188) for one window: the index of the candidate with the highest sum_logprob / penalty, the lowest
    index on ties; penalty = length (None) or ((5 + length) / 6) ** length_penalty (the Google NMT paper's).  One departure: under `None` a candidate of
    length 0 scores -inf, where the reference divides by zero."""
    best, best_score = 0, None
    for i, (tokens, logprob) in enumerate(candidates):
        length = len(tokens)
        if length_penalty is None:
            score = -math.inf if length == 0 else logprob / length
        else:
            score = logprob / ((5 + length) / 6) ** length_penalty
        if best_score is None or score > best_score:
            best, best_score = i, score
    return best


def results(windows: SampledWindows, length_penalty: Optional[float]):
    """the ranked candidate of every window as a DecodingResult (decoding.py:680-707): avg_logprob = sum / (len + 1); text "" and compression_ratio nan"""
    out = []
    for a, group in enumerate(windows.candidates):
        seq, total = group[rank(group, length_penalty)]
        out.append(DecodingResult(audio_features=windows.audio_features[a], language=windows.languages[a], language_probs=windows.language_probs[a], tokens=list(seq),
                                  avg_logprob=total / (len(seq) + 1), no_speech_prob=windows.no_speech_probs[a], temperature=windows.temperature))
    return out[0] if windows.single else out


def sample(model, mel_or_features, options: DecodingOptions = DecodingOptions(temperature=1.0), seed: int = 0, streams: Optional[Sequence[int]] = None,
           eos_check_interval: int = 8, **kwargs):
    """`decode` at temperature > 0: the DecodingResult (a list of them for a 3-D input) of the candidate the ranker prefers among `best_of or 1` samples"""
    if kwargs:
        options = replace(options, **kwargs)
    return results(sample_candidates(model, mel_or_features, options, seed=seed, streams=streams, eos_check_interval=eos_check_interval), options.length_penalty)


def fallback_loop(n: int, temperatures: Sequence[float], greedy: Callable[[List[int]], list], sampled: Callable[[List[int], float], list],
                  logprob_threshold: Optional[float], no_speech_threshold: Optional[float]) -> list:
    """whisper.py:503-541 for n windows at once.  Every window runs at the first temperature; those whose result needs fallback run TOGETHER at the next.
    `greedy(indices)` and `sampled(indices, t)` return one result per listed window (original indices).  A window keeps the result of the last
    temperature it ran at.  needs fallback: avg_logprob below logprob_threshold, unless no_speech_prob is above no_speech_threshold (silence)."""
    out: list = [None] * n
    todo = list(range(n))
    for t in temperatures:
        if not todo:
            break
        res = greedy(todo) if t == 0 else sampled(todo, t)
        if len(res) != len(todo):
            raise RuntimeError("a decoding pass returned another number of results than windows")
        again = []
        for i, r in zip(todo, res):
            out[i] = r
            needs_fallback = logprob_threshold is not None and r.avg_logprob < logprob_threshold
            if no_speech_threshold is not None and r.no_speech_prob > no_speech_threshold:
                needs_fallback = False  # silence
            if needs_fallback:
                again.append(i)
        todo = again
    return out


def decode_with_fallback(model, mel_or_features, temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), logprob_threshold: Optional[float] = -1.0,
                         no_speech_threshold: Optional[float] = 0.6, seed: int = 0, **decode_options):
    """decode_with_fallback of the reference's transcription loop (whisper.py:503-541) for a batch of windows: decode at the first temperature, and again
    at the next for the windows whose average log-probability is too low, until one passes or the temperatures run out.  At 0 `model.decode` runs with
    `best_of` dropped, above 0 `sample` with `beam_size` / `patience` dropped; re-run windows keep their original indices as stream ids.  There is no
    `compression_ratio_threshold`: without a tokenizer `compression_ratio` is nan and that check could never fire."""
    temperatures = [float(temperature)] if isinstance(temperature, (int, float)) else [float(t) for t in temperature]
    if not temperatures:
        raise ValueError("temperature must name at least one temperature")
    feats, single = _features(model, mel_or_features)  # encoded once, whatever the number of passes

    def greedy(idx):
        kw = {k: v for k, v in decode_options.items() if k != "best_of"}
        return model.decode(feats[idx], DecodingOptions(**kw))

    def sampled(idx, t):
        kw = {k: v for k, v in decode_options.items() if k not in ("beam_size", "patience")}
        return sample(model, feats[idx], DecodingOptions(**kw, temperature=t), seed=seed, streams=idx)

    out = fallback_loop(feats.shape[0], temperatures, greedy, sampled, logprob_threshold, no_speech_threshold)
    return out[0] if single else out
