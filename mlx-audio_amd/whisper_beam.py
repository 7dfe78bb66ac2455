"""Beam search on the Whisper text side: `beam_size` live prefixes per window, `patience`, and the temperature fallback with beam search as its
temperature-0 pass.  The reference carries the options and `Inference.rearrange_kv_cache` (mlx_audio/stt/models/whisper/decoding.py:82-116, 149-152) but
answers them with "Beam search decoder is not yet implemented"; the semantics here are those of OpenAI's BeamSearchDecoder, which the options were named for:

  per window K = beam_size live prefixes, a list `finished`, max_candidates = round(K * (patience or 1.0)).  A step filters every live row's logits as the
  greedy pick does and takes logprobs = l - logsumexp(l); every live row offers its K + 1 most probable tokens (equal ones by the lower id, never a masked
  one; at the first sampled position only row 0 of a window offers, its rows being one prefix), candidate (row j, token t) scoring sum_logprob[j] +
  logprob[j][t]; the window's candidates are walked by score descending, then row, then rank within the row: one ending in eot joins this step's newly
  finished, any other becomes the next free slot's prefix, until K are saved; the newly finished join `finished` while it holds fewer than max_candidates;
  the window is complete when it holds that many.  Slots left without a prefix are dead.  The loop ends when every window is complete, after sample_len
  steps, or when the text context is full.  Finalize: a window with fewer than K finished sequences takes its live prefixes in descending sum_logprob, each
  as if eot followed, until it has K; the candidates go to whisper_sampling.rank.

The step runs in libkokoro_hip.so with no host round trip: the grouped window state of whisper_sampling (K rows per window on ONE cross K/V slice), then
kk_op_whisper_beam_topk and kk_op_whisper_beam_select.  The self K/V is never moved: an owner table names the physical row that holds each position of a
beam, and the step's self-attention reads its keys through it.

`decode`, `verify_options`, `verify_sampling_options`, the batcher's `submit` and `Model.decode_with_fallback` keep refusing `beam_size`; beam search is reached
through the names of this module, the thin methods `Model.beam_search`, `Model.beam_candidates` and `Model.beam_decode_with_fallback`, and, in the running batch,
`WhisperBatcher.submit_beam` / `Model.beam_transcribe`.
"""
from __future__ import annotations

import math
from dataclasses import replace
from typing import Optional

from . import whisper_sampling
from .whisper_decoding import DecodingOptions, _features, window_loop, window_prologue
from .whisper_sampling import MAX_GROUP, SampledWindows, fallback_loop, results


def max_candidates(beam_size: int, patience: Optional[float]) -> int:
    return round(beam_size * (patience or 1.0))


def verify_beam_options(options: DecodingOptions) -> DecodingOptions:
    """_verify_options (decoding.py:465-478) word for word, then what beam search needs and what this build leaves out."""
    if options.beam_size is not None and options.best_of is not None:
        raise ValueError("beam_size and best_of can't be given together")
    if options.temperature == 0:
        if options.best_of is not None:
            raise ValueError("best_of with greedy sampling (T=0) is not compatible")
    if options.patience is not None and options.beam_size is None:
        raise ValueError("patience requires beam_size to be given")
    if options.length_penalty is not None and not (0 <= options.length_penalty <= 1):
        raise ValueError("length_penalty (alpha) should be a value between 0 and 1")
    k = options.beam_size
    if k is None:
        raise ValueError("beam search needs beam_size; without it call decode or sample")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_GROUP:
        raise ValueError(f"beam_size must be an integer in 1 .. {MAX_GROUP} (KK_WHISPER_MAX_GROUP)")
    p = options.patience
    if p is not None and (isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or not p > 0):
        raise ValueError("patience must be finite and > 0")
    if not 1 <= max_candidates(k, p) <= 2 * MAX_GROUP:
        raise ValueError(f"round(beam_size * patience) must be in 1 .. {2 * MAX_GROUP} finished sequences per window")
    if options.temperature != 0:
        raise ValueError("beam search runs at temperature 0; above it call sample")
    for name in ("prompt", "prefix"):
        v = getattr(options, name)
        if isinstance(v, str):
            raise ValueError(f"{name} must be a list of token ids: the tokenizer is not built")
    if isinstance(options.language, str):
        raise ValueError("language must be a language-token id or index: the tokenizer is not built")
    if options.task == "lang_id":
        raise ValueError("lang_id searches nothing: call decode")
    if options.task not in ("transcribe", "translate"):
        raise ValueError(f"unknown task {options.task!r}")
    return options


def finalize(finished, live, beam_size: int):
    """BeamSearchDecoder.finalize for one window: `finished` [(tokens, sum)] in the order they finished, `live` [(tokens, sum)] by slot.  A window with
    fewer than beam_size finished sequences takes its live prefixes in descending sum (equal sums by the lower slot), eot appended and the sum
    unchanged -- the tokens, cut at eot, are the prefix's -- until it has beam_size.  A dead slot (sum -inf) is no prefix."""
    out = [(list(t), float(s)) for t, s in finished]
    alive = [(list(t), float(s)) for t, s in live if s != -math.inf]
    for t, s in sorted(alive, key=lambda c: -c[1]):  # (stable: equal sums keep their slot order)
        if len(out) >= beam_size:
            break
        out.append((t, s))
    return out


def beam_candidates(model, mel_or_features, options: DecodingOptions = DecodingOptions(beam_size=5), eos_check_interval: int = 8, **kwargs) -> SampledWindows:
    """DecodingTask.run (decoding.py:618-707) up to the ranker with the beam search decoder: per window its finished sequences, topped up to `beam_size`
    from the live prefixes (`finalize`).  Language detection and no_speech_prob as in whisper_sampling.sample_candidates."""
    import torch

    if kwargs:
        options = replace(options, **kwargs)
    options = verify_beam_options(options)
    if eos_check_interval < 1:
        raise ValueError("eos_check_interval must be >= 1")
    rt, K = model._text, options.beam_size
    w = window_prologue(model, mel_or_features, options, K)
    with torch.cuda.device(model.device):
        no_speech = window_loop(model, w, options, K, eos_check_interval, lambda: rt.beam_setup(K, max_candidates(K, options.patience)),
                                lambda: rt.beam_not_complete() == 0)
        finished, live = rt.beam_read()
        no_speech = no_speech.cpu().numpy()
    cands = [finalize(finished[a], live[a], K) for a in range(w.feats.shape[0])]
    return SampledWindows(candidates=cands, languages=w.languages, language_probs=w.lang_probs, no_speech_probs=[float(p) for p in no_speech],
                          audio_features=w.feats, single=w.single, temperature=0.0)


def beam_search(model, mel_or_features, options: DecodingOptions = DecodingOptions(beam_size=5), eos_check_interval: int = 8, **kwargs):
    """`decode` with the beam search decoder: the DecodingResult (a list of them for a 3-D input) of the candidate the ranker prefers"""
    if kwargs:
        options = replace(options, **kwargs)
    return results(beam_candidates(model, mel_or_features, options, eos_check_interval=eos_check_interval), options.length_penalty)


def decode_with_fallback(model, mel_or_features, temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), beam_size: Optional[int] = 5, best_of: Optional[int] = 5,
                         logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6, seed: int = 0, **decode_options):
    """whisper_sampling.decode_with_fallback with OpenAI's pairing: at temperature 0 `beam_search` with `beam_size` (and `patience`, if given) and
    `best_of` dropped, above 0 `sample` with `best_of` and the beam options dropped; re-run windows keep their original indices as stream ids.
    beam_size None: the temperature-0 pass is greedy `decode`."""
    temperatures = [float(temperature)] if isinstance(temperature, (int, float)) else [float(t) for t in temperature]
    if not temperatures:
        raise ValueError("temperature must name at least one temperature")
    feats, single = _features(model, mel_or_features)  # encoded once, whatever the number of passes
    plain = {k: v for k, v in decode_options.items() if k != "patience"}

    def cold(idx):
        if beam_size is None:
            return model.decode(feats[idx], DecodingOptions(**plain))
        return beam_search(model, feats[idx], DecodingOptions(**decode_options, beam_size=beam_size))

    def sampled(idx, t):
        return whisper_sampling.sample(model, feats[idx], DecodingOptions(**plain, best_of=best_of, temperature=t), seed=seed, streams=idx)

    out = fallback_loop(feats.shape[0], temperatures, cold, sampled, logprob_threshold, no_speech_threshold)
    return out[0] if single else out
