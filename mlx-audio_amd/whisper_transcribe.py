"""Long-form transcription: the loop of the reference's `Model.generate` (mlx_audio/stt/models/whisper/whisper.py:437-866) as
`Model.transcribe`, for one recording or for many at once on ONE running decoder batch.

Three layers:
  * `FileState` -- the reference's loop for ONE file as a state machine with no torch and no device in it.  `next_window()` asks for one window
    (`seek`, `size`, the prompt tokens, the index into the temperatures); `feed(result)` takes that window's `DecodingResult` and either asks for the same
    window at the next temperature (the fallback of whisper.py:503-541) or cuts the result into segments and moves `seek` on (:601-846).  What it
    restates: `clip_timestamps`, `segment_size`, the fallback on compression ratio and log-probability with the no-speech override, the no-speech skip
    and its log-probability exception, the three segmentation cases, the seek advance, the clearing of instantaneous or blank segments, `all_tokens` and
    `prompt_reset_since`.  A window that does not move `seek` forward raises RuntimeError -- the reference would loop forever there.
  * `drive` -- the scheduler over many FileStates behind a small backend seam (a fake backend tests it without a GPU).  A round collects every file
    whose state machine has a window ready, has the NEW windows cut and encoded together, and submits one request per file; a file has at most one
    window in flight, and at most `max_rows` files are in flight at all.
  * `transcribe` -- the backend on the device: one log-mel per file (padding = W * HOP_LENGTH samples, kept on the device), ONE kk_op_mel_windows launch
    and ONE `embed_audio` call per round for the windows that became ready in it, and a `WhisperBatcher` whose rows decode greedily (`submit`) or sample
    (`submit_sampled`, stream id `(seek * 16 + temperature index) & 0xFFFFFFFF`) side by side in one pick launch.

The contract: a file's `TranscribeResult` equals (==) that of `transcribe` on the file alone, whatever is transcribed with it, and equals the
reference's loop driven by `model.decode` / `model.sample` per window on `embed_audio` of that window alone with the same seed and stream ids.

W = 2 * n_audio_ctx stands where the reference writes N_FRAMES (3000 for every real checkpoint).  What is taken over as it is: the loop keeps ONE
`seek` across the clips of `clip_timestamps` and never moves it up to a later clip's start (whisper.py:543-584), so a clip that starts behind the
previous clip's end begins where that one stopped.  `beam_transcribe` is the same loop with OpenAI's pairing: a window at temperature 0 is
searched with a beam (`WhisperBatcher.submit_beam`), one above it sampled `best_of` times (`submit_group`); `transcribe` itself keeps refusing `beam_size`
and `best_of` > 1.  Not built: `word_timestamps`, `hallucination_silence_threshold`, text prompts (`initial_prompt` is a list of token ids), a vocabulary
file (the caller names theirs: `tokenizer=`)."""
from __future__ import annotations

import zlib
from collections import deque
from dataclasses import dataclass, field, replace
from typing import Deque, Dict, List, Optional, Sequence, Tuple, Union

SAMPLE_RATE = 16000
HOP_LENGTH = 160
FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH
MAX_TEMPERATURES = 16  # the stream id of a sampled window keeps the temperature's index in its low four bits


def compression_ratio(text: str) -> float:
    """decoding.py:15-17"""
    text_bytes = text.encode("utf-8")
    return len(text_bytes) / len(zlib.compress(text_bytes))


@dataclass(frozen=True)
class WindowRequest:
    seek: int                    # the window's first frame in the file's spectrogram
    size: int                    # frames of content; the window is these, then zeros up to W
    prompt: Tuple[int, ...]      # all_tokens[prompt_reset_since:]
    temperature_index: int
    temperature: float

    @property
    def stream(self) -> int:
        """the stream id a sampled pass of this window draws on"""
        return (self.seek * 16 + self.temperature_index) & 0xFFFFFFFF


@dataclass
class TranscribeResult:
    """`text` is None without a tokenizer; `language` is the language-token id (None for an English-only model); `tokens`: every segment's tokens in
    order (the initial prompt left out).  A segment: id, seek, start, end, text (None without a tokenizer), tokens, temperature, avg_logprob,
    compression_ratio (None without a tokenizer), no_speech_prob."""
    text: Optional[str]
    segments: List[dict] = field(default_factory=list)
    language: Optional[int] = None
    tokens: List[int] = field(default_factory=list)


def parse_clip_timestamps(clip_timestamps: Union[str, Sequence[float]], content_frames: int) -> List[Tuple[int, int]]:
    """whisper.py:480-496: seconds (a comma-separated string or a list) -> (start, end) frame pairs; an odd count ends at the content's end, an even
    count has its LAST end clamped to it"""
    if isinstance(clip_timestamps, str):
        clip_timestamps = [float(ts) for ts in (clip_timestamps.split(",") if clip_timestamps else [])]
    seek_points = [round(ts * FRAMES_PER_SECOND) for ts in clip_timestamps]
    if len(seek_points) == 0:
        seek_points.append(0)
    if len(seek_points) % 2 == 1:
        seek_points.append(content_frames)
    else:
        seek_points[-1] = min(content_frames, seek_points[-1])
    return list(zip(seek_points[::2], seek_points[1::2]))


def check_temperatures(temperature) -> Tuple[float, ...]:
    temps = (float(temperature),) if isinstance(temperature, (int, float)) else tuple(float(t) for t in temperature)
    if not temps:
        raise ValueError("temperature must name at least one temperature")
    if len(temps) > MAX_TEMPERATURES:
        raise ValueError(f"at most {MAX_TEMPERATURES} temperatures (a sampled window's stream id keeps the index in four bits)")
    if any(not (t >= 0.0) or t == float("inf") for t in temps):
        raise ValueError("temperatures must be finite and >= 0")
    return temps


class FileState:
    """The reference's loop for one file.  content_frames: the file's frames without the padding; W: frames of a window (2 * n_audio_ctx);
    n_audio_ctx, timestamp_begin, eot: the model's.  The tokenizer is anything with `decode(ids) -> str` (whisper_tokenizer.Tokenizer), or None."""

    def __init__(self, content_frames: int, *, W: int, n_audio_ctx: int, timestamp_begin: int, eot: int, temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                 compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                 condition_on_previous_text: bool = True, initial_prompt: Optional[Sequence[int]] = None, clip_timestamps: Union[str, Sequence[float]] = "0",
                 tokenizer=None):
        if tokenizer is None and compression_ratio_threshold is not None:
            raise ValueError("compression_ratio_threshold needs the text of a window, and there is no tokenizer to make it: pass tokenizer=, or "
                             "compression_ratio_threshold=None")
        if isinstance(initial_prompt, str):
            raise ValueError("initial_prompt must be a list of token ids: text-to-id encoding is not built")
        self.content_frames, self.W, self.timestamp_begin, self.eot = int(content_frames), int(W), int(timestamp_begin), int(eot)
        self.temperatures = check_temperatures(temperature)
        self.compression_ratio_threshold, self.logprob_threshold, self.no_speech_threshold = compression_ratio_threshold, logprob_threshold, no_speech_threshold
        self.condition_on_previous_text, self.tokenizer = condition_on_previous_text, tokenizer
        self.input_stride = self.W // int(n_audio_ctx)  # mel frames per output token: 2
        self.time_precision = self.input_stride * HOP_LENGTH / SAMPLE_RATE  # time per output token: 0.02 (seconds)
        self.clips = parse_clip_timestamps(clip_timestamps, self.content_frames)
        self.clip_idx = 0
        self.seek = self.clips[0][0]
        self.initial_prompt_tokens = [int(t) for t in (initial_prompt or [])]
        self.all_tokens: List[int] = list(self.initial_prompt_tokens)
        self.all_segments: List[dict] = []
        self.prompt_reset_since = 0
        self._pending: Optional[WindowRequest] = None
        self.windows = 0  # decoding passes asked for so far

    # ---- asking -----------------------------------------------------------------------------------------------------------------------------
    def next_window(self) -> Optional[WindowRequest]:
        """the window to decode next (the same object until it was fed), or None when the file is done"""
        if self._pending is not None:
            return self._pending
        while self.clip_idx < len(self.clips) and not self.seek < self.clips[self.clip_idx][1]:
            self.clip_idx += 1
        if self.clip_idx == len(self.clips):
            return None
        size = min(self.W, self.content_frames - self.seek, self.clips[self.clip_idx][1] - self.seek)
        if size <= 0:
            raise RuntimeError(f"transcription stalled: the window at frame {self.seek} holds no content ({self.content_frames} frames, clip "
                               f"{self.clips[self.clip_idx]})")
        self._pending = WindowRequest(self.seek, size, tuple(self.all_tokens[self.prompt_reset_since:]), 0, self.temperatures[0])
        self.windows += 1
        return self._pending

    # ---- feeding ----------------------------------------------------------------------------------------------------------------------------
    def feed(self, result) -> None:
        """the DecodingResult of the pending window at its temperature"""
        req = self._pending
        if req is None:
            raise RuntimeError("feed without a pending window")
        if self.tokenizer is not None:  # decoding.py:675, 702
            text = self.tokenizer.decode(result.tokens).strip()
            result = replace(result, text=text, compression_ratio=compression_ratio(text))
        # decode_with_fallback (whisper.py:522-539)
        needs_fallback = False
        if self.compression_ratio_threshold is not None and result.compression_ratio > self.compression_ratio_threshold:
            needs_fallback = True  # too repetitive
        if self.logprob_threshold is not None and result.avg_logprob < self.logprob_threshold:
            needs_fallback = True  # average log probability is too low
        if self.no_speech_threshold is not None and result.no_speech_prob > self.no_speech_threshold:
            needs_fallback = False  # silence
        if needs_fallback and req.temperature_index + 1 < len(self.temperatures):
            i = req.temperature_index + 1
            self._pending = replace(req, temperature_index=i, temperature=self.temperatures[i])
            self.windows += 1
            return
        self._pending = None
        self._consume(req, result)

    def _segment(self, req: WindowRequest, start: float, end: float, tokens: List[int], result) -> dict:
        text = None if self.tokenizer is None else self.tokenizer.decode([t for t in tokens if t < self.eot])
        return {"seek": req.seek, "start": start, "end": end, "text": text, "tokens": list(tokens), "temperature": result.temperature,
                "avg_logprob": result.avg_logprob, "compression_ratio": None if self.tokenizer is None else result.compression_ratio,
                "no_speech_prob": result.no_speech_prob}

    def _consume(self, req: WindowRequest, result) -> None:
        tb, seek, size = self.timestamp_begin, req.seek, req.size
        tokens = [int(t) for t in result.tokens]
        if self.no_speech_threshold is not None:  # no voice activity check (:603-615)
            should_skip = result.no_speech_prob > self.no_speech_threshold
            if self.logprob_threshold is not None and result.avg_logprob > self.logprob_threshold:
                should_skip = False  # don't skip if the logprob is high enough, despite the no_speech_prob
            if should_skip:
                self.seek = seek + size  # fast-forward to the next segment boundary
                return
        time_offset = float(seek * HOP_LENGTH / SAMPLE_RATE)
        segment_duration = size * HOP_LENGTH / SAMPLE_RATE
        current: List[dict] = []
        is_ts = [t >= tb for t in tokens]
        single_timestamp_ending = is_ts[-2:] == [False, True]
        consecutive = [i + 1 for i in range(len(tokens) - 1) if is_ts[i] and is_ts[i + 1]]
        if consecutive:  # the output contains two consecutive timestamp tokens
            slices = list(consecutive)
            if single_timestamp_ending:
                slices.append(len(tokens))
            last_slice = 0
            for current_slice in slices:
                sliced = tokens[last_slice:current_slice]
                current.append(self._segment(req, time_offset + (sliced[0] - tb) * self.time_precision, time_offset + (sliced[-1] - tb) * self.time_precision,
                                             sliced, result))
                last_slice = current_slice
            if single_timestamp_ending:  # no speech after the last timestamp
                new_seek = seek + size
            else:  # ignore the unfinished segment and seek to the last timestamp
                new_seek = seek + (tokens[last_slice - 1] - tb) * self.input_stride
        else:
            duration = segment_duration
            timestamps = [t for t in tokens if t >= tb]
            if timestamps and timestamps[-1] != tb:  # no consecutive timestamps but it has a timestamp; use the last one
                duration = (timestamps[-1] - tb) * self.time_precision
            current.append(self._segment(req, time_offset, time_offset + duration, tokens, result))
            new_seek = seek + size
        if new_seek <= seek:
            raise RuntimeError(f"transcription stalled: the window at frame {seek} ended on the timestamp {tokens[-1] - tb if tokens else None} and would "
                               "be decoded again for ever")
        self.seek = new_seek
        for segment in current:  # if a segment is instantaneous or does not contain text, clear it
            if segment["start"] == segment["end"] or (self.tokenizer is not None and segment["text"].strip() == ""):
                segment["text"] = None if self.tokenizer is None else ""
                segment["tokens"] = []
        self.all_segments.extend({"id": i, **segment} for i, segment in enumerate(current, start=len(self.all_segments)))
        self.all_tokens.extend(token for segment in current for token in segment["tokens"])
        if not self.condition_on_previous_text or result.temperature > 0.5:
            self.prompt_reset_since = len(self.all_tokens)  # do not feed the prompt tokens if a high temperature was used

    def result(self, language: Optional[int]) -> TranscribeResult:
        tokens = self.all_tokens[len(self.initial_prompt_tokens):]
        return TranscribeResult(text=None if self.tokenizer is None else self.tokenizer.decode(tokens), segments=self.all_segments, language=language,
                                tokens=list(tokens))


# ---- the scheduler over many files ---------------------------------------------------------------------------------------------------------
def drive(states: Sequence[FileState], backend, max_rows: int) -> None:
    """Run every state machine to its end.  backend:
         encode(batch) -- batch: [(file index, seek, size)] of this round's NEW windows (1 .. max_rows of them) -> their windows' audio features, in order;
         submit(file index, features, request) -> a Future of the request's DecodingResult;
         step() -- one round of whatever decodes (the futures of finished requests are settled when it returns).
    A file whose window is asked for again at the next temperature keeps its features: they are encoded once."""
    if max_rows < 1:
        raise ValueError("max_rows must be >= 1")
    ready: Deque[int] = deque(range(len(states)))
    flying: Dict[int, object] = {}
    kept: Dict[int, tuple] = {}  # file -> (seek, size, features) of its last window
    while ready or flying:
        batch = []
        while ready and len(flying) + len(batch) < max_rows:
            i = ready.popleft()
            req = states[i].next_window()
            if req is None:
                kept.pop(i, None)
                continue
            batch.append((i, req))
        new = [(i, r.seek, r.size) for i, r in batch if kept.get(i, (None, None))[:2] != (r.seek, r.size)]
        if new:
            feats = backend.encode(new)
            if len(feats) != len(new):
                raise RuntimeError("the encoder returned another number of windows than it was given")
            for (i, seek, size), f in zip(new, feats):
                kept[i] = (seek, size, f)
        for i, r in batch:
            flying[i] = backend.submit(i, kept[i][2], r)
        if not flying:
            continue
        backend.step()
        for i in [i for i, f in flying.items() if f.done()]:
            states[i].feed(flying.pop(i).result())
            ready.append(i)


# ---- on the device ----------------------------------------------------------------------------------------------------------------------------
class _DeviceBackend:
    def __init__(self, model, batcher, mels, languages, seed: int, decode_options: dict, beam: Optional[dict] = None):
        self.model, self.batcher, self.mels, self.languages, self.seed, self.options = model, batcher, mels, languages, seed, decode_options
        self.W = 2 * model.dims.n_audio_ctx
        self.beam = beam  # beam_transcribe: dict(beam_size, best_of, patience); None: transcribe

    def encode(self, batch):
        from .whisper import mel_windows

        w = mel_windows([self.mels[i] for i, _, _ in batch], [s for _, s, _ in batch], [n for _, _, n in batch], self.W)
        feats = self.model.embed_audio(w)  # ONE encoder call for the round's windows; a row has the bits of its B = 1 call
        return [feats[r] for r in range(len(batch))]

    def submit(self, i: int, features, req: WindowRequest):
        from .whisper_decoding import DecodingOptions

        # (an English-only vocabulary has no language token: the options' language is never written into its sot sequence, 0 only passes the checks)
        kw = dict(self.options, language=0 if self.languages[i] is None else self.languages[i], prompt=list(req.prompt))
        kw.pop("best_of", None)
        if self.beam is not None:
            return submit_window(self.batcher, features, req, kw, self.seed, **self.beam)
        if req.temperature > 0:
            return self.batcher.submit_sampled(features, DecodingOptions(**kw, temperature=req.temperature), seed=self.seed, stream=req.stream)
        return self.batcher.submit(features, DecodingOptions(**kw, temperature=0.0))

    def step(self):
        self.batcher.step()


def group_stream(req: WindowRequest) -> int:
    """the stream id of a window's best_of group: row g draws on group_stream * best_of + g, which fits 32 bits for best_of <= 8 (KK_WHISPER_MAX_GROUP)"""
    return (req.seek * 16 + req.temperature_index) % 2 ** 28


def submit_window(batcher, features, req: WindowRequest, kw: dict, seed: int, beam_size: Optional[int], best_of: Optional[int], patience: Optional[float]):
    """beam_transcribe's routing of one window (OpenAI's pairing, as whisper_beam.decode_with_fallback's): at temperature 0 the beam search (greedy
    `submit` when beam_size is None), above it `best_of` samples on the group's stream id (`submit_sampled` on it when best_of is None or 1)"""
    from .whisper_decoding import DecodingOptions

    if req.temperature > 0:
        if best_of in (None, 1):
            return batcher.submit_sampled(features, DecodingOptions(**kw, temperature=req.temperature), seed=seed, stream=group_stream(req))
        return batcher.submit_group(features, DecodingOptions(**kw, temperature=req.temperature, best_of=best_of), seed=seed, stream=group_stream(req))
    if beam_size is None:
        return batcher.submit(features, DecodingOptions(**kw, temperature=0.0))
    return batcher.submit_beam(features, DecodingOptions(**kw, temperature=0.0, beam_size=beam_size, patience=patience))


def check_transcribe_options(decode_options: dict, word_timestamps=False, hallucination_silence_threshold=None, beam: bool = False) -> None:
    if word_timestamps:
        raise NotImplementedError("word_timestamps is not built in transcribe (find_alignment gives token timestamps for one window)")
    if hallucination_silence_threshold is not None:
        raise NotImplementedError("hallucination_silence_threshold needs word_timestamps, which transcribe does not build")
    if not beam and (decode_options.get("beam_size") is not None or decode_options.get("patience") is not None):
        raise NotImplementedError("beam search is not built in transcribe: the batcher's rows decode greedily or sample (Model.beam_search runs one window)")
    if not beam and decode_options.get("best_of") not in (None, 1):
        raise NotImplementedError("best_of > 1 is not built in transcribe: the batcher has no candidate groups (Model.sample runs them for one window)")
    if decode_options.get("task", "transcribe") not in ("transcribe", "translate"):
        raise ValueError(f"transcribe takes task 'transcribe' or 'translate', not {decode_options.get('task')!r}")
    if "prompt" in decode_options:
        raise ValueError("prompt is the loop's own (a window's prompt is its file's previous text): give the first one as `initial_prompt`")


def transcribe(model, audio, *, temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold: Optional[float] = 2.4,
               logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
               initial_prompt: Optional[Sequence[int]] = None, clip_timestamps: Union[str, Sequence[float]] = "0", tokenizer=None, seed: int = 0, max_rows: int = 8,
               word_timestamps: bool = False, hallucination_silence_threshold: Optional[float] = None, _beam: Optional[dict] = None, **decode_options):
    """whisper.py:355-866 for one recording (1-D samples at 16 kHz: numpy or torch) -> TranscribeResult, or for a list of them -> a list, all on one
    decoder batch of `max_rows` rows.  tokenizer: a whisper_tokenizer.Tokenizer, or the path of a tiktoken-format rank file, or None (then every `text`
    is None and `compression_ratio_threshold` must be None).  decode_options: DecodingOptions fields (language, task, sample_len, suppress_tokens, ...)."""
    from .whisper import HOP_LENGTH as HOP, log_mel_spectrogram
    from .whisper_decoding import NOT_BUILT, DecodingOptions, language_token, special_tokens
    from .whisper_serve import WhisperBatcher

    if getattr(model, "_text", None) is None:
        raise NotImplementedError(NOT_BUILT)
    decode_options = dict(decode_options)
    decode_options.pop("max_tokens", None)  # (whisper.py:437-438)
    decode_options.pop("generation_stream", None)
    check_transcribe_options(decode_options, word_timestamps, hallucination_silence_threshold, beam=_beam is not None)
    DecodingOptions(**decode_options)  # an unknown name is a TypeError here, before anything runs
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError("seed must be an int")
    d = model.dims
    tok = special_tokens(d)
    W = 2 * d.n_audio_ctx
    single = not isinstance(audio, (list, tuple))
    clips = [audio] if single else list(audio)
    if isinstance(tokenizer, (str, bytes)) or hasattr(tokenizer, "__fspath__"):
        from .whisper_tokenizer import Tokenizer

        tokenizer = Tokenizer.from_file(tokenizer, d)
    kw = dict(W=W, n_audio_ctx=d.n_audio_ctx, timestamp_begin=tok.timestamp_begin, eot=tok.eot, temperature=temperature,
              compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold,
              condition_on_previous_text=condition_on_previous_text, initial_prompt=initial_prompt, clip_timestamps=clip_timestamps, tokenizer=tokenizer)
    FileState(0, **kw)  # the argument checks, before anything runs
    if not clips:
        return []
    language = decode_options.get("language")
    if language is not None and tok.multilingual:
        language = language_token(tok, language)
    mels = [log_mel_spectrogram(a, n_mels=d.n_mels, padding=W * HOP, device=str(model.device)) for a in clips]  # each file once; they stay on the device
    states = [FileState(int(m.shape[0]) - W, **kw) for m in mels]
    languages: List[Optional[int]] = [language if tok.multilingual else None] * len(clips)
    if getattr(model, "_server", None) is not None and not model._server.closed:
        raise RuntimeError("this model's WhisperBatcher is still open: close() it first")
    batcher = model._server = WhisperBatcher(model, max_rows=max_rows)
    try:
        if tok.multilingual and language is None:  # whisper.py:454-465: the first W frames of every file, as lang_id requests of the same batch
            futs = [batcher.submit(m[:W], DecodingOptions(task="lang_id")) for m in mels]
            batcher.run_until_idle()
            languages = [f.result().language for f in futs]
        # (beam_transcribe: max_rows files in flight may wait for each other's rows; the batcher queues them in order)
        drive(states, _DeviceBackend(model, batcher, mels, languages, seed, decode_options, _beam), max_rows)
    finally:
        batcher.close()
    out = [s.result(l) for s, l in zip(states, languages)]
    return out[0] if single else out


def beam_transcribe(model, audio, *, beam_size: Optional[int] = 5, best_of: Optional[int] = 5, patience: Optional[float] = None, **kw):
    """`transcribe` with OpenAI's transcription defaults: a window at temperature 0 is searched with a beam of `beam_size`
    (`WhisperBatcher.submit_beam`; greedy `submit` when beam_size is None), a window above it is sampled `best_of` times and ranked (`submit_group` on the
    stream id `(seek * 16 + temperature index) % 2 ** 28`; `submit_sampled` on the same id when best_of is None or 1).  Every other argument is
    transcribe's, and so are the loop, the files' state machines and the contract: a file's result equals that of the file alone.  max_rows must hold
    the larger of the two group sizes."""
    from .whisper_beam import max_candidates, verify_beam_options
    from .whisper_decoding import DecodingOptions
    from .whisper_sampling import MAX_GROUP

    if beam_size is not None:
        verify_beam_options(DecodingOptions(beam_size=beam_size, patience=patience))
        if max_candidates(beam_size, patience) < beam_size:
            raise ValueError("round(beam_size * patience) must be at least beam_size in the batcher (WhisperBatcher.submit_beam)")
    elif patience is not None:
        raise ValueError("patience requires beam_size to be given")
    if best_of is not None and (isinstance(best_of, bool) or not isinstance(best_of, int) or not 1 <= best_of <= MAX_GROUP):
        raise ValueError(f"best_of must be in 1 .. {MAX_GROUP} (KK_WHISPER_MAX_GROUP)")
    need = max(beam_size or 1, best_of or 1)
    if kw.get("max_rows", 8) < need:
        raise ValueError(f"max_rows = {kw.get('max_rows', 8)} cannot hold a group of {need} rows")
    return transcribe(model, audio, _beam=dict(beam_size=beam_size, best_of=best_of, patience=patience), **kw)
