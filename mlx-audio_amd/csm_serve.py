"""Continuous batching for CSM: independent requests enter and leave ONE running batch on one copy of the weights.

`generate_batch` is static: B prompts start together and all B rows are stepped until the last stream ends.  `CSMBatcher` keeps a batch of
`max_batch` cache rows running instead.  A finished stream's row is PARKED (kk_csm_park_row: it sees no key and appends nothing) and handed
to the next queued request, whose prompt is written right-aligned below the shared cache position (kk_csm_admit) while the other rows keep
their state; when the position reaches the end of the cache every live window is moved down (kk_csm_shift_caches), and up when a prompt is
longer than the position.  A stream's codes and waveform are, bit for bit, those of `Model.generate_batch([prompt], seed=...)` alone:
  * rng "host": one `np.random.default_rng(seed)` per stream, one [n_cb] draw per frame, stacked per frame over the rows;
  * rng "device": the sampling kernels draw from Philox on (the batcher's seed, the stream's id, the stream's own position, code book).

One scheduling round (`step`): poll the EOS flags (one sync every `eos_check_interval` frames, as generate_batch does), park finished rows
and decode them (streams of equal length in one Mimi.decode call), admit queued requests FIFO into parked rows, shift if needed, then one
frame for all rows through the captured single-token graph.  An admission stalls the other rows for one prompt block and one B = 1 frame.

A voice service's requests share most of their prompt: the speaker's reference segment.  `submit(prefix=vp, text=...)` (vp from
`Model.voice_prefix(context)`) admits a request on top of the prefix's K / V, which are copied under the request's own text frames instead of being
computed again (kk_csm_admit_prefixed): no Mimi.encode and no context tokenisation per request, a prompt block of the text frames
only, the same bits.  Requests with and without a prefix mix freely in one batch.

Audio while a stream runs: `CSMBatcher(..., stream_chunk_frames=N)` and `submit_stream(...)`.  The codec follows the batch in
a row-mode streaming decoder (`Mimi.row_decoder`: one position and one lifetime per row, the decoder row is the cache row), and a request's
audio arrives in chunks of N frames -- chunk k is its frames [kN, (k+1)N), the last one the remainder -- whose concatenation is, bit for
bit, a batch-1 `Mimi.decode_step` stream over its codes in steps of N, ..., r.  A chunk is decoded only after an EOS poll has confirmed its
frames (polls run every N frames then), so nothing at or after a stream's EOS frame or past its frame limit is ever emitted.  Ready chunks
are decoded in one aligned round per poll: all rows with a full chunk in one `step(F=N)`, tails grouped by equal r.  `submit` is unchanged
(one offline `Mimi.decode` at the end) and mixes with `submit_stream` in one batch.

A sampler per request: `CSMBatcher(..., row_samplers=True)` and `submit(..., sampler=, seed=)`.  The frame step then reads every
row's settings from a device table (`SesameModel.set_row_sampler`, written at admission) instead of launch arguments: a greedy request, one at
temp 0.7 / top_p 0.9 and one with a seed of its own run in ONE batch, in the same launches per frame and one captured graph whatever the mix.
Each request still carries the bits of its own `generate_batch([prompt], sampler=its own, seed=its own)`.

A conversation: `sess = batcher.session(context)` and `submit(session=sess, text=...)`.  When a session's turn ends, the K / V of
its prompt and of the frames it kept are copied out of the row before it is parked (kk_csm_prefix_capture); the next turn is admitted on top of
that copy and computes only what is new: the frames the cache did not hold yet, the EOS frame, what the session has heard since
(`sess.hear(segment)`) and the turn's text.  No earlier answer is encoded by Mimi again and no earlier position is computed again.  A session's
turns are, bit for bit, those of the same session run alone, whatever else the batch runs.

Admissions off the batch's stream: `CSMBatcher(..., overlap_admission=True, prefill_lanes=1)`.  The head of the queue is prefilled
in a LANE -- a `share()` generator with one cache row -- on a side stream while the batch keeps stepping: the same `admit` / `admit(prefix=)`
calls, so the same first frame and K / V.  When a row is free and the lane's event has completed, the request is COMMITTED: one copy launch
moves the lane's window into the row (kk_csm_admit_transfer), which is all the batch's stream pays for the admission.  FIFO order is kept, and
every request still carries the bits of its own `generate_batch([prompt])` run.

Stopping: `cancel(handle)` and `interrupt(handle, played_frames=)` (also on a `CSMAudioStream` and a `CSMSession`).  A caller's thread
only records the wish; the scheduler applies it at the top of its next round.  A cancelled request leaves the queue, its lane or its row at once
and never happened: `CancelledError` for whoever waits, the session as it was.  An interrupted stream ends NOW with the k frames that were heard:
its limit is lowered to k and the EOS flags are polled, so its result, its last chunk and -- for a session's turn -- the K / V the next turn
is conditioned on are those of a turn of k frames.  The other rows see a park and a poll, neither of which they can tell from any other.

Listening: `CSMBatcher(..., listen_rows=K)` and `batcher.listen()` / `sess.listen(speaker)` (DESIGN 8d-9 ... 8d-13): microphones at any sample
rate and in any PCM format, with endpointing and barge-in, one-shot or always open.  That edge touches no cache row and lives in csm_listen.py
and csm_continuous.py; this module calls `_listen_init`, `_listen_consume`, `_listen_round`, `_listen_due` and `_listen_close` and re-exports its names.
With `stt=` (a `whisper_serve.WhisperBatcher`) a listener made with `transcribe=` has its utterance transcribed: `_stt_init`, and `_stt_round`
behind the listen round, which also steps `stt`; its work counts as due work (`_stt_has_work`).

Audio out at other rates and in PCM formats: `submit(..., sample_rate=R, format="s16le")` / `submit_stream(...)` (`pcm.FORMATS`).
Every chunk passes through the cache row's resampler row (`resample.RowResampler`), the last one flushes, and the chunks concatenate, bit for
bit, to `resample(a, model rate, R)` of the audio `a` the request yields without a rate.  With a format the request gets `int16` / `uint8` device
tensors, encoded in that resampler step or, at the model's rate, by one convert launch (`pcm.RowConverter`) for the round's rows: they concatenate,
element for element, to `pcm.encode` of that audio; `played_samples` stays in samples.  Without either no resampler or converter is made."""
from __future__ import annotations

import queue
import threading
import time
from collections import deque
from concurrent.futures import CancelledError, Future
from dataclasses import dataclass, field
from typing import Deque, Dict, List, Optional, Sequence

import weakref

import numpy as np
import torch

from . import pcm as PCM
from . import resample as RS
from . import ring as RING
from . import vad as VAD
from .csm_continuous import ContinuousMixin, CSMContinuousListener, CSMUtterance  # noqa: F401
from .csm_listen import CSMListener, ListenResult, SpeechSpan, _claim, _fail_future  # noqa: F401


@dataclass
class StreamResult:
    """One request's result: what `BatchResult` holds for one stream."""
    audio: Optional[torch.Tensor]  # [samples], None with decode=False
    frames: int                    # frames generated (up to, not including, the EOS frame)
    codes: torch.Tensor            # [n_cb, frames]
    sample_rate: int
    stream_id: int
    row: int                       # the cache row the stream ran in
    processing_time_seconds: float  # submit -> result
    interrupted: bool = False      # ended by `interrupt`: `frames` is what was kept of it
    format: str = "f32"            # what `audio` holds (`pcm.FORMATS`): float32, int16 ("s16le") or uint8 ("mulaw", "alaw") samples


@dataclass
class AudioChunk:
    """One piece of a streaming request's waveform: stream-local frames [first_frame, first_frame + frames).  A request made with
    `sample_rate=R` gets its audio at R: a chunk then holds the resampler's finished outputs for the samples up to its frames (about ten samples
    of the slower rate lag behind), the final chunk the rest.  The chunks add up to `StreamResult.audio` unless an `interrupt` cut the stream
    inside a chunk it had already been sent: then the result is the resample of the kept audio and the chunks sent are not a prefix of it."""
    audio: torch.Tensor  # [samples]
    first_frame: int
    frames: int
    final: bool          # the stream's last chunk: `result()` is ready
    format: str = "f32"  # what `audio` holds (`pcm.FORMATS`): a request made with `format=` gets int16 / uint8 samples


class CSMAudioStream:
    """What `submit_stream` returns.  Iterating yields the request's `AudioChunk`s as the scheduler produces them and ends behind the final
    one; a failed request (or `close()`) ends the iteration by raising its error and a cancelled one by raising `CancelledError`, never by
    hanging.  `result(timeout)` is the usual `StreamResult`; its audio is the concatenation of the chunks (of an interrupted stream: cut to
    the frames kept).  `first_audio_seconds`: submit -> first chunk, once there is one.  `cancel()` / `interrupt(...)`: the batcher's."""

    def __init__(self, future: Future, batcher: Optional["CSMBatcher"] = None):
        self.future = future
        self._batcher = batcher
        self.first_audio_seconds: Optional[float] = None
        self._q: "queue.Queue" = queue.Queue()
        future.add_done_callback(self._ended)

    def _ended(self, fut: Future) -> None:  # a failure from ANY path of the scheduler reaches the consumer (success: the final chunk is already queued)
        e = CancelledError() if fut.cancelled() else fut.exception()
        if e is not None:
            self._q.put(e)

    def __iter__(self):
        while True:
            item = self._q.get()
            if isinstance(item, BaseException):
                raise item
            yield item
            if item.final:
                return

    def result(self, timeout: Optional[float] = None) -> StreamResult:
        return self.future.result(timeout)

    def cancel(self) -> bool:
        return self._batcher.cancel(self)

    def interrupt(self, played_frames: Optional[int] = None, played_samples: Optional[int] = None) -> bool:
        return self._batcher.interrupt(self, played_frames=played_frames, played_samples=played_samples)


@dataclass
class _Stream:
    future: Future
    context: Sequence
    text: object
    speaker: int
    voice_match: bool
    max_frames: int
    seed: Optional[int]
    stream_id: int
    length: int                     # prompt frames
    t0: float
    prompt: Optional[tuple] = None  # (tokens [S, n_cb+1], mask); with `prefix`: the frames behind the prefix
    prefix: object = None           # sesame.VoicePrefix: the prompt is the prefix followed by `prompt`
    row: int = -1
    rng: Optional[np.random.Generator] = None
    codes: List[torch.Tensor] = field(default_factory=list)  # one [n_cb] tensor per generated frame
    audio: Optional[CSMAudioStream] = None  # submit_stream: where the chunks go
    sampler: object = None          # row_samplers: the request's sampler (the batcher's when it gave none)
    chunks: List[torch.Tensor] = field(default_factory=list)  # the audio of the chunks emitted so far
    emitted: int = 0                # frames decoded and emitted
    confirmed: int = 0              # frames a poll has confirmed (below the EOS frame and the limit)
    ended: bool = False             # a poll has seen the stream's end: `confirmed` is its length
    session: object = None          # CSMSession: the request is a turn of it
    captured: Optional[dict] = None  # the session's next state (CSMSession._capture), taken before the row was parked
    capture_error: Optional[BaseException] = None
    lane: int = -1                  # overlap_admission: the prefill lane that holds the request until it is committed
    prefill: object = None          # what the engine's `prefill` returned for it
    admit_args: Optional[tuple] = None  # (sampler, seed) of its admission: what `set_row_sampler` takes at the commit
    cut: Optional[int] = None       # interrupt: the frames that were heard; the next poll ends the stream with at most that many
    decodable: int = 0              # interrupt of a streaming request: the frames that poll confirmed before the cut (what the codec may be fed)
    rate: Optional[int] = None      # sample_rate=R: the audio leaves at R (None: the model's rate)
    rchunks: List[torch.Tensor] = field(default_factory=list)  # a streaming request with a rate: the audio of its chunks at R
    rflushed: bool = False          # ... and whether its resampler row has been flushed: `rchunks` is then the whole result
    fmt: Optional[str] = None       # format=: the audio leaves as int16 / uint8 samples (None: float32); `rchunks` then holds the encoded chunks
    held: bool = True               # the scheduler still has the request (queue, lane or row): a cancelled turn keeps its session busy until it is dropped


def _no_frames(n_cb: int):
    return np.zeros((0, n_cb + 1), np.int32), np.zeros((0, n_cb + 1), np.float32)


def _cat(a, b):
    return np.concatenate([a[0], b[0]], 0), np.concatenate([a[1], b[1]], 0)


class CSMSession:
    """One conversation on a `CSMBatcher` (`batcher.session(context, speaker)`): the K / V of everything said so far stay on the device between
    its turns.  `submit(text)` / `submit_stream(text)` (or the batcher's `submit(session=self, ...)`) run the next turn, `hear(segment)` adds
    another speaker's turn, `rebuild()` re-prefills the history when it has outgrown the cache, `close()` frees the device copy.

    prefix: None, or what the next turn is admitted on top of -- the K / V captured at the end of the last turn, or the caller's `VoicePrefix`
    the session started from.  n: the positions it covers.  pending: host frames (tokens, mask), each [k, n_cb+1], that belong to the history but
    are not in the prefix yet: the next turn's prompt block starts with them.  history: the frames of all n + k positions.  turns: (speaker,
    text, frames generated) per turn, 0 frames for a turn that was heard.

    One turn at a time: a second `submit` while one is queued or live is refused, and so is `hear`.  A turn that fails, wherever, leaves the
    session as it was: the state is replaced as a whole when the turn's result is ready.  The session destroys the prefixes it captured (on
    replace and on `close`), never a caller's `VoicePrefix`."""

    def __init__(self, batcher: "CSMBatcher", context=None, speaker: int = 0):
        self.batcher, self.engine, self.speaker = batcher, batcher.engine, int(speaker)
        self.prefix, self.n, self._own = None, 0, False
        self.pending = _no_frames(self.engine.n_cb)
        self.history = _no_frames(self.engine.n_cb)
        self.turns: List[tuple] = []
        self._starts: List[int] = []  # where in `history` each turn begins
        self._voice = 0               # leading history frames that are no turn: the caller's voice prefix (`rebuild` keeps them)
        self._turn: Optional[Future] = None
        self._stream: Optional[_Stream] = None  # the turn's request, while the scheduler has it
        self._hearing: Optional[Future] = None  # a listener's `end()`, until the scheduler has entered the heard turn
        self._closed = False
        if context is None:
            return
        if hasattr(context, "length"):  # a sesame.VoicePrefix: its K / V are on the device already
            if not self.engine.owns(context):
                raise ValueError("the voice prefix was made on another model's weights (Model.voice_prefix on this model or one it shares weights with)")
            self.prefix, self.n = context, int(context.length)
            self._voice = self.n
            self.history = (np.array(context.tokens, np.int32), np.array(context.mask, np.float32))
            return
        for seg in context:
            self.hear(seg)

    @property
    def length(self) -> int:
        """Positions of the history: what the next turn's text is put behind."""
        return self.n + int(self.pending[0].shape[0])

    @property
    def busy(self) -> bool:
        """A turn is queued or live.  A cancelled turn counts until the scheduler has dropped it: its row is live until then."""
        t, s, h = self._turn, self._stream, self._hearing
        if h is not None and not h.done():  # from a listener's `end()` to its result
            return True
        return t is not None and (not t.done() or (t.cancelled() and s is not None and s.held))

    def _ready(self, what: str) -> None:
        if self._closed:
            raise ValueError(f"{what}: the session is closed")
        if self.busy:
            raise ValueError(f"{what}: the session has a turn queued or live; wait for its result first")

    def hear(self, segment, codes=None) -> None:
        """Another speaker's turn: its text frames, its audio frames and the EOS frame, as `Model.prompt_frames` lays a context segment out.
        They join `pending`; the frame generator sees them at the next admission.  The clip goes through `Model.encode_audios` here, on the
        caller's thread, unless `codes` [n_cb, T] (its Mimi codes) are passed."""
        self._ready("hear")
        self._hear(segment, codes)

    def _hear(self, segment, codes) -> None:
        f = self.engine.segment_frames(segment, codes)
        f = (np.asarray(f[0], np.int32), np.asarray(f[1], np.float32))
        self._starts.append(int(self.history[0].shape[0]))
        self.turns.append((int(segment.speaker), segment.text, 0))
        self.pending, self.history = _cat(self.pending, f), _cat(self.history, f)

    def listen(self, speaker: int = 0, sample_rate: Optional[int] = None, format: Optional[str] = None, vad=None, barge_in: bool = False,
               continuous: bool = False, transcribe=None):
        """`CSMBatcher.listen` for this conversation: another speaker's microphone.  Allowed while the session's own turn is queued or live
        (a barge-in); the turn enters the history at the listener's `end(text)`, which waits for that turn as `hear` does.
        vad (`vad.VadConfig`, or True for the defaults): the scheduler finds the utterance itself.  barge_in (needs vad): the
        round that sees the speaker's onset interrupts this session's queued or live turn, which keeps what it has emitted.
        continuous (needs vad): the microphone stays open and yields one `CSMUtterance` per utterance (`CSMContinuousListener`, DESIGN
        8d-13); each `utt.end(text)` enters the history as `hear` would, and with barge_in EVERY onset interrupts the queued or live turn.
        transcribe (needs a batcher made with `stt=`): `lis.transcript` / `utt.transcript` resolves with Whisper's
        `DecodingResult` of the utterance; with the batcher's `stt_text=`, `end()` may then be called without text."""
        if self._closed:
            raise ValueError("listen: the session is closed")
        kw = {} if format is None else {"format": format}
        if continuous:
            kw["continuous"] = True
        if transcribe is not None and transcribe is not False:
            kw["transcribe"] = transcribe
        if vad is not None and vad is not False:
            kw.update(vad=vad, barge_in=barge_in)
        elif barge_in:
            raise ValueError("listen: barge_in needs vad=")
        return self.batcher.listen(speaker=speaker, session=self, sample_rate=sample_rate, **kw)

    def submit(self, text, **kw) -> Future:
        kw.setdefault("speaker", self.speaker)
        return self.batcher.submit(session=self, text=text, **kw)

    def submit_stream(self, text, **kw) -> CSMAudioStream:
        kw.setdefault("speaker", self.speaker)
        return self.batcher.submit_stream(session=self, text=text, **kw)

    def cancel(self) -> bool:
        """`CSMBatcher.cancel` of the session's queued or live turn: the turn did not happen, the session is as it was before its submit and takes
        the next `submit` / `hear` once the scheduler has dropped the turn (`busy`).  False without such a turn."""
        return self._turn is not None and self.batcher.cancel(self._turn)

    def interrupt(self, played_frames: Optional[int] = None, played_samples: Optional[int] = None) -> bool:
        """`CSMBatcher.interrupt` of the session's queued or live turn: the turn ends now and enters the history as a turn of the k frames that
        were heard (its text frames stay whole: they are in the K / V already and the listener's side of the conversation has no say in them).
        With k = 0 the turn is cancelled.  False without such a turn."""
        return self._turn is not None and self.batcher.interrupt(self._turn, played_frames=played_frames, played_samples=played_samples)

    # ---- the end of a turn (the scheduler's thread) ------------------------------------------------------------------------------------
    def _capture(self, s: "_Stream", count: int) -> dict:
        """Before the turn's row is parked: the session's next state.  The prompt had L positions; after len(codes) samples the row holds
        L + len(codes) - 1 (the last sample was never fed).  Of the `count` kept frames those that were fed are in the cache: the capture
        takes L + min(count, len(codes) - 1) positions and never one past the kept frames, so it does not depend on how far the row ran
        beyond its EOS frame.  What the cache lacks -- the last kept frame after a limit end, nothing after an EOS end -- and the EOS frame
        are the next turn's first prompt frames."""
        L, n_cb = int(s.length), self.engine.n_cb
        n = L + min(count, len(s.codes) - 1)
        prefix = self.engine.capture(s.row, n)
        try:
            kept = torch.stack(s.codes[:count]).cpu().numpy()
            tok, msk = np.zeros((count + 1, n_cb + 1), np.int32), np.zeros((count + 1, n_cb + 1), np.float32)
            tok[:count, :n_cb] = kept  # (the last row stays zero: the EOS frame, Model._tokenize_audio)
            msk[:, :n_cb] = 1
            k = int(self.pending[0].shape[0])
            said = (s.prompt[0][k:], s.prompt[1][k:])  # the turn's text frames
            return dict(prefix=prefix, n=n, pending=(tok[n - L:], msk[n - L:]), history=_cat(_cat(self.history, said), (tok, msk)),
                        turn=(s.speaker, s.text, count))
        except BaseException:
            prefix.close()
            raise

    def _commit(self, c: dict) -> None:
        if self._closed:
            c["prefix"].close()
            return
        old, own = self.prefix, self._own
        self._starts.append(int(self.history[0].shape[0]))
        self.turns.append(c["turn"])
        self.prefix, self.n, self.pending, self.history, self._own = c["prefix"], c["n"], c["pending"], c["history"], True
        if own and old is not None:
            old.close()

    # ---- the way out of a full cache ---------------------------------------------------------------------------------------------------
    def rebuild(self, keep_last_turns: Optional[int] = None) -> None:
        """Compute the prefix again from `history` through the prompt kernels (`SesameModel.make_prefix`) -- of the whole history, or of the
        voice prefix the session started from and its last `keep_last_turns` turns; the dropped turns leave `history` and `turns`.  The kept
        turns move to new positions and their K / V are a prompt block's from then on: later turns differ from those of the untrimmed
        session, as any shorter prompt's would.  Runs on the caller's thread, as `Model.voice_prefix` does."""
        self._ready("rebuild")
        tok, msk = self.history
        if keep_last_turns is not None:
            k = int(keep_last_turns)
            if k < 0:
                raise ValueError("keep_last_turns must be >= 0")
            if k < len(self.turns):
                cut = self._starts[len(self.turns) - k] if k > 0 else int(tok.shape[0])
                v = self._voice
                tok, msk = np.concatenate([tok[:v], tok[cut:]], 0), np.concatenate([msk[:v], msk[cut:]], 0)
                self.turns = self.turns[len(self.turns) - k:] if k > 0 else []
                self._starts = [st - (cut - v) for st in self._starts[len(self._starts) - k:]] if k > 0 else []
        new = self.engine.make_prefix(tok, msk) if tok.shape[0] else None
        old, own = self.prefix, self._own
        self.prefix, self.n, self._own = new, int(tok.shape[0]), new is not None
        self.history, self.pending = (tok, msk), _no_frames(self.engine.n_cb)
        if own and old is not None:
            old.close()

    def close(self) -> None:
        """Free the session's captured prefix; a turn still queued or live fails or is dropped at its end.  Later submits are refused."""
        self._closed = True
        if self._own and self.prefix is not None and not self.busy:
            self.prefix.close()
        if not self.busy:
            self.prefix, self._own = None, False


class ModelEngine:
    """What the batcher needs of a `sesame.Model` (frame generator + codec).  The scheduler talks to this surface only, so it can be
    driven against a scripted engine without a device."""

    def __init__(self, model):
        self.model = model
        self.csm = model.model
        self.n_cb = int(model.n_cb)
        self.max_pos = int(self.csm.cfg["max_seq_len"])
        self.sample_rate = int(model.sample_rate)
        self.device = self.csm.device

    @property
    def samples_per_frame(self) -> int:
        """Waveform samples of one frame: what `interrupt(played_samples=)` divides by (a frame is 80 ms where there is no codec to ask)."""
        mimi = self.model._audio_tokenizer
        return int(mimi.lib.kk_mimi_samples_per_frame(mimi._h)) if mimi is not None else int(round(self.sample_rate * 0.08))

    def start(self, max_batch: int) -> None:
        if not self.csm.caches_are_enabled() or self.csm.max_batch != max_batch:
            self.csm.setup_caches(max_batch)
        self.csm.reset_caches_parked()
        self.csm.set_graph_mode(True)

    def prompt_length(self, context, text, speaker: int, voice_match: bool) -> int:
        """Frames of `Model.prompt_frames(...)` from lengths alone (no device work: submit() runs on the caller's thread)."""
        m = self.model
        mimi = m._audio_tokenizer

        def audio_frames(a):
            return int(mimi.lib.kk_mimi_encode_frames(mimi._h, int(np.asarray(a).shape[-1])))

        if voice_match:
            if not context:
                raise ValueError("voice_match needs a context segment")
            c0 = context[0]
            if text is None:
                n = len(m._text_ids(c0.text, speaker))
            elif not isinstance(c0.text, str) or not isinstance(text, str):
                n = len(m._text_ids(c0.text, speaker)) + len(m._text_ids(text, speaker))
            else:
                n = len(m._text_ids((c0.text + " " + text).strip(), speaker))
            return n + (audio_frames(c0.audio) if c0.audio is not None else 0)
        n = 0
        for seg in context:
            n += len(m._text_ids(seg.text, seg.speaker)) + (audio_frames(seg.audio) + 1 if seg.audio is not None else 0)
        return n + (len(m._text_ids(text, speaker)) if text is not None else 0)

    def prompts(self, streams: Sequence[_Stream]):
        """The prompts of the requests admitted in one round; streams that agree on (speaker, voice_match) share Mimi.encode calls."""
        out: Dict[int, tuple] = {}
        groups: Dict[tuple, List[int]] = {}
        for i, s in enumerate(streams):
            groups.setdefault((s.speaker, s.voice_match), []).append(i)
        for (speaker, vm), idx in groups.items():
            got = self.model.prompt_frames_batch([streams[i].context for i in idx], [streams[i].text for i in idx], speaker, vm)
            for i, p in zip(idx, got):
                out[i] = p
        return [out[i] for i in range(len(streams))]

    def prefixed_prompt(self, prefix, text, speaker: int):
        """The frames a request puts behind the voice prefix `prefix` (sesame.VoicePrefix): its own text segment.  Host work only.  ValueError
        for a prefix that was made on other weights than this engine's."""
        if getattr(prefix, "root", None) is not self.csm.weights_root():
            raise ValueError("the voice prefix was made on another model's weights (Model.voice_prefix on this model or one it shares weights with)")
        return self.model._tokenize_text_segment(text, speaker)

    def owns(self, prefix) -> bool:
        """Whether a sesame.VoicePrefix was made on the weights this engine runs on."""
        return getattr(prefix, "root", None) is self.csm.weights_root()

    def segment_frames(self, segment, codes=None):
        """A heard turn's frames (text, audio, EOS) for `CSMSession.hear`; `codes`: the clip's Mimi codes, else it is encoded here."""
        return self.model._tokenize_segment(segment, add_eos=True, codes=codes)

    def make_prefix(self, tokens, mask):
        """`CSMSession.rebuild`: the frames' K / V through the prompt kernels, as a VoicePrefix."""
        from .sesame import VoicePrefix

        return self._mark(VoicePrefix(prefix=self.csm.make_prefix(tokens, mask), tokens=tokens, mask=mask, length=int(tokens.shape[0]),
                                      root=self.csm.weights_root()))

    def _mark(self, vp):
        """With prefill lanes: an event behind the launch that wrote the prefix, for the side stream to wait on (`prefill`)."""
        if getattr(self, "_side", None) is not None:
            vp.ready = torch.cuda.Event()
            vp.ready.record(torch.cuda.current_stream(self.device))
        return vp

    def session_prompt(self, sess: CSMSession, text, speaker: int):
        """The frames a session's turn puts behind the session's prefix: its pending history frames, then the turn's own text segment.  Host
        work only.  ValueError for a session of another engine."""
        if sess.engine is not self:
            raise ValueError("the session belongs to another batcher's engine (CSMBatcher.session on this batcher)")
        return _cat(sess.pending, self.model._tokenize_text_segment(text, speaker))

    def capture(self, row: int, n: int):
        """The first `n` positions of live row `row` as a prefix of the session's own (SesameModel.capture_prefix): what `admit(prefix=)` takes."""
        from .sesame import VoicePrefix

        return self._mark(VoicePrefix(prefix=self.csm.capture_prefix(row, n), tokens=None, mask=None, length=int(n), root=self.csm.weights_root()))

    def row_state(self):
        return self.csm.row_state()

    def park(self, row: int) -> None:
        self.csm.park(row)

    def shift(self, delta: int) -> None:
        self.csm.shift(delta)

    def admit(self, row: int, prompt, sampler, uniforms, seed, stream_id: int, prefix=None) -> torch.Tensor:
        return self.csm.admit(row, prompt[0], prompt[1], sampler=sampler, uniforms=uniforms, seed=seed, stream_id=stream_id,
                              prefix=prefix.prefix if prefix is not None else None)

    def set_row_sampler(self, row: int, sampler, seed) -> None:
        """Cache row `row` samples with `sampler` (and draws on `seed` on the device) in every later `frame(sampler="rows")`."""
        self.csm.set_row_sampler(row, sampler, seed)

    def frame(self, prev: torch.Tensor, sampler, uniforms, seed, stream_ids, device_rng: bool = False) -> torch.Tensor:
        """sampler "rows": every row's settings (and seed, with device_rng) are those of `set_row_sampler`; `seed` is not read then."""
        B, n = prev.shape
        curr = torch.zeros((B, 1, n + 1), dtype=torch.int32, device=self.device)
        curr[:, 0, :n] = prev
        mask = torch.zeros((B, 1, n + 1), dtype=torch.float32, device=self.device)
        mask[:, 0, :n] = 1
        u = torch.tensor(np.asarray(uniforms, np.float32), device=self.device) if uniforms is not None else None
        if isinstance(sampler, str):
            return self.csm.generate_frame(curr, mask, sampler=sampler, uniforms=u, device_rng=device_rng, stream_ids=stream_ids)
        return self.csm.generate_frame(curr, mask, sampler=sampler, uniforms=u, seed=seed, stream_ids=stream_ids)

    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        if self.model._audio_tokenizer is None:
            raise ValueError("decoding needs the Mimi codec: pass mimi= or config['mimi_path']")
        return self.model._audio_tokenizer.decode(codes)[:, 0]

    def row_decoder(self, max_batch: int, max_frames: int, max_chunk: int):
        """The codec's row-mode streaming decoder (mimi.MimiRowDecoder): reset_row, step(codes, active), row_frames, close."""
        if self.model._audio_tokenizer is None:
            raise ValueError("streaming audio needs the Mimi codec: pass mimi= or config['mimi_path']")
        return self.model._audio_tokenizer.row_decoder(max_batch, max_frames, max_chunk)

    def row_encoder(self, max_batch: int, max_frames: int, max_chunk: int):
        """The codec's row-mode streaming encoder (mimi.MimiRowEncoder): reset_row, step(pcm, active), row_frames, close."""
        if self.model._audio_tokenizer is None:
            raise ValueError("listening needs the Mimi codec: pass mimi= or config['mimi_path']")
        return self.model._audio_tokenizer.row_encoder(max_batch, max_frames, max_chunk)

    def row_resampler(self, max_rows: int, max_in: int):
        """A row-mode polyphase resampler on the engine's device (resample.RowResampler): set_row, step(x, n_in, flush), out_view, close."""
        return RS.RowResampler(max_rows, max_in, device=self.device)

    def row_vad(self, max_rows: int):
        """A row-mode voice-activity detector on the engine's device (vad.RowVad): set_row, step(x, n_avail), fetch, close."""
        return VAD.RowVad(max_rows, device=self.device)

    def row_ring_vad(self, max_rows: int):
        """The re-arming detector over a ring on the engine's device (vad.RingVad): set_row, step(x, n_avail, acked), fetch, close."""
        return VAD.RingVad(max_rows, device=self.device)

    def ring_write(self, src, ring, ring_len: int, pos, n) -> None:
        """ring[b, (pos[b] + i) % ring_len] = src[b, i], i < n[b]: one launch for all rows (ring.write_rows)."""
        RING.write_rows(src, ring, ring_len, pos, n)

    def ring_read(self, ring, ring_len: int, dst, pos, n, n_total) -> None:
        """dst[b, i] = ring[b, (pos[b] + i) % ring_len], i < n[b], zeros up to n_total[b]: one launch for all rows (ring.read_rows)."""
        RING.read_rows(ring, ring_len, dst, pos, n, n_total)

    def pcm_converter(self):
        """The PCM converter of rows at the model's own rate on the engine's device (pcm.RowConverter): convert(x, in_formats, out_formats, n), close."""
        return PCM.RowConverter(device=self.device)

    def heard_segment(self, speaker: int, text, audio):
        """The `Segment` a listened turn enters a session's history as (`CSMSession._hear` -> `segment_frames`)."""
        from .sesame import Segment

        return Segment(speaker=int(speaker), text=text, audio=audio)

    def span_windows(self, spans, W: int, n_mels: int) -> torch.Tensor:
        """Spans (buffer row, ring length or 0, start, samples) of the listeners' device buffers at the model's rate -> their Whisper windows
        (R, W, n_mels) in one launch pair (whisper.span_windows)."""
        from . import whisper as WH

        return WH.span_windows(spans, W, n_mels, src_rate=int(self.sample_rate))

    def synchronize(self) -> None:
        torch.cuda.current_stream(self.device).synchronize()

    # ---- prefill lanes: admissions computed on a side stream, committed by one copy -------------------------------------------
    def open_lanes(self, n: int) -> None:
        """`n` one-row generators on this model's weights (`share()` + `setup_caches(1)`) and ONE side stream that runs all their prefills.
        A second stream runs no kernel: it stands for "this lane's prefill is done" at a commit (`commit`)."""
        self._side = torch.cuda.Stream(self.device)
        self._hand = torch.cuda.Stream(self.device)
        self._lanes = []
        for _ in range(int(n)):
            g = self.csm.share()
            g.setup_caches(1)
            self._lanes.append(g)

    def prefill(self, lane: int, prompt, sampler, uniforms, seed, stream_id: int, prefix=None, timed: bool = False):
        """Begin a request's admission in lane `lane`, on the side stream: what the batcher does on its own generator for a plain admission --
        `reset_caches_parked`, a bare position move to the prompt's length, `admit` / `admit(prefix=)` into row 0 -- and an event behind it.
        Nothing here waits for the device: the frames go up from pinned memory.  Returns the handle `prefill_ready` and `commit` take."""
        g, dev = self._lanes[lane], self.device
        L = int(prompt[0].shape[0]) + (int(prefix.length) if prefix is not None else 0)

        def up(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a, dtype)).pin_memory().to(dev, non_blocking=True)

        main = torch.cuda.current_stream(dev)
        if prefix is not None:  # its K / V were written on the batch's stream (a capture, `make_prefix`): the lane reads them behind that point
            ready = getattr(prefix, "ready", None)
            if ready is None:
                ready = prefix.ready = torch.cuda.Event()
                ready.record(main)
            self._side.wait_event(ready)
        with torch.cuda.stream(self._side):
            start = None
            if timed:
                start = torch.cuda.Event(enable_timing=True)
                start.record()
            g.reset_caches_parked()
            g.shift(L)  # nothing is live in the lane: only its position moves
            u = up(np.asarray(uniforms, np.float32).reshape(-1), np.float32) if uniforms is not None else None
            codes = g.admit(0, up(prompt[0], np.int32), up(prompt[1], np.float32), sampler=sampler, uniforms=u, seed=seed, stream_id=stream_id,
                            prefix=prefix.prefix if prefix is not None else None)
            end = torch.cuda.Event(enable_timing=timed)
            end.record()
        codes.record_stream(main)  # read by the batch's stream behind the commit
        return {"codes": codes, "start": start, "end": end}

    def prefill_ready(self, handle, wait: bool = False) -> bool:
        """Whether the lane's admission has completed (`event.query()`: no sync).  wait: block until it has -- only while no row is live."""
        if wait:
            handle["end"].synchronize()
            return True
        return bool(handle["end"].query())

    def commit(self, row: int, lane: int, handle) -> torch.Tensor:
        """The lane's finished admission enters cache row `row` (`SesameModel.admit_transfer`: one copy launch on the batch's stream, ordered
        behind the lane's work and ahead of the lane's next use) and the lane's row is parked.  Returns the admission's codes [n_cb].
        The entry orders the copy behind everything its source stream holds at the call.  On the side stream that would include the prefills
        other lanes have queued behind this one, so the source stream handed over is the hand-off stream, which waits for THIS prefill's
        event only; the side stream then waits for the hand-off stream, which the entry has put behind the copy."""
        g = self._lanes[lane]
        self._hand.wait_event(handle["end"])
        self.csm.admit_transfer(row, g, 0, self._hand)
        self._side.wait_stream(self._hand)
        g.park(0)
        return handle["codes"]

    def prefill_seconds(self, handle) -> float:
        """Device time of a completed `prefill(timed=True)` on the side stream."""
        return float(handle["start"].elapsed_time(handle["end"])) * 1e-3 if handle["start"] is not None else 0.0

    def close_lanes(self) -> None:
        if getattr(self, "_side", None) is not None:
            self._side.synchronize()
        self._lanes, self._side, self._hand = [], None, None


def _check_sampler(sampler) -> None:
    """The ranges the library accepts (kk_csm_sampler), checked where the request is made"""
    try:
        temp, top_k = float(sampler.temp), int(sampler.top_k)
        top_p, min_p, keep = float(getattr(sampler, "top_p", 0.0)), float(getattr(sampler, "min_p", 0.0)), int(getattr(sampler, "min_tokens_to_keep", 1))
    except (AttributeError, TypeError) as e:
        raise ValueError(f"sampler must carry temp / top_k (make_sampler): {e}") from None
    if not (temp >= 0.0 and 0.0 <= top_p <= 1.0 and 0.0 <= min_p <= 1.0 and keep >= 1 and top_k >= -1):
        raise ValueError("sampler out of range (temp >= 0, top_p and min_p in [0, 1], min_tokens_to_keep >= 1, top_k >= -1)")


def _fail(s: _Stream, e: BaseException) -> None:
    """The request failed and is nowhere in the scheduler any more.  A future that was cancelled meanwhile keeps its cancellation."""
    s.held = False
    _fail_future(s.future, e)


class CSMBatcher(ContinuousMixin):
    def __init__(self, model, max_batch: int = 8, eos_check_interval: int = 8, rng: str = "device", sampler=None, seed: int = 0,
                 stop_on_eos: bool = True, decode: bool = True, profile: bool = False, engine=None, stream_chunk_frames: Optional[int] = None,
                 stream_max_frames: int = 1125, row_samplers: bool = False, overlap_admission: bool = False, prefill_lanes: int = 1,
                 listen_rows: int = 0, listen_chunk_frames: int = 6, listen_max_frames: int = 375, stt=None, stt_rounds_per_round: int = 4,
                 stt_text=None):
        """model: a loaded sesame.Model (its frame generator's caches are taken over; use `model.share()` for a generator of its own).
        sampler: `make_sampler(...)` for every stream of the batch (default temp 0.9 / top_k 50; with `row_samplers` the default of a request).  seed: the device generator's seed (rng
        "device": one seed per batcher, streams differ by their ids).  profile: time admissions and shifts (one sync each) into `stats`.
        engine: the surface of `ModelEngine`, for a scheduler without a device.
        stream_chunk_frames: N enables `submit_stream` (audio in chunks of N frames through the codec's row-mode decoder); the EOS flags are
        then polled every N frames instead of every `eos_check_interval`.  stream_max_frames: the longest streaming request (the decoder's K / V
        cache holds that many frames per row; 1125 = the default 90 s limit of a request).
        row_samplers: True lets `submit` / `submit_stream` take a `sampler` (None: the batcher's) and, with rng "device", a `seed` of the
        request's own (None: the batcher's); the frame step then reads each row's settings from the device table (`set_row_sampler`).  Off by
        default: the frame step is the launch-argument one, and a per-request sampler or a foreign seed is refused.
        overlap_admission: True prefills every request in one of `prefill_lanes` lanes (a `share()` generator with one cache row each, one side
        stream for all) while the batch keeps stepping, and commits it with one copy when a row is free and the lane is done.
        Off by default: no lane is made and admissions run on the batch's stream.
        listen_rows: K > 0 enables `listen` (up to K listeners at a time) on one row-mode streaming encoder of K rows; encoder rows are not
        cache rows, so listening never occupies a generation row.  listen_chunk_frames: M, the frames of one encode step (a listener's
        stream is always encoded in [M] * (T // M) + [T % M]).  listen_max_frames: the longest heard turn (the encoder's K / V cache holds
        that many frames per row; 375 = 30 s).  0: no encoder is made and `step` is what it was.
        stt: a `whisper_model.serve(...)` (whisper_serve.WhisperBatcher) that has NOT been started enables `listen(transcribe=...)` (DESIGN
        8d-15): this scheduler cuts the listeners' utterances into Whisper windows on the device and steps `stt` itself, on its own thread and
        stream -- up to `stt_rounds_per_round` of its rounds per scheduling round while it has queued or live requests.  The caller may still
        `stt.submit(...)`; `close()` leaves `stt` open.  stt_text: a callable DecodingResult -> what `end(text)` takes (ids or str), which
        lets a session's transcribing listener `end()` without text.  None: nothing of it is made and `step` is what it was."""
        if overlap_admission and int(prefill_lanes) < 1:
            raise ValueError("prefill_lanes must be >= 1")
        if rng not in ("host", "device"):
            raise ValueError(f"rng must be 'host' or 'device', not {rng!r}")
        if max_batch < 1 or eos_check_interval < 1:
            raise ValueError("max_batch and eos_check_interval must be >= 1")
        if stream_chunk_frames is not None and (int(stream_chunk_frames) < 1 or int(stream_max_frames) < int(stream_chunk_frames) or not decode):
            raise ValueError("stream_chunk_frames must be in [1, stream_max_frames] and needs decode=True")
        if int(listen_rows) < 0 or (int(listen_rows) > 0 and not 1 <= int(listen_chunk_frames) <= int(listen_max_frames)):
            raise ValueError("listen_rows must be >= 0 and listen_chunk_frames in [1, listen_max_frames]")
        if sampler is None:
            from .sesame import make_sampler

            sampler = make_sampler(temp=0.9, top_k=50)
        self.engine = engine if engine is not None else ModelEngine(model)
        self.max_batch, self.interval, self.rng, self.sampler, self.seed = int(max_batch), int(eos_check_interval), rng, sampler, int(seed)
        self.stop_on_eos, self.decode, self.profile = bool(stop_on_eos), bool(decode), bool(profile)
        self._sampled = float(sampler.temp) > 0
        self.row_samplers = bool(row_samplers)
        if self.row_samplers:
            _check_sampler(sampler)
        self._lock = threading.Lock()          # queue, closed flag, stream id counter, pending controls
        self._wake = threading.Condition(self._lock)
        self._queue: Deque[_Stream] = deque()
        self._controls: List[tuple] = []       # (future, "cancel" | "interrupt", frames heard or None): recorded by callers, applied by `step`
        self._closed = False
        self._thread: Optional[threading.Thread] = None
        self._next_id = 0
        self._rows: List[Optional[_Stream]] = [None] * self.max_batch
        self._since_poll = 0
        self.stats = {"frames": 0, "live_row_frames": 0, "admissions": 0, "admit_seconds": 0.0, "shifts": 0, "shift_seconds": 0.0,
                      "shifts_down": 0, "shifts_up": 0, "polls": 0, "finished": 0, "prefixed_admissions": 0, "session_admissions": 0, "captures": 0,
                      "overlapped_admissions": 0, "commit_seconds": 0.0, "prefill_seconds": 0.0, "cancelled": 0, "interrupted": 0}
        self.engine.start(self.max_batch)
        self.overlap = bool(overlap_admission)
        self._lane_of: List[Optional[_Stream]] = []   # per lane: the request it holds
        self._inflight: Deque[_Stream] = deque()      # requests in a lane, in queue order: only the head may be committed
        if self.overlap:
            self.engine.open_lanes(int(prefill_lanes))
            self._lane_of = [None] * int(prefill_lanes)
            if self.profile:  # the frame step's time with / without a prefill in flight on the side stream
                self.stats.update(frames_prefill_in_flight=0, frame_seconds_prefill_in_flight=0.0, frames_no_prefill=0, frame_seconds_no_prefill=0.0)
        self.chunk = int(stream_chunk_frames) if stream_chunk_frames is not None else None
        self.stream_max_frames = int(stream_max_frames)
        self._dec = None
        if self.chunk is not None:
            self.interval = self.chunk  # a chunk is decoded once a poll has confirmed it: poll at the chunk cadence
            self.stats.update(chunks=0, chunk_rounds=0)
            self._dec = self.engine.row_decoder(self.max_batch, self.stream_max_frames, self.chunk)
        self._listen_init(listen_rows, listen_chunk_frames, listen_max_frames)  # (csm_listen.py: also the stateless PCM converter `_cvt`, which the output side shares)
        self._stt_init(stt, stt_rounds_per_round, stt_text)  # (csm_listen.py)
        # other sample rates: made by the scheduler when the first request with a rate needs them, never before
        self._ors = None                       # the streaming requests' resampler, one row per cache row
        self._crs = None                       # one row for whole clips (a plain request's result): made once, so no allocation per result
        self._rate_of: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()  # future -> the request's rate (under the lock)
        dev = self.engine.device
        self._prev = torch.zeros((self.max_batch, self.engine.n_cb), dtype=torch.int32, device=dev)
        self._first_eos = torch.full((self.max_batch,), -1, dtype=torch.int64, device=dev)  # stream-local index of the first all-zero frame
        self._local = torch.zeros((self.max_batch,), dtype=torch.int64, device=dev)        # stream-local index of the next frame

    # ---- requests ---------------------------------------------------------------------------------------------------------------------
    def session(self, context=None, speaker: int = 0) -> CSMSession:
        """A conversation on this batcher (`CSMSession`).  context: None, a `Model.voice_prefix(...)` (its K / V are used as they are and stay
        the caller's), or segments that the session hears before its first turn.  speaker: the default speaker of the session's own turns."""
        return CSMSession(self, context, speaker)

    def submit(self, context=None, text=None, speaker: int = 0, voice_match: Optional[bool] = None, max_audio_length_ms: float = 90_000,
               seed: Optional[int] = None, stream_id: Optional[int] = None, prompt=None, prefix=None, sampler=None, session=None,
               sample_rate: Optional[int] = None, format: Optional[str] = None) -> Future:
        """Queue one request; the future yields a `StreamResult`.  `prompt` (tokens, mask) skips the prompt building.  rng "host": `seed`
        seeds this stream's generator (None: fresh entropy).  rng "device": the batcher's seed is used, `seed` must be None or equal to it.
        ValueError at once for a request that cannot fit the cache; a request that races `close()` gets a failed future.
        `prefix` (`Model.voice_prefix(context)`): the request's prompt is the prefix followed by the text segment of `text` / `speaker` -- the
        non-voice_match layout with the prefix's context.  Its length is prefix.length + the text frames; the prefix's K / V are copied under
        the text frames at admission, nothing of the context is encoded, tokenised or computed again.  `prefix` excludes `context`, `prompt`
        and `voice_match=True` (ValueError): the voice_match layout merges the context's text with the request's in front of the audio, so it
        has no shareable prefix.  voice_match defaults to True without a prefix, as before.
        `sampler` (a batcher made with `row_samplers=True`; ValueError otherwise): this request's `make_sampler(...)`, None = the batcher's;
        with rng "device" such a batcher also takes a `seed` of the request's own.  An out-of-range sampler is a ValueError here.
        `session` (`self.session(...)`): the request is the session's next turn.  Its prompt is the session's prefix followed by the session's
        pending frames and the text segment of `text` / `speaker`; without a prefix (a first turn without a voice prefix) the whole goes through
        the plain admission.  The length that counts everywhere is session.n + those frames.  When the turn ends its K / V are captured for the
        next one.  `session` excludes `context`, `prompt`, `prefix` and `voice_match=True`; a session with a turn queued or live, a closed one
        and one of another batcher are refused (ValueError).
        `sample_rate` (None: the model's): the result's audio is `resample(a, model rate, sample_rate)` of the audio `a` the request yields
        without it, and `StreamResult.sample_rate` says so; `interrupt(played_samples=)` then counts samples at that rate.  ValueError for a
        rate the resampler does not take, and for a batcher made with decode=False.
        `format` (`pcm.FORMATS`; None or "f32": float32): the result's audio is `pcm.encode(a, format)` of the audio `a` the request yields
        without it at the same rate -- an int16 ("s16le") or uint8 ("mulaw", "alaw") device tensor, encoded in the resampler's launch or, at
        the model's rate, by one convert launch -- and `StreamResult.format` says so.  ValueError for another name and with decode=False."""
        return self._enqueue(False, context, text, speaker, voice_match, max_audio_length_ms, seed, stream_id, prompt, prefix, sampler, session,
                             sample_rate, format)

    def submit_stream(self, context=None, text=None, speaker: int = 0, voice_match: Optional[bool] = None, max_audio_length_ms: float = 90_000,
                      seed: Optional[int] = None, stream_id: Optional[int] = None, prompt=None, prefix=None, sampler=None,
                      session=None, sample_rate: Optional[int] = None, format: Optional[str] = None) -> CSMAudioStream:
        """`submit` with the audio delivered while the stream runs: the same arguments and refusals, a `CSMAudioStream` back.  Needs a batcher
        made with `stream_chunk_frames=N`; the request may not be longer than `stream_max_frames`.  With `sample_rate` every chunk passes
        through the cache row's resampler row and the final chunk flushes it: `AudioChunk.audio` is at that rate, a chunk's `frames` still
        count codec frames, and the chunks concatenate, bit for bit, to the resampled whole.  That also holds for a stream interrupted at or
        behind the frames it has been sent (the last chunk, of the frames still due or of 0 frames, carries the flush).  It does NOT hold for
        one cut inside a chunk it was already sent: the samples behind the cut have left, and the result is the resample of the kept audio.
        With `format` every chunk is encoded in that resampler step (at the model's rate: one convert launch for the round's rows):
        `AudioChunk.audio` holds int16 / uint8 samples and the chunks concatenate, element for element, to the encoded whole."""
        if self._dec is None:
            raise ValueError("submit_stream needs a batcher made with stream_chunk_frames=N")
        return self._enqueue(True, context, text, speaker, voice_match, max_audio_length_ms, seed, stream_id, prompt, prefix, sampler, session,
                             sample_rate, format)

    def _enqueue(self, _streaming: bool, context, text, speaker, voice_match, max_audio_length_ms, seed, stream_id, prompt, prefix, sampler=None,
                 session=None, sample_rate=None, fmt=None):
        max_frames = int(max_audio_length_ms / 80)
        sample_rate = self._rate(sample_rate, inward=False)
        if sample_rate is not None and not self.decode:
            raise ValueError("sample_rate= resamples the decoded audio: the batcher was made with decode=False")
        fmt = self._format(fmt)
        if fmt is not None and not self.decode:
            raise ValueError("format= encodes the decoded audio: the batcher was made with decode=False")
        if sampler is not None:
            if not self.row_samplers:
                raise ValueError("a per-request sampler needs a batcher made with row_samplers=True; this one samples every stream with its own")
            _check_sampler(sampler)
        elif self.row_samplers:
            sampler = self.sampler
        if session is not None:
            if context or prompt is not None or prefix is not None or voice_match:
                raise ValueError("session= carries the conversation: it excludes context, prompt, prefix and voice_match=True")
            if text is None:
                raise ValueError("a session's turn needs its own text")
            session._ready("submit")
            voice_match = False
            prompt = self.engine.session_prompt(session, text, speaker)
            prompt = (np.asarray(prompt[0], np.int32), np.asarray(prompt[1], np.float32))
            prefix = session.prefix
            length = int(session.n) + int(prompt[0].shape[0])
        elif prefix is not None:
            if context or prompt is not None or voice_match:
                raise ValueError("prefix= stands for the context of the non-voice_match layout: it excludes context, prompt and voice_match=True")
            if text is None:
                raise ValueError("a request on a prefix needs its own text")
            voice_match = False
            prompt = self.engine.prefixed_prompt(prefix, text, speaker)
            prompt = (np.asarray(prompt[0], np.int32), np.asarray(prompt[1], np.float32))
            length = int(prefix.length) + int(prompt[0].shape[0])
        elif prompt is not None:
            prompt = (np.asarray(prompt[0], np.int32), np.asarray(prompt[1], np.float32))
            length = int(prompt[0].shape[0])
        else:
            length = int(self.engine.prompt_length(context, text, speaker, True if voice_match is None else voice_match))
        limit = self.engine.max_pos - max_frames
        if length >= limit:
            raise ValueError(f"Inputs too long, must be below max_seq_len - max_audio_frames: {limit}"  # sesame.py:755-758
                             + ("; session.rebuild(keep_last_turns=k) re-prefills a shorter history" if session is not None else ""))
        if max_frames < 1 or length < 1:
            raise ValueError("a request needs a prompt and at least one frame")
        if _streaming and max_frames > self.stream_max_frames:
            raise ValueError(f"a streaming request of {max_frames} frames: the batcher was made for stream_max_frames = {self.stream_max_frames}")
        if self.rng == "device" and seed is None and self.row_samplers:
            seed = self.seed
        if self.rng == "device" and seed is not None and int(seed) != self.seed and not self.row_samplers:
            raise ValueError(f"rng 'device': every stream draws from the batcher's seed {self.seed}; streams differ by stream_id")
        if stream_id is not None and not 0 <= int(stream_id) < 2 ** 31:
            raise ValueError("stream_id must be in [0, 2^31)")
        fut: Future = Future()
        audio = CSMAudioStream(fut, self) if _streaming else None
        with self._lock:
            if self._closed:
                fut.set_exception(RuntimeError("CSMBatcher is closed"))
                return audio if _streaming else fut
            if session is not None:
                session._ready("submit")  # (again, under the lock: two threads on one session)
                session._turn = fut
            if stream_id is None:
                stream_id = self._next_id
            self._next_id = max(self._next_id, int(stream_id)) + 1
            self._queue.append(_Stream(future=fut, context=context, text=text, speaker=int(speaker),
                                       voice_match=True if voice_match is None else bool(voice_match),
                                       max_frames=max_frames, seed=seed, stream_id=int(stream_id), length=length, t0=time.perf_counter(),
                                       prompt=prompt, prefix=prefix, audio=audio, sampler=sampler, session=session, rate=sample_rate, fmt=fmt))
            if sample_rate is not None:
                self._rate_of[fut] = sample_rate
            if session is not None:
                session._stream = self._queue[-1]
            self._wake.notify()
        return audio if _streaming else fut

    # ---- stopping a request ------------------------------------------------------------------------------------------------
    def _control(self, handle, kind: str, frames: Optional[int]) -> bool:
        """A caller's thread: record the wish and wake the scheduler.  Nothing of the engine, the rows or the lanes is touched here."""
        fut = handle.future if isinstance(handle, CSMAudioStream) else handle
        if not isinstance(fut, Future):
            raise TypeError("cancel / interrupt take what submit / submit_stream returned")
        with self._lock:
            if fut.done():
                return False
            self._controls.append((fut, kind, frames))
            self._wake.notify()
        return True

    def cancel(self, handle) -> bool:
        """The request of `handle` (the `Future` of `submit`, the `CSMAudioStream` of `submit_stream`) did not happen.  Applied at the top of the
        scheduler's next round: a queued request is never admitted, one in a prefill lane leaves it, a live one has its row parked, without
        a capture; the row goes to the next queued request in that round.  Then `future.cancelled()` is true, `result()` and the stream's
        iterator raise `CancelledError`, and a session is what it was before the turn.  A plain `future.cancel()` has the same effect.
        False, and no effect, for a request that has already finished.  Any thread."""
        return self._control(handle, "cancel", None)

    def interrupt(self, handle, played_frames: Optional[int] = None, played_samples: Optional[int] = None) -> bool:
        """End the stream now and keep what was heard.  Heard: `played_frames`, or ceil(`played_samples` / samples per frame) -- a frame that was
        partly played counts --, or with neither the frames emitted so far (`submit_stream`) / generated so far (`submit`).  Kept: k = min(heard,
        the frames generated, the index of the first EOS frame, the request's limit).  A request made with `sample_rate=R` counts `played_samples` at R: p R-samples are p * model rate // R of the codec's.  Applied at the top of the scheduler's next round, with
        one poll.  k >= 1: the future resolves with a `StreamResult` of k frames and `interrupted=True`; a plain request decodes its k frames,
        a streaming one gets the chunks up to frame k it has not had yet -- the last with `final=True` -- or, when it has had them all,
        one `AudioChunk` of 0 frames with `final=True`, and its result's audio is what was emitted cut to k frames.  A session's turn is
        committed as a turn of k frames.  k = 0, a request still queued or in a prefill lane: as `cancel`.  False for a finished request.
        Any thread."""
        if played_frames is not None and played_samples is not None:
            raise ValueError("interrupt takes played_frames or played_samples, not both")
        heard = played_frames
        if played_samples is not None:
            with self._lock:
                rate = self._rate_of.get(handle.future if isinstance(handle, CSMAudioStream) else handle)
            if rate is not None:  # the caller counts what it played at the request's own rate
                played_samples = int(played_samples) * int(self.engine.sample_rate) // rate
            heard = -(-int(played_samples) // int(self.engine.samples_per_frame))
        if heard is not None and int(heard) < 0:
            raise ValueError("played_frames / played_samples must be >= 0")
        return self._control(handle, "interrupt", None if heard is None else int(heard))

    def _release(self, s: _Stream) -> None:
        """The stream's row is parked and free for the next admission."""
        self.engine.park(s.row)
        self._rows[s.row] = None
        s.held = False

    def _drop(self, s: _Stream) -> None:
        """A cancelled request leaves the scheduler: a live row is parked without a capture (its decoder row is reset by the next admission)."""
        if s.row >= 0 and self._rows[s.row] is s:
            self._release(s)
        s.held = False
        s.future.cancel()
        self.stats["cancelled"] += 1

    def _apply_controls(self) -> bool:
        """The scheduler's thread, at the top of a round: every request with a cancel wish or a cancelled future leaves the queue, its lane or
        its row; an interrupt lowers its stream's limit.  True when a stream was interrupted: the round polls at once."""
        with self._lock:
            controls, self._controls = self._controls, []
            wish: Dict[Future, list] = {}
            for fut, kind, frames in controls:
                wish.setdefault(fut, []).append((kind, frames))
            gone = [s for s in self._queue if s.future.cancelled() or s.future in wish]  # (an interrupt of a request nobody has heard yet: a cancel)
            for s in gone:
                self._queue.remove(s)
        for s in [s for s in self._inflight if s.future.cancelled() or s.future in wish]:
            self._inflight.remove(s)  # (the others keep their order; the lane's next prefill starts from a reset, behind this one on the side stream)
            self._lane_of[s.lane] = None
            gone.append(s)
        poll = False
        for s in self._live():
            w = wish.get(s.future)
            if s.future.cancelled() or (w is not None and any(kind == "cancel" for kind, _ in w)):
                gone.append(s)
            elif w is not None:
                so_far = s.emitted if s.audio is not None else len(s.codes)
                s.cut = min([so_far if frames is None else frames for _, frames in w] + ([s.cut] if s.cut is not None else []))
                poll = True
        for s in gone:
            self._drop(s)
        return poll

    # ---- one scheduling round -----------------------------------------------------------------------------------------------------------
    def _live(self) -> List[_Stream]:
        return [s for s in self._rows if s is not None]

    def _poll(self, keep_cadence: bool = False) -> None:
        """One sync: which streams have ended (EOS frame seen, their own frame limit, or an interrupt: `cut`), park their rows, decode,
        resolve.  keep_cadence: a poll an interrupt asked for between two regular ones, which come when they would have."""
        self.stats["polls"] += 1
        if not keep_cadence:
            self._since_poll = 0
        fe = self._first_eos.cpu().tolist() if self.stop_on_eos else [-1] * self.max_batch
        done: Dict[int, List[_Stream]] = {}
        streaming = [s for s in self._live() if s.audio is not None]
        for s in streaming:  # this poll confirms every frame generated so far, up to the EOS frame and the limit
            eos = fe[s.row]
            s.confirmed = min(eos if eos >= 0 else len(s.codes), s.max_frames)
            s.ended = eos >= 0 or len(s.codes) >= s.max_frames
            if s.cut is not None:  # interrupted: the stream ends here with what was heard of the confirmed frames
                s.decodable, s.confirmed, s.ended = s.confirmed, min(s.confirmed, s.cut), True
                if s.confirmed == 0:  # nothing was heard: the request did not happen
                    self._drop(s)
                    continue
            if s.ended:
                self._turn_end(s, s.confirmed)
                self._release(s)  # (the decoder row keeps its state until the next admission resets it: the tail is decoded below)
        if streaming:
            self._emit(streaming)
        for s in self._live():
            if s.audio is not None:
                continue
            eos = fe[s.row]
            if eos < 0 and len(s.codes) < s.max_frames and s.cut is None:
                continue
            count = min(eos if eos >= 0 else len(s.codes), s.max_frames)  # frames past the EOS frame / the limit are dropped
            if s.cut is not None:  # interrupted: and those that were not heard
                count = min(count, s.cut)
                if count == 0:  # nothing was heard: the request did not happen
                    self._drop(s)
                    continue
            self._turn_end(s, count)
            self._release(s)
            done.setdefault(count, []).append(s)
        for count, group in done.items():
            self.stats["finished"] += len(group)
            self.stats["interrupted"] += sum(s.cut is not None for s in group)
            if count == 0:
                for s in group:
                    _fail(s, AssertionError("No audio generated"))
                continue
            try:
                codes = torch.stack([torch.stack(s.codes[:count], dim=1) for s in group])  # [b, n_cb, T]
                pcm = self.engine.decode(codes) if self.decode else None
                if pcm is not None:
                    self.engine.synchronize()
                for j, s in enumerate(group):
                    audio = pcm[j] if pcm is not None else None
                    if s.fmt is not None:
                        audio = self._resample_clip(audio, s.rate, s.fmt)
                    elif s.rate is not None:
                        audio = self._resample_clip(audio, s.rate)
                    self._resolve(s, StreamResult(audio=audio, frames=count, codes=codes[j],
                                                  sample_rate=s.rate if s.rate is not None else self.engine.sample_rate, stream_id=s.stream_id, row=s.row,
                                                  processing_time_seconds=time.perf_counter() - s.t0, interrupted=s.cut is not None, **self._fmt_kw(s)))
            except Exception as e:  # noqa: BLE001
                for s in group:
                    _fail(s, e)

    # ---- sessions ----------------------------------------------------------------------------------------------------------
    def _turn_end(self, s: _Stream, count: int) -> None:
        """A session's turn has ended with `count` kept frames and its row is about to be parked: copy its K / V out first (a parked row has no
        window).  The copy becomes the session's prefix when the turn's result is ready (`_resolve`); if the turn fails on the way there it
        is destroyed and the session stays as it was."""
        if s.session is None or count == 0 or s.future.done():
            return
        try:
            s.captured = c = s.session._capture(s, count)
            self.stats["captures"] += 1
            s.future.add_done_callback(lambda f: c["prefix"].close() if f.cancelled() or f.exception() is not None else None)
        except Exception as e:  # noqa: BLE001
            s.capture_error = e

    def _resolve(self, s: _Stream, result: StreamResult) -> None:
        if not _claim(s.future):  # cancelled on the way here: nothing is committed (the capture is destroyed by its callback)
            return
        if s.capture_error is not None:
            s.future.set_exception(s.capture_error)
            return
        if s.captured is not None:
            s.session._commit(s.captured)  # before the result: whoever waits on it finds the session ready for the next turn
        s.future.set_result(result)

    # ---- streaming audio --------------------------------------------------------------------------------------------------
    def _emit(self, streams: List[_Stream]) -> None:
        """The aligned decode round of one poll.  Chunk k of a stream is its frames [kN, (k+1)N): it is decoded once a poll has confirmed one
        frame MORE (the stream goes on, so the chunk is not its last) or the stream's end (then `final` is known: when the length is a
        multiple of N the last full chunk carries it).  All rows with such a chunk go through one step(F=N); then the tails, grouped by r."""
        N = self.chunk
        while True:
            ready = [s for s in streams if not s.future.done() and s.emitted + N <= s.confirmed and (s.ended or s.emitted + N < s.confirmed)]
            if not ready:
                break
            self._decode_round(ready, N)
        tails: Dict[tuple, List[_Stream]] = {}
        for s in streams:
            if s.ended and not s.future.done() and 0 < s.confirmed - s.emitted:
                r = s.confirmed - s.emitted
                # An interrupted stream's last chunk goes through the step its chunk would have had -- the N frames if they exist -- and is cut
                # to the r frames that were heard: the codec is causal, so these are the samples the uninterrupted stream carries there.
                tails.setdefault((r, min(N, s.decodable - s.emitted) if s.cut is not None else r), []).append(s)
        for (r, F), group in tails.items():
            self._decode_round(group, F, keep=r)
        for s in streams:
            if not s.ended or s.future.done():
                continue
            self.stats["finished"] += 1
            if s.confirmed == 0:
                _fail(s, AssertionError("No audio generated"))
                continue
            audio = torch.cat(s.chunks)
            try:
                if s.cut is not None:
                    self.stats["interrupted"] += 1
                    if s.emitted >= s.confirmed:  # it has had every frame that was heard: the iterator ends behind a chunk of 0 frames
                        audio = audio[: s.confirmed * (audio.shape[0] // s.emitted)]
                        tail = audio[:0] if s.fmt is None else torch.zeros(0, dtype=PCM.torch_dtype(s.fmt), device=audio.device)
                        if s.rate is not None and not s.rflushed and s.emitted == s.confirmed:
                            # the cut is where the emitted chunks end: the row is flushed now and the 0-frame chunk carries the filter's tail
                            n_in, flush = [0] * self.max_batch, [False] * self.max_batch
                            flush[s.row] = True
                            out, n_out = self._ors.step(torch.zeros((self.max_batch, 4), dtype=torch.float32, device=self.engine.device), n_in, flush)
                            tail = self._rs_out(self._ors, out, s.row, n_out[s.row]).clone()
                            s.rchunks.append(tail)
                            s.rflushed = True
                        s.audio._q.put(AudioChunk(audio=tail, first_frame=s.confirmed, frames=0, final=True, **self._fmt_kw(s)))
                if s.rate is None and s.fmt is not None:
                    # At the model's rate the encoding is element-wise: the encoded chunks, cut where the kept audio ends, are the encoded whole.
                    audio = torch.cat(s.rchunks)[: audio.shape[0]]
                elif s.rate is not None and s.fmt is not None:
                    audio = torch.cat(s.rchunks) if s.rflushed else self._resample_clip(audio, s.rate, s.fmt)
                elif s.rate is not None:
                    # Flushed with its last chunk: the chunks are the whole.  An interrupted stream that was cut INSIDE what it had been sent
                    # cannot be flushed (its row has consumed samples behind the cut): its result is the resample of the 24 kHz audio that was
                    # kept, as a plain request's is, and its chunks do not add up to it.
                    audio = torch.cat(s.rchunks) if s.rflushed else self._resample_clip(audio, s.rate)
            except Exception as e:  # noqa: BLE001
                _fail(s, e)
                continue
            self._resolve(s, StreamResult(audio=audio, frames=s.confirmed, codes=torch.stack(s.codes[: s.confirmed], dim=1),
                                          sample_rate=s.rate if s.rate is not None else self.engine.sample_rate, stream_id=s.stream_id, row=s.row,
                                          processing_time_seconds=time.perf_counter() - s.t0, interrupted=s.cut is not None, **self._fmt_kw(s)))

    @staticmethod
    def _fmt_kw(s: _Stream) -> dict:
        return {"format": s.fmt} if s.fmt is not None else {}

    def _decode_round(self, group: List[_Stream], F: int, keep: Optional[int] = None) -> None:
        """One step of the row decoder: F frames for the rows of `group`, the other rows inactive; the chunks carry the first `keep` of them
        (all, but for an interrupted stream's last chunk).  A failure fails the group's requests (their iterators raise) and frees their
        rows; the other streams go on."""
        keep = F if keep is None else keep
        try:
            codes = torch.zeros((self.max_batch, self.engine.n_cb, F), dtype=torch.int32, device=self.engine.device)
            active = [False] * self.max_batch
            for s in group:
                codes[s.row] = torch.stack(s.codes[s.emitted : s.emitted + F], dim=1)
                active[s.row] = True
            pcm = self._dec.step(codes, active)
            rated = [s for s in group if s.rate is not None]
            if rated:  # ONE resampler step for the round's rows with a rate: the kept samples in, the final chunk flushes
                n_in, flush = [0] * self.max_batch, [False] * self.max_batch
                for s in rated:
                    n_in[s.row], flush[s.row] = keep * (pcm.shape[-1] // F), s.ended and s.emitted + keep == s.confirmed
                out, n_out = self._ors.step(pcm[:, 0, :], n_in, flush)
            coded = [s for s in group if s.rate is None and s.fmt is not None]
            if coded:  # ONE convert launch for the round's rows with a format at the model's rate: the kept samples, encoded
                fmts, cnt = ["f32"] * self.max_batch, [0] * self.max_batch
                for s in coded:
                    fmts[s.row], cnt[s.row] = s.fmt, keep * (pcm.shape[-1] // F)
                enc = self._cvt.convert(pcm[:, 0, :], ["f32"] * self.max_batch, fmts, cnt)
            self.engine.synchronize()
            self.stats["chunk_rounds"] += 1
            for s in group:
                chunk = AudioChunk(audio=pcm[s.row, 0, : keep * (pcm.shape[-1] // F)].clone(), first_frame=s.emitted, frames=keep,
                                   final=s.ended and s.emitted + keep == s.confirmed)
                s.chunks.append(chunk.audio)
                if s.rate is not None:
                    chunk.audio = self._rs_out(self._ors, out, s.row, n_out[s.row]).clone()
                    s.rchunks.append(chunk.audio)
                    s.rflushed = flush[s.row]
                elif s.fmt is not None:
                    chunk.audio = PCM.view(enc, s.row, s.fmt)[: cnt[s.row]].clone()
                    s.rchunks.append(chunk.audio)
                if s.fmt is not None:
                    chunk.format = s.fmt
                s.emitted += keep
                if s.audio.first_audio_seconds is None:
                    s.audio.first_audio_seconds = time.perf_counter() - s.t0
                self.stats["chunks"] += 1
                s.audio._q.put(chunk)
        except Exception as e:  # noqa: BLE001
            for s in group:
                _fail(s, e)
                if self._rows[s.row] is s:
                    self._release(s)

    def _resample_clip(self, audio: torch.Tensor, rate: Optional[int], fmt: Optional[str] = None) -> torch.Tensor:
        """A whole clip at the model's rate -> `rate`: one step with the flush on a one-row resampler the batcher keeps, on the batch's stream.
        The same kernel and bits as `resample.resample`, without that call's allocations and its synchronisation.  `fmt`: the step encodes
        its outputs; without a rate there is no ratio and the clip goes through one convert launch instead."""
        if rate is None:
            if self._cvt is None:
                self._cvt = self.engine.pcm_converter()
            y = self._cvt.convert(audio.reshape(1, -1), ["f32"], [fmt], [int(audio.shape[0])])
            return PCM.view(y, 0, fmt)[: int(audio.shape[0])].clone()
        if self._crs is None:
            self._crs = self.engine.row_resampler(1, 1 << 30)
        if fmt is None:
            self._crs.set_row(0, self.engine.sample_rate, rate)
        else:
            self._crs.set_row(0, self.engine.sample_rate, rate, out_format=fmt)
        y, n = self._crs.step(audio.reshape(1, -1), [int(audio.shape[0])], [True])
        return self._rs_out(self._crs, y, 0, n[0]).clone()

    def _out_row(self, s: _Stream, row: int) -> None:
        """A streaming request with a rate is admitted: its resampler row is the cache row, and a new stream starts in it."""
        if s.rate is None:
            if s.fmt is not None and self._cvt is None:  # at the model's rate its chunks go through the stateless converter
                self._cvt = self.engine.pcm_converter()
            return
        if self._ors is None:
            self._ors = self.engine.row_resampler(self.max_batch, self.chunk * int(self.engine.samples_per_frame))
        if s.fmt is None:
            self._ors.set_row(row, self.engine.sample_rate, s.rate)
        else:
            self._ors.set_row(row, self.engine.sample_rate, s.rate, out_format=s.fmt)

    def _timed(self, what: str, fn) -> None:
        if self.profile:
            self.engine.synchronize()
            t = time.perf_counter()
            fn()
            self.engine.synchronize()
            self.stats[what + "_seconds"] += time.perf_counter() - t
        else:
            fn()

    def _shift(self, delta: int) -> None:
        self._timed("shift", lambda: self.engine.shift(delta))
        self.stats["shifts"] += 1
        self.stats["shifts_down" if delta < 0 else "shifts_up"] += 1

    def _draws(self, s: _Stream):
        """(sampler, first-frame uniforms, device seed) of a request's admission; a sampled host-rng stream gets its generator here."""
        u = None
        sampler = s.sampler if self.row_samplers else self.sampler  # the request's own: its admission block, then its row's table entry
        sampled = float(sampler.temp) > 0 if self.row_samplers else self._sampled
        if sampled and self.rng == "host":  # (a greedy stream has no generator: it consumes no draws, as its solo run)
            s.rng = np.random.default_rng(s.seed)
            u = s.rng.uniform(size=(1, self.engine.n_cb))[0].astype(np.float32)
        seed = (s.seed if self.row_samplers else self.seed) if (sampled and self.rng == "device") else None
        return sampler, u, seed

    # ---- admissions off the batch's stream -----------------------------------------------------------------------------------
    def _begin_prefills(self) -> bool:
        """Queue heads go to free lanes, in queue order, whether or not a cache row is free.  Host work and launches on the side stream only."""
        began = False
        while None in self._lane_of:
            with self._lock:
                s = self._queue.popleft() if self._queue else None
            if s is None:
                break
            if s.future.cancelled():
                self._drop(s)
                continue
            began = True
            lane = self._lane_of.index(None)
            try:
                if s.prompt is None:
                    s.prompt = self.engine.prompts([s])[0]
                S = int(s.prompt[0].shape[0]) + (int(s.prefix.length) if s.prefix is not None else 0)
                if S != s.length:
                    raise ValueError(f"the prompt has {S} frames, {s.length} were announced")
                sampler, u, seed = self._draws(s)
                s.admit_args = (sampler, seed)
                s.prefill = self.engine.prefill(lane, s.prompt, sampler, u, seed, s.stream_id, prefix=s.prefix, timed=self.profile)
            except Exception as e:  # noqa: BLE001  (the lane stays free: its next prefill starts from a reset)
                _fail(s, e)
                continue
            s.lane = lane
            self._lane_of[lane] = s
            self._inflight.append(s)
        return began

    def _commit_ready(self) -> bool:
        """The oldest request in a lane enters a free row once its prefill has completed; never a later one in front of it.  While rows are
        live the lane is only asked (`event.query()`), so the frames go on; with nothing live there is nothing to stall and the batcher waits."""
        done = False
        while self._inflight:
            free = [r for r in range(self.max_batch) if self._rows[r] is None]
            if not free:
                break
            s, row = self._inflight[0], free[0]
            try:
                if not self.engine.prefill_ready(s.prefill, wait=not self._live()):
                    break
            except Exception as e:  # noqa: BLE001
                self._drop_prefill(s, e)
                done = True
                continue
            self._inflight.popleft()
            self._lane_of[s.lane] = None
            done = True
            moved = False
            try:
                _, P = self.engine.row_state()
                if not self._live() and P != s.length:
                    self._shift(s.length - P)   # nothing live: only the position moves
                elif s.length > P:
                    self._shift(s.length - P)   # the live windows move up so that the admission fits below the position
                out: List[torch.Tensor] = []
                self._timed("commit", lambda: out.append(self.engine.commit(row, s.lane, s.prefill)))
                moved = True
                if self.row_samplers:
                    self.engine.set_row_sampler(row, *s.admit_args)
                if s.audio is not None:
                    self._dec.reset_row(row)  # the decoder row is the cache row: a new stream starts in it
                    self._out_row(s, row)
                if self.profile:
                    self.stats["prefill_seconds"] += self.engine.prefill_seconds(s.prefill)
            except Exception as e:  # noqa: BLE001
                _fail(s, e)
                if moved:
                    self.engine.park(row)
                continue
            self.stats["overlapped_admissions"] += 1
            self._seat(s, row, out[0])
        return done

    def _drop_prefill(self, s: _Stream, e: BaseException) -> None:
        if self._inflight and self._inflight[0] is s:
            self._inflight.popleft()
        else:
            self._inflight.remove(s)
        self._lane_of[s.lane] = None
        _fail(s, e)

    def _seat(self, s: _Stream, row: int, codes: torch.Tensor) -> None:
        """The request's stream is live in `row` with `codes` as its first frame."""
        self.stats["admissions"] += 1
        self.stats["prefixed_admissions"] += s.prefix is not None
        self.stats["session_admissions"] += s.session is not None
        s.row = row
        s.codes = [codes]
        self._rows[row] = s
        self._prev[row] = codes
        self._first_eos[row] = torch.where((codes == 0).all(), 0, -1)
        self._local[row] = 1

    def _admit(self) -> None:
        if self.overlap:
            # Commits only, while rows are live: the next queue heads go to the lanes BEHIND the round's frame launch (`step`), so that the
            # batch's stream has a frame to run while the host enqueues a prompt block on the side stream.  With nothing live and nothing in
            # a lane there is no frame to put in front: the heads start now and the first is waited for.
            while self._commit_ready() | (not self._live() and not self._inflight and self._begin_prefills()):
                pass
            return
        free = [r for r in range(self.max_batch) if self._rows[r] is None]
        with self._lock:
            new = [self._queue.popleft() for _ in range(min(len(free), len(self._queue)))]
        for s in [s for s in new if s.future.cancelled()]:  # (cancelled since the top of the round: no prompt is built for it)
            new.remove(s)
            self._drop(s)
        if not new:
            return
        need = [s for s in new if s.prompt is None]
        try:
            for s, p in zip(need, self.engine.prompts(need) if need else []):
                s.prompt = p
        except Exception as e:  # noqa: BLE001
            for s in need:
                _fail(s, e)
            new = [s for s in new if s.prompt is not None]
        for s, row in zip(new, free):
            S = int(s.prompt[0].shape[0]) + (int(s.prefix.length) if s.prefix is not None else 0)  # the whole prompt: what must fit below P
            try:
                if S != s.length:
                    raise ValueError(f"the prompt has {S} frames, {s.length} were announced")
                _, P = self.engine.row_state()
                if not self._live() and P != S:
                    self._shift(S - P)       # nothing live: only the position moves
                elif S > P:
                    self._shift(S - P)       # the live windows move up so that the prompt fits below the position
                sampler, u, seed = self._draws(s)
                out: List[torch.Tensor] = []
                if s.prefix is not None:
                    self._timed("admit", lambda: out.append(self.engine.admit(row, s.prompt, sampler, u, seed, s.stream_id, prefix=s.prefix)))
                else:
                    self._timed("admit", lambda: out.append(self.engine.admit(row, s.prompt, sampler, u, seed, s.stream_id)))
                codes = out[0]
                if self.row_samplers:
                    self.engine.set_row_sampler(row, sampler, seed)
            except Exception as e:  # noqa: BLE001
                _fail(s, e)
                continue
            if s.audio is not None:
                try:
                    self._dec.reset_row(row)  # the decoder row is the cache row: a new stream starts in it
                    self._out_row(s, row)
                except Exception as e:  # noqa: BLE001
                    _fail(s, e)
                    self.engine.park(row)
                    continue
            self._seat(s, row, codes)

    def _frame(self) -> None:
        if not (self.overlap and self.profile):
            return self._frame_step()
        # profile: the step's time, booked by whether a prefill was in flight on the side stream from its start to its end
        before = [self.engine.prefill_ready(s.prefill) for s in self._inflight]
        self.engine.synchronize()
        t = time.perf_counter()
        self._frame_step()
        self.engine.synchronize()
        dt = time.perf_counter() - t
        after = [self.engine.prefill_ready(s.prefill) for s in self._inflight]
        if not all(after):
            self.stats["frames_prefill_in_flight"] += 1
            self.stats["frame_seconds_prefill_in_flight"] += dt
        elif all(before):
            self.stats["frames_no_prefill"] += 1
            self.stats["frame_seconds_no_prefill"] += dt

    def _frame_step(self) -> None:
        live = self._live()
        pad, P = self.engine.row_state()
        if P >= self.engine.max_pos:  # the position has reached the end of the cache: every live window moves down to slot 0 of the longest
            self._shift(-min(pad[s.row] for s in live))
        if self.row_samplers:  # every row's settings come from its table entry: one uniform source for the batcher's life, one captured graph
            u, ids = None, None
            if self.rng == "host":  # a greedy stream's row (and a parked one) is a constant: only sampled streams draw
                u = np.full((self.max_batch, self.engine.n_cb), 0.5, np.float32)
                for s in live:
                    if s.rng is not None:
                        u[s.row] = s.rng.uniform(size=(1, self.engine.n_cb))[0]
            else:
                ids = [self._rows[r].stream_id if self._rows[r] is not None else 0 for r in range(self.max_batch)]
            sample = self.engine.frame(self._prev, "rows", u, None, ids, device_rng=self.rng == "device").clone()
        else:
            sample = self._frame_one_sampler(live)
        self._prev = sample
        if self.stop_on_eos:
            zero = (sample == 0).all(dim=1)  # an all-zero frame is EOS (sesame.py:765-766)
            self._first_eos = torch.where((self._first_eos < 0) & zero, self._local, self._first_eos)
        self._local = self._local + 1
        for s in live:
            s.codes.append(sample[s.row])
        self.stats["frames"] += 1
        self.stats["live_row_frames"] += len(live)
        self._since_poll += 1

    def _frame_one_sampler(self, live: List[_Stream]) -> torch.Tensor:
        """The frame step with the batcher's sampler for every row (launch arguments)"""
        u = None
        if self._sampled and self.rng == "host":
            u = np.full((self.max_batch, self.engine.n_cb), 0.5, np.float32)
            for s in live:
                u[s.row] = s.rng.uniform(size=(1, self.engine.n_cb))[0]
        seed = self.seed if (self._sampled and self.rng == "device") else None
        ids = [self._rows[r].stream_id if self._rows[r] is not None else 0 for r in range(self.max_batch)] if seed is not None else None
        return self.engine.frame(self._prev, self.sampler, u, seed, ids).clone()  # (graph replay hands back a view of a persistent buffer)

    def step(self) -> bool:
        """One scheduling round; False when there was nothing to do (no live stream, empty queue, no listen round due)."""
        self._listen_consume()  # (before the controls: a barge-in's interrupt is applied in the round that sees the onset)
        now = self._apply_controls()  # (before the admissions: a row a cancel has freed is refilled in this round)
        heard = self._listen_round()  # due listen rounds are work, with or without a live row
        if self._stt is not None:
            heard = self._stt_round() or heard  # (the round's final spans are cut and submitted, then `stt` is stepped: its work is due work)
        while True:
            self._admit()  # (rows a poll has just freed are refilled in the same round)
            live = self._live()
            due = self._since_poll >= self.interval or any(len(s.codes) >= s.max_frames for s in live)
            if not (live and (due or now)):
                break
            if due:
                self._poll()
            else:
                self._poll(keep_cadence=True)
            now = False
        if not self._live():
            return heard
        self._frame()
        if self.overlap:
            self._begin_prefills()  # (also the lane a commit of this round has freed)
        return True

    def run_until_idle(self) -> None:
        while self.step() or self._queue or self._inflight:
            pass

    @property
    def occupancy(self) -> float:
        """live row-frames / computed row-frames of the single-token steps so far"""
        return self.stats["live_row_frames"] / max(1, self.stats["frames"] * self.max_batch)

    # ---- background thread --------------------------------------------------------------------------------------------------------------
    def start(self) -> "CSMBatcher":
        with self._lock:
            if self._closed:
                raise RuntimeError("CSMBatcher is closed")
            if self._thread is None:
                self._thread = threading.Thread(target=self._worker, name="csm-batcher", daemon=True)
                self._thread.start()
        return self

    def _worker(self) -> None:
        while True:
            with self._lock:
                while (not self._closed and not self._queue and not self._live() and not self._inflight and not self._controls
                       and not self._listen_due() and not self._stt_has_work()):
                    self._wake.wait()
                if self._closed:
                    return
            try:
                self.step()
            except Exception as e:  # noqa: BLE001  (a failed round fails the streams in flight, the thread lives on)
                for s in self._live():
                    _fail(s, e)
                    self._release(s)

    def close(self) -> None:
        """Stop the worker.  Requests still queued or in flight are FAILED, never dropped (their callers sit in Future.result()); the
        closed flag and the queue change under one lock, so a submit() that races close() either lands in the queue before the flag --
        and is failed here -- or sees the flag and fails at once.  A request with a `cancel` still pending is cancelled instead; a pending
        `interrupt` is not applied (no round runs any more) and its request fails like the others."""
        with self._lock:
            self._closed = True
            self._wake.notify_all()
            thread, self._thread = self._thread, None
        if thread is not None:
            thread.join()
        with self._lock:
            pending = list(self._queue)
            self._queue.clear()
            unwanted = {fut for fut, kind, _ in self._controls if kind == "cancel"}
            self._controls = []
        held = list(self._inflight)  # prefilled or being prefilled in a lane, not committed
        self._inflight.clear()
        self._lane_of = [None] * len(self._lane_of)
        for s in pending + held + self._live():
            if s.future in unwanted:
                s.future.cancel()
            _fail(s, RuntimeError("CSMBatcher is closed"))
        for s in self._live():
            self._release(s)
        if self._dec is not None:
            self._dec.close()
        self._listen_close()  # (every listener is told, the encoder and the listening objects are closed -- the shared converter with them)
        for rs in (self._ors, self._crs):
            if rs is not None:
                rs.close()
        if self.overlap:
            self.engine.close_lanes()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
