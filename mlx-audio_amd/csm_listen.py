"""The listening edge of CSM serving: what concerns a microphone and never a cache row.  `ListenMixin` is the scheduler's half (methods of
`CSMBatcher`), `CSMListener` the caller's; csm_continuous.py builds the always-open microphone on the steps both kinds share.

Listening: `CSMBatcher(..., listen_rows=K)` and `batcher.listen()` / `sess.listen(speaker)`.  A `CSMListener` takes microphone
audio in arbitrary slices (`feed`, any thread, host work only) -- also while the session's own turn is live, which is what a barge-in is -- and
the scheduler tokenises it as it arrives in a row-mode streaming ENCODER (`Mimi.row_encoder`: one position and lifetime per row, independent of
the cache rows).  The steps of a listener's stream are fixed by its length alone, [M] * (T // M) + [T % M] with M = listen_chunk_frames, so its
codes never depend on timing or slicing: they equal a fresh batch-1 `Mimi.encode_step` stream over its zero-padded pcm in those steps.  These
are streaming-encoder codes, NOT those of `Mimi.encode(clip)` (whose transformer sees the whole clip without a mask).  `end(text)` resolves
with a `ListenResult`; for a session's listener the turn has entered the history by then exactly as `hear(Segment(...), codes=codes)` does.

Other sample rates: `listen(sample_rate=R)`.  A listener is then fed at R: the scheduler uploads each row's new samples once
per round, resamples them into a per-row device buffer at the model's rate (`resample.RowResampler`: one launch for all listeners, a position
per row) and encodes from that buffer; its codes are those of a listener fed `resample(clip, R, model rate)`, whatever the slicing.
Without a rate nothing of this exists: no resampler is made.

PCM formats: `listen(format="mulaw")` with or without a rate (`pcm.FORMATS`: "f32", "s16le", "mulaw", "alaw").  A listener with
a format is fed bytes (or an array of the format's dtype), keeps them in that format and uploads them once per round; they are decoded inside
the resampler step (a listener with a rate) or by one convert launch (`pcm.RowConverter`, a listener at the model's rate) into the same
per-row device buffer, so its codes are those of an f32 listener fed `pcm.decode(the bytes)`.  Counts (`listen_max_frames`,
`ListenResult.samples`) stay in samples.  Without a format nothing of this exists: no converter is made and every call is the one it was.

Endpointing and barge-in: `listen(vad=VadConfig())`, `sess.listen(speaker, vad=..., barge_in=True)`.  Behind the round's resampler /
convert launches ONE detector step (`vad.RowVad`: the reference's energy rule and listener loop) classifies every VAD listener's new whole
frames in its device buffer; the status table travels to pinned host memory behind an event and is consumed at the top of a later round, so no
round waits for it.  A VAD listener's encoder stream is heard[start:], nothing of it is encoded before the onset, and while it is open only
steps below what the consumed status has made certain; at an endpoint (`lis.endpoint`) or at `end()` the span heard[start:stop] is final and
the rest is encoded, zeros behind `stop`: codes, frames and steps are those of a plain listener fed heard[start:stop] and ended.  `lis.onset`
resolves with the onset; with `barge_in` that round interrupts the session's turn through the controls of 8d-8.
Without `vad=` nothing of this exists: no detector is made and a listen round is the launches it was.

Always-open microphones: `listen(vad=..., continuous=True)` (csm_continuous.py).  One listener yields utterance after
utterance (`CSMUtterance`) from a ring on the device, a detector that re-arms behind every endpoint and a host queue that a silent microphone
never fills.  Without `continuous=True` nothing of it exists.

Speech to text: `CSMBatcher(..., stt=whisper_model.serve(...))` and `listen(transcribe=True | DecodingOptions | dict)`.  In the round
in which a transcribing listener's span becomes final -- a VAD endpoint, `end()` and the covering status, `end()` and the flush of a listener
without a detector (its span is everything it heard), a continuous utterance's endpoint -- the scheduler cuts the Whisper windows of ALL the
round's spans out of the device buffers in ONE launch pair (`engine.span_windows`: `_heard` rows for the one-shot listeners, the rings at their
64-bit stream positions for the continuous ones), encodes them in ONE `embed_audio` call and submits each row's features to `stt` with the
listener's options; `lis.transcript` / `utt.transcript` (a `Future[DecodingResult]`) resolves when Whisper's does, with what
`whisper_model.decode(window, options)` returns for that window alone.  The scheduler steps `stt` itself, `stt_rounds_per_round` times per round
at the most, so `stt` must not have a thread of its own.  With `stt_text=` (DecodingResult -> what `end(text)` takes) a session's listener may
`end()` without text: the heard turn waits for the transcript.  Without `stt=` nothing of this exists."""
from __future__ import annotations

from collections import deque
from concurrent.futures import Future, InvalidStateError
from dataclasses import dataclass
from typing import Deque, List, Optional

import numpy as np
import torch

from . import pcm as PCM
from . import resample as RS
from . import vad as VAD


@dataclass
class ListenResult:
    """What a listener's `end()` resolves with.  `codes` are streaming-encoder codes (`Mimi.encode_step` in `steps`), not `Mimi.encode`'s."""
    codes: torch.Tensor  # [n_cb, frames] int32
    frames: int          # T = ceil(samples / samples per frame): a partial last frame is zero-padded
    samples: int         # samples fed
    steps: List[int]     # the encoder steps of this stream: [M] * (T // M) + [T % M]
    sample_rate: int = 0  # the rate the samples were fed at; with `listen(sample_rate=R)` T = ceil(out_len(samples) / samples per frame)
    format: str = "f32"   # the format the samples were fed in (`listen(format=)`); `samples` counts samples, not bytes
    speech_start: Optional[int] = None  # a listener made with `vad=`: the samples [speech_start, speech_stop) at the model's rate of what was
    speech_stop: Optional[int] = None   # fed are what `codes` encode; None for a listener without a detector


@dataclass
class SpeechSpan:
    """What a VAD listener's `endpoint` future resolves with: the utterance is over.  Samples and frames at the model's rate; the same span
    counted at the rate the listener is fed at in `rate_start` / `rate_stop` (floor / ceil)."""
    start: int           # the first sample kept: the onset frame's first sample less the pre-roll
    stop: int            # one past the last sample kept
    onset_frame: int     # the first speech frame, in detector frames
    endpoint_frame: int  # the silent frame that made the count pass the hang
    sample_rate: int = 0  # the listener's own rate
    rate_start: int = 0
    rate_stop: int = 0
    forced: bool = False  # a continuous listener's utterance that the length limit closed, not the silence


def _speech_span(sp, onset_frame: int, endpoint_frame: int, rate: Optional[int], sr: int, fed: Optional[int] = None, forced: bool = False) -> SpeechSpan:
    """The span `sp` = (start, stop) at the model's rate `sr`, counted at the listener's own `rate` as well; fed: a one-shot listener's
    samples, which `rate_stop` never passes."""
    R = rate if rate is not None else sr
    stop = -(-sp[1] * R // sr)
    return SpeechSpan(start=sp[0], stop=sp[1], onset_frame=onset_frame, endpoint_frame=endpoint_frame, sample_rate=R,
                      rate_start=sp[0] * R // sr, rate_stop=stop if fed is None else min(fed, stop), forced=forced)


def _claim(fut: Future) -> bool:
    """True: the future is the scheduler's to finish and a `cancel()` can no longer succeed; False: it is cancelled (or finished)."""
    if fut.running():
        return True
    return not fut.done() and fut.set_running_or_notify_cancel()


def _fail_future(fut: Optional[Future], e: Optional[BaseException]) -> None:
    """A pending future fails with `e` (None: it is cancelled); one that was cancelled or has resolved meanwhile stays as it is."""
    if fut is not None and e is None:
        fut.cancel()
    elif fut is not None:
        try:
            fut.set_exception(e)
        except InvalidStateError:
            pass


class _Heard:
    """What the encoder records one stream into, and what `end(text)` resolves: the part a `CSMListener` and a `CSMUtterance` share."""

    def __init__(self, batcher):
        self.batcher = batcher
        self.frames = 0                       # encoded
        self.steps: List[int] = []
        self._codes: List[torch.Tensor] = []  # one [n_cb, F] device tensor per step
        self._fresh = True                    # the encoder row is reset before this stream's first step
        self._future: Optional[Future] = None
        self._text = None
        # speech to text: None without `transcribe=`
        self.transcript: Optional[Future] = None  # -> whisper DecodingResult of the span's window
        self._topts = None                    # the checked DecodingOptions
        self._tcut = False                    # the span's window has been cut (or the transcript has failed before)
        self._twf: Optional[Future] = None    # the Whisper request's own future, once submitted

    def _transcribes(self, options) -> None:
        self.transcript, self._topts = Future(), options

    def _text_ready(self, session) -> bool:
        """Under the lock: an ended stream's text is there -- given, or (a session's `end()` without text) its transcript has resolved."""
        return self._text is not None or session is None or self.transcript is None or self.transcript.done()

    def codes(self) -> torch.Tensor:
        """The codes encoded so far, [n_cb, frames] int32 on the host (a copy from the device)."""
        with self.batcher._lock:
            parts = list(self._codes)
        if not parts:
            return torch.zeros((self.batcher.engine.n_cb, 0), dtype=torch.int32)
        return torch.cat(parts, dim=1).cpu()

    def _took(self, codes: torch.Tensor, F: int) -> None:
        """Under the lock: an encoder step of F frames was this stream's."""
        self._codes.append(codes)
        self.steps.append(F)
        self.frames += F

    def _begin_end(self, session, text) -> Future:
        """`end(text)`: the refusals, then the future the scheduler resolves; a session is busy from here to the result."""
        b = self.batcher
        with b._lock:
            if b._closed:
                raise RuntimeError("CSMBatcher is closed")
            self._end_refused()
            if session is not None:
                if text is None and (self.transcript is None or b._stt_text is None):
                    raise ValueError("end: a session's heard turn needs its text")
                session._ready("end")
            fut: Future = Future()
            self._text = text
            if session is not None:
                session._hearing = fut
            self._future = fut
            b._wake.notify()
        return fut


def _vacate(lis) -> None:
    """Under the lock: the listener's row of `_listeners` is the next caller's."""
    lis._open = False
    if lis.batcher._listeners[lis.row] is lis:
        lis.batcher._listeners[lis.row] = None


class CSMListener(_Heard):
    """What `CSMBatcher.listen` / `CSMSession.listen` return: one microphone.  `feed(pcm)` from any thread, `frames` / `codes()` for what
    has been tokenised so far, `end(text)` for the `Future[ListenResult]`, `cancel()` to drop it.  It holds one row of the batcher's row-mode
    streaming encoder from `listen` until the result (or `cancel`)."""

    def __init__(self, batcher, row: int, speaker: int, session=None, sample_rate: Optional[int] = None, fmt: Optional[str] = None,
                 vad: Optional[VAD.VadConfig] = None, barge_in: bool = False, transcribe=None):
        super().__init__(batcher)
        self.row, self.speaker, self.session = int(row), int(speaker), session
        if transcribe is not None:
            self._transcribes(transcribe)
        # voice activity: the detector's settings, or None -- then nothing below `barge_in` is ever touched
        self.vad, self.barge_in = vad, bool(barge_in)
        self.onset: Optional[Future] = Future() if vad is not None else None     # -> the first kept sample at the model's rate, once speech began
        self.endpoint: Optional[Future] = Future() if vad is not None else None  # -> SpeechSpan, once the speaker has finished
        self._vset = False                    # the detector row holds this listener's stream
        self._vsent = 0                       # the `_n24` of the last detector step that took the row
        self._vst = VAD.NO_STATUS             # the last status the scheduler consumed, and ...
        self._vn = 0                          # ... the `_n24` it covers
        self._vstart: Optional[int] = None    # the encoder's stream is heard[_vstart:], once an onset was consumed
        self._vstop: Optional[int] = None     # ... and ends at heard[_vstop], once the span is final (`_vclosed`)
        self._vclosed = False                 # an endpoint was consumed, or `end()` and the status that covers everything fed
        self.spf = int(batcher.engine.samples_per_frame)
        self.rate = sample_rate               # None: fed at the model's rate; else the scheduler resamples what is fed
        self.fmt = fmt                        # None: fed float32; else the samples are kept and uploaded in this format
        # the encoder reads this listener from its device buffer at the model's rate (a transcribing one: the window is cut out of that buffer)
        self._dev = sample_rate is not None or fmt is not None or vad is not None or transcribe is not None
        cap = batcher.listen_max_frames * self.spf
        if self.rate is not None:             # the most samples at `rate` whose out_len fits the row: N L <= cap M
            L, M = RS.ratio(self.rate, batcher.engine.sample_rate)
            cap = cap * M // L
        self._pcm = np.zeros(cap, PCM.dtype(fmt))  # (f32: zeros behind `samples`, the padding of a partial last frame)
        self._up = 0                          # a rate or format listener: samples handed to the resampler / converter, ...
        self._n24 = 0                         # ... samples at the model's rate its device buffer holds, ...
        self._flushed = False                 # ... and whether the resampler row has been flushed (the stream has ended and is whole)
        self.samples = 0                      # fed
        self._open = True                     # False once cancelled or resolved: the row is someone else's

    @property
    def ended(self) -> bool:
        return self._future is not None

    def _total(self) -> int:
        """Frames the stream holds for the scheduler: whole frames while it is open, ceil once it has ended.  A rate listener: of the
        samples its device buffer holds -- ready(fed) while it is open, out_len(fed) once it has been flushed."""
        if self.vad is not None:
            return self._vad_total()
        if self._dev:
            return -(-self._n24 // self.spf) if self._flushed else self._n24 // self.spf
        return -(-self.samples // self.spf) if self.ended else self.samples // self.spf

    def _vad_total(self) -> int:
        """A VAD listener's frames: of heard[start:stop] once the span is final; while it is open only the whole frames below
        B = min(classified fl, (last_speech + 1) fl + keep) - start, which the final span can only grow beyond; none before an onset."""
        if self._vstart is None:
            return 0
        if self._vclosed:
            return -(-(self._vstop - self._vstart) // self.spf)
        sp = VAD.span(self.vad, self._vst, self._vn, False, self.batcher.engine.sample_rate)
        return max(0, sp[1] - self._vstart) // self.spf

    def _unresampled(self) -> bool:
        """Under the lock: the scheduler's next round has samples of this listener to resample, or its flush."""
        return self._dev and not self._vclosed and (self._up < self.samples or (self.ended and not self._flushed))

    def _vad_due(self) -> bool:
        """Under the lock: the detector has new samples of this listener to classify, or `end()` has come and the status that covers
        everything fed has been consumed: the scheduler's next round closes it."""
        if self.vad is None or self._vclosed:
            return False
        return (self._vset and self._vsent != self._n24) or (self.ended and self._flushed and self._vn == self._n24)

    def feed(self, pcm) -> None:
        """Mono float32 at the listener's sample rate (the model's, or the `sample_rate` it was made with), any number of samples.  Host
        work only: the samples join a buffer under the batcher's lock and an idle scheduler is woken.  ValueError, with nothing changed, when
        the total -- at the model's rate: out_len of it -- would pass `listen_max_frames`.
        A listener made with `format=`: `bytes`, `bytearray`, `memoryview` or a numpy array of the format's dtype, a whole number of samples
        (an "s16le" feed of an odd number of bytes is a ValueError, nothing changed; no byte is carried to the next feed)."""
        if self.fmt is not None or isinstance(pcm, (bytes, bytearray, memoryview)):
            a = PCM.samples(pcm, self.fmt)
        else:
            a = np.asarray(pcm, np.float32).reshape(-1)
        b = self.batcher
        with b._lock:
            if b._closed:
                raise RuntimeError("CSMBatcher is closed")
            if not self._open or self.ended:
                raise ValueError("feed: the listener has ended or was cancelled")
            if self._vclosed:  # behind a detected endpoint: accepted and ignored
                return
            if self.samples + a.shape[0] > self._pcm.shape[0]:
                raise ValueError(f"feed: {self.samples + a.shape[0]} samples are more than listen_max_frames = {b.listen_max_frames} frames")
            self._pcm[self.samples : self.samples + a.shape[0]] = a
            self.samples += int(a.shape[0])
            b._wake.notify()

    def _end_refused(self) -> None:
        if not self._open or self.ended:
            raise ValueError("end: the listener has ended or was cancelled")
        if self.samples == 0:
            raise ValueError("end: nothing was fed")

    def end(self, text=None) -> Future:
        """No more audio; a partial last frame is zero-padded.  The future resolves with the `ListenResult` once the scheduler has encoded the
        rest and freed the encoder row.  A session's listener: `text` is the turn's transcript, and the turn enters the session's history
        before the future resolves, as `hear(Segment(speaker, text, audio), codes=codes)` would put it.  Refused (ValueError, the listener
        stays open) while the session's turn is queued or live, as `hear` is; from here to the result the session is busy."""
        return self._begin_end(self.session, text)

    def cancel(self) -> bool:
        """Drop the buffered audio and free the encoder row; a pending `end()` future is cancelled and the session is as it was.  False when
        the listener has already finished."""
        with self.batcher._lock:
            if not self._open:
                return False
            _vacate(self)
        self._shut(None)
        return True

    def _leave(self) -> None:
        """The row is the next caller's; a VAD listener that leaves without onset or endpoint: whoever waits is told."""
        with self.batcher._lock:
            _vacate(self)
        for f in (self.onset, self.endpoint):
            if f is not None:
                f.cancel()

    def _shut(self, e: Optional[BaseException]) -> None:
        """The listener leaves before its result: a pending `end()` fails with `e` (None: it is cancelled), one that never ended just stops."""
        self._leave()
        _fail_future(self._future, e)
        _drop_transcript(self, e)


def _drop_transcript(h: _Heard, e: Optional[BaseException]) -> None:
    """A transcript that is still owed fails with `e` (None: it is cancelled).  A Whisper request that is queued is cancelled with it; one in
    flight runs out and its result is dropped."""
    if h.transcript is not None and not h.transcript.done():
        _fail_future(h.transcript, e)
        if h._twf is not None:
            h._twf.cancel()


class ListenMixin:
    """The scheduler's half of listening (methods of `CSMBatcher`, which brings `engine`, `_lock`, `_wake`, `_closed`, `_controls`, `stats`
    and `_timed`).  `CSMBatcher` itself calls `_listen_init`, `_listen_consume`, `_listen_round`, `_listen_due` and `_listen_close` only."""

    LISTEN_IN = 1 << 15  # samples per row and resampler step: a long clip fed at once takes several steps in its round

    def _listen_init(self, listen_rows: int, listen_chunk_frames: int, listen_max_frames: int) -> None:
        self.listen_rows, self.listen_chunk, self.listen_max_frames = int(listen_rows), int(listen_chunk_frames), int(listen_max_frames)
        self._enc = None
        self._listeners: List[Optional[CSMListener]] = [None] * self.listen_rows  # per encoder row (under the lock)
        if self.listen_rows > 0:
            self.stats.update(listen_rounds=0, listen_frames=0, listen_seconds=0.0)
            self._enc = self.engine.row_encoder(self.listen_rows, self.listen_max_frames, self.listen_chunk)
        # other sample rates: made by the scheduler when the first listener with a rate needs them, never before
        self._lrs = None                       # the listeners' resampler, one row per encoder row
        self._heard: Optional[torch.Tensor] = None  # [listen_rows, listen_max_frames * spf]: what the device listeners' rows hold at the model's rate
        self._cvt = None                       # PCM formats at the model's own rate: one stateless converter, made with the first such row (in or out)
        self._vad = None                       # voice activity: one detector row per encoder row, made with the first VAD listener
        self._vad_n = [0] * self.listen_rows   # per detector row: the n_avail of its last step (a row no step takes is handed the same again)
        self._vad_out: Deque[tuple] = deque()  # (ticket, {row: (listener, the `_n24` covered)}): status tables on their way to the host

    def _listen_close(self) -> None:
        """`CSMBatcher.close`, the worker has stopped: every listener's row is taken, whoever waits on one is told, the objects are closed."""
        if self._stt is not None:
            self._stt_close()
        with self._lock:
            listeners = [lis for lis in self._listeners if lis is not None]
        self._vad_out.clear()
        for lis in listeners:
            lis._shut(RuntimeError("CSMBatcher is closed"))
        for obj in (self._enc, self._lrs, self._cvt, self._vad):
            if obj is not None:
                obj.close()

    def listen(self, speaker: int = 0, session=None, sample_rate: Optional[int] = None,
               format: Optional[str] = None, vad=None, barge_in: bool = False, continuous: bool = False, transcribe=None):
        """A microphone (`CSMListener`) on a free row of the batcher's streaming encoder; ValueError when all `listen_rows` are taken (or
        the batcher was made without any).  `session`: what `CSMSession.listen` passes.  `sample_rate`: the rate `feed` takes (None: the
        model's); ValueError for a rate the resampler does not take.  `format` (`pcm.FORMATS`; None or "f32": float32): what `feed` takes --
        "s16le", "mulaw" or "alaw" bytes; ValueError for another name.  Any thread; nothing of the device is touched.
        `vad` (`vad.VadConfig`, or True for the reference's defaults): the scheduler runs a voice-activity detector over what
        the listener is fed, on the device and at the model's rate.  Nothing is encoded before the speaker's onset (`lis.onset`, a
        `Future[int]`: the first kept sample); after `silence_ms` of silence `lis.endpoint` resolves with a `SpeechSpan` and later feeds are
        ignored; `end(text)` -- before or after the endpoint -- resolves with the `ListenResult` of a plain listener fed
        heard[speech_start:speech_stop] and ended, or fails with ValueError("no speech").  `barge_in` (a session's listener): the onset
        interrupts the session's queued or live turn in the round that sees it.
        `continuous` (needs `vad`): the microphone stays open -> a `CSMContinuousListener`: one `CSMUtterance` per detected
        utterance, each with its own `onset`, `endpoint` and `end(text)`, until `close()`.
        `transcribe` (True, a whisper `DecodingOptions` or a dict of its fields; needs a batcher made with `stt=`):
        `lis.transcript` (every utterance's `utt.transcript`) is a `Future[DecodingResult]` of the span's Whisper window, decoded greedily with
        these options beside whatever else `stt` runs.  The options are checked here, with `whisper_decoding.verify_options`' exceptions."""
        topts = self._stt_options(transcribe)
        if continuous and (vad is None or vad is False):
            raise ValueError("listen: continuous=True needs vad=")
        if self._enc is None:
            raise ValueError("listen needs a batcher made with listen_rows=K")
        sample_rate = self._rate(sample_rate, inward=True)
        fmt = self._format(format)
        if vad is None or vad is False:
            vad = None
            if barge_in:
                raise ValueError("listen: barge_in needs vad=")
        else:
            vad = VAD.VadConfig() if vad is True else vad
            if not isinstance(vad, VAD.VadConfig):
                raise ValueError("listen: vad takes a vad.VadConfig or True")
            vad.frame_len(self.engine.sample_rate)  # (ValueError for a frame the detector does not take)
            if barge_in and session is None:
                raise ValueError("listen: barge_in needs a session's listener (CSMSession.listen)")
        if session is not None and session.batcher is not self:
            raise ValueError("the session belongs to another batcher (CSMBatcher.session on this batcher)")
        with self._lock:
            if self._closed:
                raise RuntimeError("CSMBatcher is closed")
            free = [r for r in range(self.listen_rows) if self._listeners[r] is None]
            if not free:
                raise ValueError(f"all {self.listen_rows} listen rows are taken")
            if continuous:  # (csm_continuous.ContinuousMixin)
                extra = {} if topts is None else {"transcribe": topts}
                lis = self._listeners[free[0]] = self._cont_listen(free[0], speaker, session, sample_rate, fmt, vad, barge_in, **extra)
                return lis
            extra = {} if vad is None else {"vad": vad, "barge_in": barge_in}
            if topts is not None:
                extra["transcribe"] = topts
            lis = self._listeners[free[0]] = CSMListener(self, free[0], speaker, session, sample_rate, fmt, **extra)
        return lis

    @staticmethod
    def _format(fmt) -> Optional[str]:
        """A caller's `format` checked where it is given: None for None and for "f32" (today's path), else the name."""
        return None if PCM.check(fmt) == "f32" else fmt

    def _rate(self, sample_rate, inward: bool) -> Optional[int]:
        """A caller's `sample_rate` checked where it is given: None for None and for the model's own rate (today's path), else the rate."""
        if sample_rate is None or int(sample_rate) == int(self.engine.sample_rate):
            return None
        RS.ratio(sample_rate, self.engine.sample_rate) if inward else RS.ratio(self.engine.sample_rate, sample_rate)
        return int(sample_rate)

    @staticmethod
    def _rs_out(rs, y, row: int, n: int) -> torch.Tensor:
        """Row `row`'s `n` new outputs of a resampler step: of a float32 y as they are, of a byte y (a row of the object has a format) as the
        row's own dtype."""
        return y[row, :n] if y.dtype == torch.float32 else rs.out_view(y, row)[:n]

    # ---- the steps both kinds of microphone share ----------------------------------------------------------------------------------------------
    def _shots(self) -> List[CSMListener]:
        """Under the lock: the open one-shot listeners (the counterpart of `_cont_mics`)."""
        return [lis for lis in self._listeners if isinstance(lis, CSMListener) and lis._open]

    def _listen_made(self, work) -> None:
        """The scheduler's thread: the resampler, the converter and the device buffer, each made when the first of `work` needs it."""
        if self._lrs is None and any(lis.rate is not None for lis in work):
            self._lrs = self.engine.row_resampler(self.listen_rows, self.LISTEN_IN)
        if self._cvt is None and any(lis.rate is None for lis in work):
            self._cvt = self.engine.pcm_converter()
        if self._heard is None:
            self._heard = torch.zeros((self.listen_rows, self.listen_max_frames * work[0].spf), dtype=torch.float32, device=self.engine.device)

    def _listen_set_row(self, lis) -> None:
        """The scheduler's thread: a new stream starts in the listener's resampler row, if it has a rate.  (Two forms of the call: an
        engine without formats does not take `in_format`.)"""
        if lis.rate is not None and lis.fmt is None:
            self._lrs.set_row(lis.row, lis.rate, self.engine.sample_rate)
        elif lis.rate is not None:
            self._lrs.set_row(lis.row, lis.rate, self.engine.sample_rate, in_format=lis.fmt)

    def _listen_stage(self, pairs, as_bytes: bool) -> torch.Tensor:
        """The scheduler's thread: (row, samples) pairs as one staging array on the device -- the rows' bytes, each in its own format (1, 2
        or 4 per sample; rows of 16-byte multiples), or float32 samples (rows of 4-sample multiples)."""
        if as_bytes:
            x = np.zeros((self.listen_rows, max(16, -(-max(a.nbytes for _, a in pairs) // 16) * 16)), np.uint8)
            for row, a in pairs:
                x[row, : a.nbytes] = a.view(np.uint8)
        else:
            x = np.zeros((self.listen_rows, max(4, -(-max(a.shape[0] for _, a in pairs) // 4) * 4)), np.float32)
            for row, a in pairs:
                x[row, : a.shape[0]] = a
        return torch.from_numpy(x).to(self.engine.device)

    def _encode_step(self, group, F: int, fill) -> None:
        """The scheduler's thread: one step of the row encoder, F frames for the (row, `_Heard`) pairs of `group`, the other rows inactive.
        A stream's first step resets its row (zero carried state, position 0, the edge fill on this step); `fill()` then hands the step's
        input [listen_rows, 1, F * spf].  The caller fails the group when this raises."""
        active = [False] * self.listen_rows
        for row, h in group:
            if h._fresh:
                self._enc.reset_row(row)
                h._fresh = False
            active[row] = True
        x = fill()
        out: List[torch.Tensor] = []
        self._timed("listen", lambda: out.append(self._enc.step(x, active)))
        self.stats["listen_rounds"] += 1
        self.stats["listen_frames"] += F * len(group)
        with self._lock:
            for row, h in group:
                h._took(out[0][row].clone(), F)

    def _barge_in(self, lis) -> None:
        """Under the lock: a `barge_in` listener's onset records the interrupt of its session's queued, prefilling or live turn, which ends
        with what it has emitted (`interrupt`) when this same round's `_apply_controls` applies it."""
        turn = lis.session._turn if (lis.barge_in and lis.session is not None) else None
        if turn is not None and not turn.done():
            self._controls.append((turn, "interrupt", None))

    def _heard_turn(self, h: _Heard, lis, audio, fields: dict, error: Optional[str] = None, release=None) -> None:
        """The scheduler's thread: a stream that was ended has all its frames.  A session's heard turn enters the history -- `audio()`: its
        samples at the model's rate, what `hear` takes -- BEFORE the result: whoever waits on it finds the turn there.  `release()` lets go
        of the stream on every way out, ahead of the future; fields: what the `ListenResult` says beyond codes, frames and steps."""
        fut, release = h._future, release or (lambda: None)
        if not _claim(fut):
            return release()
        try:
            if error is not None:
                raise ValueError(error)  # (the session is as it was: nothing was heard)
            codes = torch.cat(h._codes, dim=1)
            if lis.session is not None:
                if lis.session._closed:
                    raise ValueError("end: the session is closed")
                host = codes.cpu().numpy()  # (synchronises: the codes are the session's prompt frames from here on)
                text = h._text if h._text is not None else self._stt_text(h.transcript.result())  # (`end()` without text: a failed transcript fails the turn)
                lis.session._hear(self.engine.heard_segment(lis.speaker, text, audio()), host)
            release()
            fut.set_result(ListenResult(codes=codes, frames=h.frames, steps=list(h.steps), **fields))
        except Exception as e:  # noqa: BLE001
            release()
            fut.set_exception(e)
            if lis.session is not None and lis.session._closed:
                lis.session.close()  # (closed while it was busy with this listener: its prefix is freed now)

    # ---- the one-shot listeners' round -------------------------------------------------------------------------------------------
    def _listen_plan(self):
        """Under the lock: (rows with >= M frames not yet encoded, ended rows by remainder 0 < r < M, ended rows with nothing left).  A rate
        listener counts as ended only once its resampler row has been flushed: `end()` may come from another thread between the round's
        resampler step and this plan, and until the next round's step has taken the rest of its samples and the flush, `_total()` is not
        its length yet."""
        M = self.listen_chunk
        full, tails, done = [], {}, []
        for lis in self._shots():
            left = lis._total() - lis.frames
            ended = lis.ended and (not lis._dev or lis._flushed)
            whole = ended  # the stream's length is final: its remainder may be encoded
            if lis.vad is not None:  # the span is final at an endpoint or at `end()`; the result waits for the caller's `end()`
                whole, ended = lis._vclosed, lis._vclosed and lis.ended
            if left >= M:
                full.append(lis)
            elif whole and left > 0:
                tails.setdefault(left, []).append(lis)
            elif ended and lis._text_ready(lis.session):  # (a session's `end()` without text waits for its transcript)
                done.append(lis)
        return full, tails, done

    def _listen_due(self) -> bool:
        """Under the lock: a listen round is due."""
        if self._enc is None:
            return False
        full, tails, done = self._listen_plan()
        if self._vad_out or any(lis._vad_due() for lis in self._shots()):
            return True  # a status on its way to the host, or samples the detector has not seen, are work due
        return bool(full or tails or done) or any(lis._unresampled() for lis in self._shots())

    def _listen_resample(self) -> bool:
        """The scheduler's thread, at the top of a listen round: every rate listener's new samples go up once and through ONE
        resampler step into the row's buffer at the model's rate; a listener that has ended is flushed.  What the round then encodes is
        counted from those buffers (`CSMListener._total`), so the frames follow from the samples fed and never from the slicing.
        Formats: a listener's new samples go up as the bytes it was fed.  With a rate they are decoded in that resampler step;
        at the model's rate ONE convert launch decodes the round's rows into the same buffers."""
        with self._lock:
            work = [(lis, lis.samples, lis.ended) for lis in self._shots() if lis._unresampled()]
        if not work:
            return False
        try:
            self._listen_made([lis for lis, _, _ in work])
            if self._vad is None and any(lis.vad is not None for lis, _, _ in work):
                self._vad = self.engine.row_vad(self.listen_rows)
        except Exception as e:  # noqa: BLE001
            for lis, _, _ in work:
                lis._shut(e)
            return True
        for item in list(work):
            lis = item[0]
            if lis._up == 0 and lis._n24 == 0 and not lis._flushed:  # a new stream starts in the row: zero history, zero counts, zeros behind
                try:
                    self._listen_set_row(lis)
                    self._heard[lis.row].zero_()
                    if lis.vad is not None:
                        sr = self.engine.sample_rate
                        self._vad.set_row(lis.row, lis.vad.frame_len(sr), lis.vad.thr2n(sr), lis.vad.hang_frames)
                        self._vad_n[lis.row], lis._vset = 0, True
                except Exception as e:  # noqa: BLE001  (this row's own failure: the others go on)
                    work.remove(item)
                    lis._shut(e)
        rated = [w for w in work if w[0].rate is not None]
        plain = [w for w in work if w[0].rate is None]
        try:
            while True:
                todo = [(lis, min(self.LISTEN_IN, fed - lis._up), ended) for lis, fed, ended in rated if lis._up < fed or (ended and not lis._flushed)]
                if not todo:
                    break
                n_in, flush = [0] * self.listen_rows, [False] * self.listen_rows
                for lis, k, ended in todo:
                    n_in[lis.row], flush[lis.row] = k, ended and lis._up + k == lis.samples
                x = self._listen_stage([(lis.row, lis._pcm[lis._up : lis._up + k]) for lis, k, _ in todo], any(lis.fmt is not None for lis, _, _ in todo))
                y, n_out = self._lrs.step(x, n_in, flush)
                for lis, k, _ in todo:
                    n = n_out[lis.row]
                    self._heard[lis.row, lis._n24 : lis._n24 + n] = self._rs_out(self._lrs, y, lis.row, n)
                    with self._lock:
                        lis._up, lis._n24, lis._flushed = lis._up + k, lis._n24 + n, flush[lis.row]
        except Exception as e:  # noqa: BLE001  (the shared step: it fails the rows that took part in it, as an encode step fails its group)
            for lis, _, _ in rated:
                lis._shut(e)
        try:
            todo = [(lis, fed - lis._up, ended) for lis, fed, ended in plain]
            if any(k > 0 for _, k, _ in todo):  # ONE convert launch: the rows' bytes -> float32 at the model's rate
                fmts, n = ["f32"] * self.listen_rows, [0] * self.listen_rows
                for lis, k, _ in todo:
                    fmts[lis.row], n[lis.row] = lis.fmt or "f32", k  # (f32 at the model's rate: a VAD listener, whose samples must be in the device buffer)
                x = self._listen_stage([(lis.row, lis._pcm[lis._up : lis._up + k]) for lis, k, _ in todo], True)
                y = self._cvt.convert(x, fmts, ["f32"] * self.listen_rows, n)
                for lis, k, _ in todo:
                    self._heard[lis.row, lis._n24 : lis._n24 + k] = PCM.view(y, lis.row, "f32")[:k]
            for lis, k, ended in todo:
                with self._lock:
                    lis._up, lis._n24, lis._flushed = lis._up + k, lis._n24 + k, ended  # (ended with this snapshot: these were its last samples)
        except Exception as e:  # noqa: BLE001
            for lis, _, _ in plain:
                lis._shut(e)
        return True

    def _listen_consume(self) -> None:
        """The scheduler's thread, at the top of a round, before the controls: a barge-in's interrupt is applied in the round that sees the onset."""
        if self._vad is not None:
            self._vad_consume()

    def _listen_round(self) -> bool:
        """The scheduler's thread, once per scheduling round: ONE encode step of M frames for every row that holds M frames not yet encoded,
        then one step per distinct remainder r for the ended rows whose remainder is due, then the ended rows with nothing left resolve.  A
        listener's steps are therefore [M] * (T // M) + [T % M] whatever the slicing and the timing of its `feed` calls.  False when there
        was nothing to do: due listen rounds are work, with or without a live row."""
        if self._enc is None:
            return False
        fresh = self._listen_resample()
        if self._vad is not None and (self._vad_step() or self._vad_out):
            fresh = True
        if self._stt is not None:
            self._stt_mark_shots()  # (before anything of this round can finish a listener and hand its row on)
        with self._lock:
            full, _, _ = self._listen_plan()
        if full:
            self._encode_round(full, self.listen_chunk)
        with self._lock:
            _, tails, _ = self._listen_plan()  # (after the full round: a row it brought to its remainder goes on in this round)
        for r in sorted(tails):
            self._encode_round(tails[r], r)
        with self._lock:
            _, _, done = self._listen_plan()
        for lis in done:
            self._listen_finish(lis)
        return bool(full or tails or done or fresh)

    def _encode_round(self, group: List[CSMListener], F: int) -> None:
        """One step of the row encoder for the listeners of `group`.  A failure fails them."""
        def fill():
            pcm = np.zeros((self.listen_rows, 1, F * spf), np.float32)
            for lis in group:
                if not lis._dev:
                    pcm[lis.row, 0] = lis._pcm[lis.frames * spf : (lis.frames + F) * spf]  # (zeros behind the fed samples)
            x = torch.from_numpy(pcm)
            rated = [lis for lis in group if lis._dev]
            if rated:  # their samples are on the device already, at the model's rate (zeros behind what the resampler / converter wrote)
                x = x.to(self.engine.device)
                for lis in rated:
                    if lis.vad is None:
                        x[lis.row, 0] = self._heard[lis.row, lis.frames * spf : (lis.frames + F) * spf]
                        continue
                    # a VAD listener's stream is heard[start:stop]: zeros, not the samples the buffer holds there, behind `stop`
                    a = lis._vstart + lis.frames * spf
                    b = a + F * spf if not lis._vclosed else min(a + F * spf, lis._vstop)
                    x[lis.row, 0, : b - a] = self._heard[lis.row, a:b]
            return x

        try:
            spf = group[0].spf
            self._encode_step([(lis.row, lis) for lis in group], F, fill)
        except Exception as e:  # noqa: BLE001
            for lis in group:
                lis._shut(e)

    def _listen_finish(self, lis: CSMListener) -> None:
        """An ended listener has all its frames: free its row, enter a session's heard turn, resolve."""
        def audio():
            if lis.vad is not None:
                return self._heard[lis.row, lis._vstart : lis._vstop].cpu().numpy()
            return lis._pcm[: lis.samples].copy() if not lis._dev else self._heard[lis.row, : lis._n24].cpu().numpy()

        lis._leave()
        span = {} if lis.vad is None else {"speech_start": lis._vstart, "speech_stop": lis._vstop}
        fields = dict(samples=lis.samples, sample_rate=lis.rate if lis.rate is not None else int(self.engine.sample_rate),
                      **({"format": lis.fmt} if lis.fmt is not None else {}), **span)
        self._heard_turn(lis, lis, audio, fields, error="no speech" if lis.vad is not None and lis._vstart is None else None)

    # ---- speech to text -------------------------------------------------------------------------------------------------------
    def _stt_init(self, stt, rounds_per_round: int, stt_text) -> None:
        self._stt, self._stt_text = None, None
        self._stt_rounds = None
        self._stt_due = None   # spans that became final in this round: (holder, listener row, ring length or 0, start, samples)
        self._stt_owed = None  # holders whose Whisper request has been submitted and has not resolved
        if stt is None:
            if stt_text is not None:
                raise ValueError("stt_text needs stt=")
            return
        if int(rounds_per_round) < 1:
            raise ValueError("stt_rounds_per_round must be >= 1")
        if stt_text is not None and not callable(stt_text):
            raise ValueError("stt_text must be a callable: DecodingResult -> what end(text) takes")
        if getattr(stt, "_thread", None) is not None:
            raise ValueError("stt must not have been start()ed: the CSM scheduler steps it on its own thread and stream")
        if getattr(stt, "closed", False):
            raise ValueError("stt is closed")
        self._stt, self._stt_text, self._stt_rounds = stt, stt_text, int(rounds_per_round)
        self._stt_due, self._stt_owed = [], []
        self.stats.update(stt_cuts=0, stt_windows=0, stt_rounds=0, stt_cut_seconds=0.0)
        stt.on_submit = self._stt_poke  # a window the caller submits to `stt` directly wakes this scheduler, which steps it

    def _stt_poke(self) -> None:
        with self._lock:
            self._wake.notify()

    def _stt_options(self, transcribe):
        """A caller's `transcribe` checked where it is given: None for None and False, else the DecodingOptions `submit` will take."""
        if transcribe is None or transcribe is False:
            return None
        if self._stt is None:
            raise ValueError("listen: transcribe= needs a batcher made with stt=")
        from .whisper_decoding import DecodingOptions, verify_options

        if transcribe is True:
            transcribe = DecodingOptions()
        elif isinstance(transcribe, dict):
            transcribe = DecodingOptions(**transcribe)
        elif not isinstance(transcribe, DecodingOptions):
            raise ValueError("listen: transcribe takes True, a whisper DecodingOptions or a dict of its fields")
        return verify_options(transcribe)

    def _stt_has_work(self) -> bool:
        """`stt` has queued or live requests, or spans wait for their cut: due work."""
        if self._stt is None:
            return False
        with self._stt._lock:
            queued = bool(self._stt._queue)
        return queued or bool(self._stt_due) or any(r is not None for r in self._stt._rows)

    def _stt_mark(self, spans) -> None:
        """Spans that became final, (holder, listener row, ring length or 0, start or None, samples): their windows are cut by this round's
        `_stt_round`; a span without speech fails its transcript like `end()`."""
        for it in spans:
            if it[3] is None or it[4] < 1:
                _fail_future(it[0].transcript, ValueError("no speech"))
            else:
                with self._lock:
                    self._stt_due.append(it)

    def _stt_mark_shots(self) -> None:
        """The one-shot listeners whose span became final: a detector's [start, stop), or all a listener without one has heard."""
        spans = []
        with self._lock:
            for lis in self._shots():
                if lis.transcript is None or lis._tcut:
                    continue
                if lis.vad is not None and lis._vclosed:
                    spans.append((lis, lis.row, 0, lis._vstart, (lis._vstop or 0) - (lis._vstart or 0)))
                elif lis.vad is None and lis.ended and lis._flushed:
                    spans.append((lis, lis.row, 0, 0, lis._n24))
            for it in spans:
                it[0]._tcut = True
        self._stt_mark(spans)

    def _stt_round(self) -> bool:
        """The scheduler's thread, once per scheduling round behind the listen round: the round's final spans become Whisper windows in ONE
        `span_windows` launch pair and ONE `embed_audio` call and are submitted in row order; then `stt` is stepped, `stt_rounds_per_round`
        times at the most, while it has queued or live requests.  False when there was nothing to do."""
        with self._lock:
            due, self._stt_due = self._stt_due, []
        if due:
            self._stt_cut(sorted(due, key=lambda it: it[1]))
        n = 0
        while n < self._stt_rounds and self._stt_has_work():
            self._stt.step()
            n += 1
        self.stats["stt_rounds"] += n
        self._stt_owed = [h for h in self._stt_owed if not h.transcript.done()]
        return bool(due) or n > 0

    def _stt_cut(self, due) -> None:
        from . import whisper as WH
        from ._lib import WHISPER_MAX_ROWS

        stt = self._stt
        d = stt.engine.dims
        W, sr = 2 * int(d.n_audio_ctx), int(self.engine.sample_rate)
        rows = []
        for it in due:
            h, row, _, _, n = it
            try:
                L, M = WH.span_ratio(sr)
                if WH.span_len16(n, L, M) > W * WH.HOP_LENGTH:
                    raise ValueError(f"transcribe: the utterance of listen row {row} is {WH.span_len16(n, L, M)} samples at 16 kHz, more than the "
                                     f"{W * WH.HOP_LENGTH} of one Whisper window (long-form decoding of listeners is not built)")
            except ValueError as e:
                _fail_future(h.transcript, e)
                continue
            if not h.transcript.done():  # (cancelled meanwhile)
                rows.append(it)
        for at in range(0, len(rows), WHISPER_MAX_ROWS):
            chunk = rows[at : at + WHISPER_MAX_ROWS]
            try:
                out: List[torch.Tensor] = []
                spans = [(self._heard[row], ring_len, start, n) for _, row, ring_len, start, n in chunk]
                self._timed("stt_cut", lambda: out.append(stt.engine.embed_audio(self.engine.span_windows(spans, W, int(d.n_mels)))))
                feats = out[0]
            except Exception as e:  # noqa: BLE001  (the shared launch: it fails the rows that took part in it)
                for it in chunk:
                    _fail_future(it[0].transcript, e)
                continue
            self.stats["stt_cuts"] += 1
            self.stats["stt_windows"] += len(chunk)
            for i, (h, _, _, _, _) in enumerate(chunk):
                try:
                    h._twf = stt.submit(feats[i], h._topts)
                except Exception as e:  # noqa: BLE001  (this row's own refusal: the others go on)
                    _fail_future(h.transcript, e)
                    continue
                self._stt_owed.append(h)
                h._twf.add_done_callback(lambda wf, h=h: self._stt_done(h, wf))

    def _stt_done(self, h: _Heard, wf: Future) -> None:
        """Whisper's future has resolved (on the thread that stepped `stt`: this scheduler's): so does the transcript, unless it was dropped."""
        if h.transcript.done():
            return
        if wf.cancelled():
            h.transcript.cancel()
            return
        e = wf.exception()
        try:
            if e is not None:
                h.transcript.set_exception(e)
            else:
                h.transcript.set_result(wf.result())
        except InvalidStateError:
            pass
        with self._lock:
            self._wake.notify()  # (a session's `end()` without text may be waiting for it)

    def _stt_close(self) -> None:
        """`CSMBatcher.close`: `stt` stays open and is the caller's again; the transcripts still owed fail."""
        self._stt.on_submit = None
        with self._lock:
            due, self._stt_due = self._stt_due, []
        for h in [it[0] for it in due] + self._stt_owed:
            _drop_transcript(h, RuntimeError("CSMBatcher is closed"))
        self._stt_owed = []

    # ---- voice activity -----------------------------------------------------------------------------------------------------
    def _vad_step(self) -> bool:
        """The scheduler's thread, behind the round's resampler / convert launches: ONE detector step over the listeners' device buffers for
        every VAD row that holds samples the detector has not seen, then the status table starts its way to pinned host memory (`fetch`: a
        copy and an event, nothing waits).  The status is consumed at the top of a later round (`_vad_consume`)."""
        with self._lock:
            rows = [lis for lis in self._shots() if lis.vad is not None and lis._vset and not lis._vclosed and lis._vsent != lis._n24]
            if not rows:
                return False
            n = list(self._vad_n)
            for lis in rows:
                n[lis.row] = lis._n24
        try:
            self._vad.step(self._heard, n)
            self._vad_n = n  # (the detector's own counts have moved, whatever becomes of the hand-back)
            ticket = self._vad.fetch()
        except Exception as e:  # noqa: BLE001  (the shared step: it fails the rows that took part in it)
            for lis in rows:
                lis._shut(e)
            return True
        with self._lock:
            for lis in rows:
                lis._vsent = n[lis.row]
        self._vad_out.append((ticket, {lis.row: (lis, n[lis.row]) for lis in rows}))
        return True

    def _vad_consume(self) -> None:
        """The scheduler's thread, at the top of a round: every status table that has landed (`ready()`, no sync) becomes its listeners'
        state.  An onset resolves `lis.onset` and, with `barge_in`, records an interrupt of the session's turn, which this same round's
        `_apply_controls` applies.  An endpoint, or `end()` and the status that covers everything fed, makes the span final."""
        while self._vad_out and self._vad_out[0][0].ready():
            ticket, covered = self._vad_out.popleft()
            table = ticket.take()
            with self._lock:
                for row, (lis, n24) in covered.items():
                    if lis._open and self._listeners[row] is lis and not lis._vclosed:
                        lis._vst, lis._vn = tuple(int(v) for v in table[row]), n24
        with self._lock:
            mine = [lis for lis in self._shots() if lis.vad is not None and not lis._vclosed]
        sr = int(self.engine.sample_rate)
        for lis in mine:
            _, o, _, e = lis._vst
            if lis._vstart is None and o >= 0:
                start = VAD.span(lis.vad, lis._vst, lis._vn, False, sr)[0]
                with self._lock:
                    lis._vstart = start
                    self._barge_in(lis)
                if _claim(lis.onset):
                    lis.onset.set_result(start)
            with self._lock:
                final = e >= 0 or (lis.ended and lis._flushed and lis._vn == lis._n24)
                if not final:
                    continue
                sp = VAD.span(lis.vad, lis._vst, lis._n24, True, sr)
                lis._vstop = sp[1] if sp is not None else 0
                lis._vclosed = True
            if e >= 0 and _claim(lis.endpoint):
                lis.endpoint.set_result(_speech_span(sp, o, e, lis.rate, sr, fed=lis.samples))
            elif e < 0:
                lis.endpoint.cancel()  # the caller ended the listener first: there was no endpoint
