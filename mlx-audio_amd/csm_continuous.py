"""Always-open microphones for CSM serving: `batcher.listen(vad=..., continuous=True)` and
`sess.listen(speaker, vad=..., continuous=True, barge_in=...)`.

One listener lives as long as the call does.  Its row of the batcher's device buffer at the model's rate is a RING of
`listen_max_frames * samples_per_frame` samples; the stream S = resample(pcm.decode(everything fed)) is numbered from 0 in Python integers
and sample p lives at ring[p % ring_len].  Per round and whatever the number of such listeners: one resampler step or convert launch per
kind of row, one ring write (`ring.write_rows`), one detector step (`vad.RingVad`, which re-arms behind every utterance) and one ring read
(`ring.read_rows`) per encode step.  `feed` joins a host queue that is drained as samples go up, so a silent microphone never fills up.

Upload gate: samples go up only while n24 (the samples at the model's rate the ring has taken) stays below keep_from + ring_len, where
keep_from = max(0, min(start of the oldest utterance not yet finished, classified * frame_len - pre_roll)) of the last CONSUMED status
(`vad.keep_from`).  The status lags the device, so the gate is conservative; what does not fit waits in the host queue, and since the
encoder reads positions, never arrival times, codes do not depend on when a sample goes up.

Each detected utterance is a `CSMUtterance`, made in the round that consumes its onset (or its record, when it closed inside one step).
Contract: the utterances are those of `vad.utterances` on S, and utterance u resolves with the codes, frames and steps of a plain listener
at the model's rate fed S[start_u:stop_u] and ended."""
from __future__ import annotations

import queue
from collections import deque
from concurrent.futures import Future
from typing import Deque, List, Optional

import numpy as np
import torch

from . import pcm as PCM
from . import resample as RS
from . import vad as VAD
from .csm_listen import ListenMixin, _claim, _drop_transcript, _fail_future, _Heard, _speech_span, _vacate

_END = object()  # what the utterance queue holds behind the last utterance of a closed microphone


class CSMUtterance(_Heard):
    """One utterance of a continuous listener.  `onset`: its first kept sample at the model's rate (the onset frame's first sample less the
    pre-roll).  `endpoint`: a `Future[SpeechSpan]` that resolves when the detector has closed the utterance (`forced`: by the length limit
    that keeps it inside the encoder's capacity); cancelled when `close()` ended the microphone first.  `end(text)` -- before or after the
    endpoint -- returns the `Future[ListenResult]`: codes, frames and steps of a plain listener fed S[speech_start:speech_stop] and ended;
    `samples` counts that span at the model's rate.  A session's utterance enters the history at its result, as `hear` would put it.
    An utterance nobody `end()`s holds its audio in the ring and the encoder row only until the next utterance needs them: then it is
    DROPPED -- `dropped` is set, a later `end()` is a ValueError and nothing of it enters a session."""

    def __init__(self, listener: "CSMContinuousListener", start: int, onset_frame: int):
        super().__init__(listener.batcher)
        self.listener, self.onset, self.onset_frame = listener, int(start), int(onset_frame)
        self.endpoint: Future = Future()
        self.forced = False
        self.dropped = False
        self._start, self._stop, self._final = int(start), None, False
        self._done = False                    # resolved, dropped or failed: the scheduler has let go of it
        if listener._topts is not None:       # a transcribing microphone: every utterance has its transcript
            self._transcribes(listener._topts)

    def _took(self, codes: torch.Tensor, F: int) -> None:
        super()._took(codes, F)
        self.listener.frames += F

    def _end_refused(self) -> None:
        if self.dropped:
            raise ValueError("end: the utterance was dropped: the next one needed its encoder row and its room in the ring")
        if self._future is not None or self._done or not self.listener._open:
            raise ValueError("end: the utterance has ended or its listener was cancelled")

    def end(self, text=None) -> Future:
        return self._begin_end(self.listener.session, text)


class CSMContinuousListener:
    """What `listen(..., vad=..., continuous=True)` returns: one microphone that stays open.  `feed(pcm)` from any thread;
    `utterances()` iterates over its `CSMUtterance`s as the scheduler detects them and ends behind the last one of a closed microphone;
    `next_utterance(timeout)` takes one (None: the microphone has closed; `queue.Empty` at the timeout).  `close()`: no more audio -- an
    open utterance becomes final as if the stream ended there (its `endpoint` is cancelled: there was none), and the row is freed when the
    last utterance has resolved.  `cancel()` drops everything at once.  It holds one row of the batcher's streaming encoder, resampler,
    detector and device buffer from `listen` until then."""

    def __init__(self, batcher, row: int, speaker: int, session, sample_rate: Optional[int], fmt: Optional[str], vad: VAD.VadConfig, barge_in: bool,
                 transcribe=None):
        self.batcher, self.row, self.speaker, self.session = batcher, int(row), int(speaker), session
        self.cfg, self.barge_in = vad, bool(barge_in)
        self._topts = transcribe              # the checked whisper DecodingOptions of `listen(transcribe=)`, or None
        self._open = True                     # False once cancelled or freed: the row is someone else's
        self.spf = int(batcher.engine.samples_per_frame)
        self.rate, self.fmt = sample_rate, fmt
        sr = int(batcher.engine.sample_rate)
        self.ring_len = batcher.listen_max_frames * self.spf
        self.max_frames = VAD.ring_max_frames(vad, sr, self.ring_len)  # every span fits the ring, and the encoder row, from its start
        self.cap = self.ring_len              # the host queue's cap: what a one-shot listener's buffer is
        self._LM = None
        if self.rate is not None:
            self._LM = RS.ratio(self.rate, sr)
            self.cap = self.ring_len * self._LM[1] // self._LM[0]
        self._dtype = PCM.dtype(fmt)
        self._q: Deque[np.ndarray] = deque()  # fed and not yet uploaded
        self._qn = 0
        self.samples = 0                      # fed, at the listener's rate
        self.frames = 0                       # encoded, over all utterances
        self._up = 0                          # uploaded, at the listener's rate
        self._n24 = 0                         # samples of S the ring has taken
        self._carry = None                    # (float32 [rows, W] tensor, column, count): flushed outputs that wait for room in the ring
        self._cset = False                    # resampler and detector rows hold this stream
        self._closing = False                 # `close()` was called
        self._flushed = False                 # ... and everything fed, the resampler's tail included, has left the host
        self._whole = False                   # ... and the status that covers all of S has been consumed: no utterance will follow
        self._sent = (-1, -1)                 # the (n24, acked) of the last detector step that took the row
        self._cst = VAD.NO_RING_STATUS        # the last status consumed, and ...
        self._cn = 0                          # ... the n24 it covers
        self._acked = 0                       # records consumed
        self._utts: Deque[CSMUtterance] = deque()  # not yet resolved or dropped, oldest first
        self._open_utt: Optional[CSMUtterance] = None  # the one the detector has not closed yet
        self._uq: "queue.Queue" = queue.Queue()

    # ---- the caller's side ------------------------------------------------------------------------------------------------------------------
    def feed(self, pcm) -> None:
        """Samples at the listener's rate and in its format, any number.  They join a host queue under the batcher's lock; the scheduler
        drains it as it uploads.  ValueError, with nothing changed and nothing dropped, when the queue would hold more than
        `listen_max_frames` frames' worth of samples: the caller is feeding faster than the scheduler can take."""
        if self.fmt is not None or isinstance(pcm, (bytes, bytearray, memoryview)):
            a = np.array(PCM.samples(pcm, self.fmt))
        else:
            a = np.array(pcm, np.float32).reshape(-1)
        b = self.batcher
        with b._lock:
            if b._closed:
                raise RuntimeError("CSMBatcher is closed")
            if not self._open or self._closing:
                raise ValueError("feed: the listener was closed or cancelled")
            if self._qn + a.shape[0] > self.cap:
                raise ValueError(f"feed: {self._qn + a.shape[0]} samples wait for the scheduler, more than listen_max_frames = {b.listen_max_frames} frames")
            if a.shape[0]:
                self._q.append(a)
                self._qn += int(a.shape[0])
                self.samples += int(a.shape[0])
                b._wake.notify()

    def _take(self, k: int) -> np.ndarray:
        """Under the lock: the next k queued samples leave the queue."""
        out = np.zeros(k, self._dtype)
        i = 0
        while i < k:
            a = self._q[0]
            m = min(k - i, a.shape[0])
            out[i : i + m] = a[:m]
            if m == a.shape[0]:
                self._q.popleft()
            else:
                self._q[0] = a[m:]
            i += m
        self._qn -= k
        return out

    def utterances(self):
        while True:
            u = self._uq.get()
            if u is _END:
                self._uq.put(_END)  # (every later call ends at once, too)
                return
            yield u

    def next_utterance(self, timeout: Optional[float] = None) -> Optional[CSMUtterance]:
        u = self._uq.get(timeout=timeout) if timeout is None or timeout > 0 else self._uq.get_nowait()
        if u is _END:
            self._uq.put(_END)
            return None
        return u

    def close(self) -> None:
        b = self.batcher
        with b._lock:
            if not self._open or self._closing:
                return
            self._closing = True
            b._wake.notify()

    def cancel(self) -> bool:
        with self.batcher._lock:
            if not self._open:
                return False
            _vacate(self)
            self._q.clear()
            self._qn = 0
        self._shut(None)
        return True

    def _shut(self, e: Optional[BaseException]) -> None:
        """The microphone leaves: its row is the next caller's, the utterances the scheduler still held lose their endpoint, a pending
        `end()` fails with `e` (None: it is cancelled), and the utterance queue ends."""
        with self.batcher._lock:
            _vacate(self)
            utts = list(self._utts)
            self._utts.clear()
        for u in utts:
            u._done = True
            u.endpoint.cancel()
            _fail_future(u._future, e)
            _drop_transcript(u, e)
        self._uq.put(_END)


class ContinuousMixin(ListenMixin):
    """The scheduler's half (methods of `CSMBatcher`), on top of the one-shot listeners'.  Nothing here runs, and none of its objects is
    made, before the first `listen(continuous=True)`."""

    def _listen_init(self, *a) -> None:
        super()._listen_init(*a)
        self._cont_made = False                 # a continuous listener was made: the hooks of `step` are live
        self._rvad = None                       # vad.RingVad, one row per encoder row
        self._rvad_n = [0] * self.listen_rows   # per detector row: the n_avail and ...
        self._rvad_a = [0] * self.listen_rows   # ... the acked of its last step (a row no step takes is handed the same again)
        self._cont_out: Deque[tuple] = deque()  # (ticket, {row: (listener, the n24 covered)}): status and log on their way to the host

    def _cont_listen(self, row, speaker, session, sample_rate, fmt, vad, barge_in, **extra) -> CSMContinuousListener:
        """Under the lock."""
        lis = CSMContinuousListener(self, row, speaker, session, sample_rate, fmt, vad, barge_in, **extra)
        self._cont_made = True
        return lis

    def _cont_mics(self) -> List[CSMContinuousListener]:
        return [lis for lis in self._listeners if isinstance(lis, CSMContinuousListener) and lis._open]

    # ---- the batcher's hooks: the one-shot listeners first, then this ----------------------------------------------------------------------------
    def _listen_due(self) -> bool:
        return bool(self._cont_made and self._cont_due()) or super()._listen_due()

    def _listen_consume(self) -> None:
        super()._listen_consume()
        if self._cont_made:
            self._cont_consume()  # (likewise before the controls: every onset of a barge-in microphone)

    def _listen_round(self) -> bool:
        heard = super()._listen_round()
        return (self._cont_made and self._cont_round()) or heard

    def _listen_close(self) -> None:
        self._cont_out.clear()
        if self._rvad is not None:
            self._rvad.close()
        super()._listen_close()

    # ---- arithmetic (under the lock) ----------------------------------------------------------------------------------------------------------
    def _cont_room(self, lis: CSMContinuousListener) -> int:
        """Samples of S the ring can take now: n24 stays below keep_from + ring_len."""
        oldest = lis._utts[0]._start if lis._utts else None
        return VAD.keep_from(lis.cfg, int(self.engine.sample_rate), lis._cst[0], oldest) + lis.ring_len - lis._n24

    def _cont_waiting(self, lis: CSMContinuousListener) -> bool:
        """Something of this microphone has still to go up."""
        return lis._qn > 0 or lis._carry is not None or (lis._closing and not lis._flushed)

    def _cont_avail(self, lis: CSMContinuousListener, u: CSMUtterance) -> int:
        """Frames of u's stream S[start:] that may be encoded: all of S[start:stop] once it is final; while it is open only the whole frames
        below B = min(classified fl, (last_speech + 1) fl + keep) - start of the consumed status, which the final span can only grow beyond."""
        if u._final:
            return -(-(u._stop - u._start) // lis.spf)
        c, _, o, s = lis._cst
        sp = VAD.span(lis.cfg, (c, o, s, -1), lis._cn, False, int(self.engine.sample_rate))
        return max(0, sp[1] - u._start) // lis.spf

    def _cont_plan(self, lis: CSMContinuousListener):
        """What the head utterance is due: ("full", u), ("tail", u, r), ("finish", u), ("drop", u) or None."""
        if not lis._utts:
            return None
        u = lis._utts[0]
        left = self._cont_avail(lis, u) - u.frames
        M = self.listen_chunk
        if left >= M:
            return ("full", u)
        if not u._final:
            return None
        if left > 0:
            return ("tail", u, left)
        if u._future is not None:
            return ("finish", u) if u._text_ready(lis.session) else None  # (a session's `end()` without text waits for its transcript)
        nxt = lis._utts[1] if len(lis._utts) > 1 else None
        if nxt is not None and (nxt._final or self._cont_avail(lis, nxt) >= M):
            return ("drop", u)  # the next utterance needs the encoder row
        if self._cont_waiting(lis) and self._cont_room(lis) <= 0:
            return ("drop", u)  # ... or the stream needs its room in the ring
        return None

    def _cont_due(self) -> bool:
        """Under the lock: a continuous listener has work for the scheduler's next round."""
        if self._cont_out:
            return True
        for lis in self._cont_mics():
            if self._cont_waiting(lis) and (not lis._cset or self._cont_room(lis) > 0):
                return True
            if lis._cset and lis._sent != (lis._n24, lis._acked):
                return True
            if self._cont_plan(lis) is not None or self._cont_closable(lis):
                return True
        return False

    def _cont_closable(self, lis: CSMContinuousListener) -> bool:
        if not lis._closing:
            return False
        if not lis._whole:  # everything fed is in the ring, and the consumed status has classified every whole frame of it
            fl = lis.cfg.frame_len(int(self.engine.sample_rate))
            return lis._flushed and lis._carry is None and lis._cset and lis._cn == lis._n24 and lis._cst[0] == lis._n24 // fl
        return not lis._utts

    # ---- a round ----------------------------------------------------------------------------------------------------------------------------
    def _cont_round(self) -> bool:
        """The scheduler's thread, once per scheduling round, behind the one-shot listeners' round: upload, ONE detector step, one encode
        step of M frames for every head utterance that holds M frames, one per distinct remainder of the final ones, then the results."""
        did = self._cont_upload()
        if self._cont_detect() or self._cont_out:
            did = True
        with self._lock:
            mics = self._cont_mics()
            for lis in mics:
                if self._cont_closable(lis) and not lis._whole:
                    self._cont_whole(lis)
                    did = True
            plans = [(lis, self._cont_plan(lis)) for lis in mics]
        if self._stt is not None:
            self._stt_mark_utts()  # (before anything of this round can finish or drop an utterance and hand its room in the ring on)
        full = [(lis, p[1]) for lis, p in plans if p is not None and p[0] == "full"]
        if full:
            self._cont_encode(full, self.listen_chunk)
        with self._lock:
            plans = [(lis, self._cont_plan(lis)) for lis in self._cont_mics()]
        tails = {}
        for lis, p in plans:
            if p is not None and p[0] == "tail":
                tails.setdefault(p[2], []).append((lis, p[1]))
        for r in sorted(tails):
            self._cont_encode(tails[r], r)
        with self._lock:
            plans = [(lis, self._cont_plan(lis)) for lis in self._cont_mics()]
        for lis, p in plans:
            if p is not None and p[0] == "finish":
                self._cont_finish(lis, p[1])
                did = True
            elif p is not None and p[0] == "drop":
                self._cont_drop(lis, p[1])
                did = True
        with self._lock:
            gone = [lis for lis in self._cont_mics() if lis._whole and not lis._utts]
        for lis in gone:
            self._cont_free(lis)
            did = True
        return bool(did or full or tails)

    def _stt_mark_utts(self) -> None:
        """The utterances that became final (endpoints, forced ones and a closed microphone's last included): their spans of the ring, at
        64-bit stream positions, join the round's cut (csm_listen.py).  An utterance stays in `_utts`, and so behind the upload
        gate's `keep_from`, until this round's finish or drop at the earliest; nothing is written to the ring between here and the round's
        cut, which is stream-ordered before every later write."""
        spans = []
        with self._lock:
            for lis in self._cont_mics():
                for u in lis._utts:
                    if u.transcript is not None and not u._tcut and u._final:
                        u._tcut = True
                        spans.append((u, lis.row, lis.ring_len, u._start, u._stop - u._start))
        self._stt_mark(spans)

    def _cont_whole(self, lis: CSMContinuousListener) -> None:
        """Under the lock: the closed microphone's stream is whole and classified: an utterance still open ends with it."""
        u = lis._open_utt
        if u is not None:
            c, _, o, s = lis._cst
            sp = VAD.span(lis.cfg, (c, o, s, -1), lis._n24, True, int(self.engine.sample_rate))
            u._stop, u._final = sp[1], True
            lis._open_utt = None
            u.endpoint.cancel()  # the caller closed the microphone first: there was no endpoint
        lis._whole = True
        lis._uq.put(_END)

    def _cont_free(self, lis: CSMContinuousListener) -> None:
        with self._lock:
            _vacate(lis)
        lis._uq.put(_END)

    def _cont_upload(self) -> bool:
        """Every continuous listener's queued samples that the gate lets through go up once: the rows with a rate through ONE resampler
        step, the rows at the model's rate through ONE convert launch, and each of the two staging buffers into the rings by ONE ring
        write.  A closed microphone's resampler row is flushed with its last samples; flushed outputs the ring has no room for yet are
        carried on the device and written as room comes -- as are the few samples by which a resampler step overshoots the gate."""
        with self._lock:
            work = [lis for lis in self._cont_mics() if self._cont_waiting(lis)]
        if not work:
            return False
        sr = int(self.engine.sample_rate)
        try:
            self._listen_made(work)
            if self._rvad is None:
                self._rvad = self.engine.row_ring_vad(self.listen_rows)
        except Exception as e:  # noqa: BLE001
            for lis in work:
                lis._shut(e)
            return True
        for lis in list(work):
            if lis._cset:
                continue
            try:  # a new stream starts in the row: position 0 of the ring, zero resampler history, an armed detector with an empty log
                self._listen_set_row(lis)
                self._rvad.set_row(lis.row, lis.cfg.frame_len(sr), lis.cfg.thr2n(sr), lis.cfg.hang_frames, lis.max_frames, lis.ring_len)
                self._rvad_n[lis.row] = self._rvad_a[lis.row] = 0
                lis._cset = True
            except Exception as e:  # noqa: BLE001  (this row's own failure: the others go on)
                work.remove(lis)
                lis._shut(e)
        did = False
        carried = [lis for lis in work if lis._carry is not None]
        for lis in carried:  # (only at a full ring or behind a flush, and one small write each)
            try:
                did = self._cont_write_carry(lis) or did
            except Exception as e:  # noqa: BLE001
                lis._shut(e)
        rated = [lis for lis in work if lis.rate is not None and lis._open and lis._carry is None and not lis._flushed]
        plain = [lis for lis in work if lis.rate is None and lis._open and not lis._flushed]
        try:
            did = self._cont_upload_rated(rated) or did
        except Exception as e:  # noqa: BLE001  (the shared step: it fails the rows that took part in it)
            for lis in rated:
                lis._shut(e)
        try:
            did = self._cont_upload_plain(plain) or did
        except Exception as e:  # noqa: BLE001
            for lis in plain:
                lis._shut(e)
        return did

    def _cont_write_carry(self, lis: CSMContinuousListener) -> bool:
        y, col, left = lis._carry
        with self._lock:
            w = min(left, max(0, self._cont_room(lis)))
        if w <= 0:
            return False
        pos, n = [0] * self.listen_rows, [0] * self.listen_rows
        pos[lis.row], n[lis.row] = lis._n24, w
        self.engine.ring_write(y[:, col:], self._heard, lis.ring_len, pos, n)
        with self._lock:
            lis._n24 += w
            lis._carry = (y, col + w, left - w) if left > w else None
        return True

    def _cont_upload_rated(self, rated: List[CSMContinuousListener]) -> bool:
        todo = []
        with self._lock:
            for lis in rated:
                L, M = lis._LM
                room = self._cont_room(lis)
                # the fewest inputs that fill the room: ready(N) >= n24 + room first holds at N = (target M + half) // L + 1; what a step
                # emits beyond the room (fewer than L / M + 1 samples) is carried on the device and written as room comes
                k = 0 if room <= 0 else max(0, min(lis._qn, self.LISTEN_IN, ((lis._n24 + room) * M + RS.half_len(L, M)) // L + 1 - lis._up))
                flush = lis._closing and k == lis._qn
                if k > 0 or flush:
                    todo.append((lis, lis._take(k), flush))
        if not todo:
            return False
        n_in, fl = [0] * self.listen_rows, [False] * self.listen_rows
        for lis, a, flush in todo:
            n_in[lis.row], fl[lis.row] = int(a.shape[0]), flush
        x = self._listen_stage([(lis.row, a) for lis, a, _ in todo], any(lis.fmt is not None for lis, _, _ in todo))
        y, n_out = self._lrs.step(x, n_in, fl)
        yf = y if y.dtype == torch.float32 else y.view(torch.float32)  # (a byte y: rows of 16-byte multiples, the outputs float32)
        pos, n = [0] * self.listen_rows, [0] * self.listen_rows
        with self._lock:
            for lis, a, flush in todo:
                w = min(n_out[lis.row], max(0, self._cont_room(lis)))
                pos[lis.row], n[lis.row] = lis._n24, w
        if any(n):
            self.engine.ring_write(yf, self._heard, todo[0][0].ring_len, pos, n)
        with self._lock:
            for lis, a, flush in todo:
                w = n[lis.row]
                lis._up += int(a.shape[0])
                lis._n24 += w
                lis._flushed = flush
                if n_out[lis.row] > w:
                    lis._carry = (yf, w, n_out[lis.row] - w)
        return True

    def _cont_upload_plain(self, plain: List[CSMContinuousListener]) -> bool:
        todo = []
        with self._lock:
            for lis in plain:
                k = max(0, min(lis._qn, self.LISTEN_IN, self._cont_room(lis)))
                if k > 0:
                    todo.append((lis, lis._take(k)))
                elif lis._closing and lis._qn == 0:
                    lis._flushed = True  # (nothing is carried between steps at the model's rate: the stream is whole)
        if not todo:
            return False
        fmts, n, pos = ["f32"] * self.listen_rows, [0] * self.listen_rows, [0] * self.listen_rows
        for lis, a in todo:
            fmts[lis.row], n[lis.row], pos[lis.row] = lis.fmt or "f32", int(a.shape[0]), lis._n24
        y = self._cvt.convert(self._listen_stage([(lis.row, a) for lis, a in todo], True), fmts, ["f32"] * self.listen_rows, n)
        self.engine.ring_write(y.view(torch.float32), self._heard, todo[0][0].ring_len, pos, n)
        with self._lock:
            for lis, a in todo:
                lis._up += int(a.shape[0])
                lis._n24 += int(a.shape[0])
                if lis._closing and lis._qn == 0:
                    lis._flushed = True
        return True

    def _cont_detect(self) -> bool:
        """ONE detector step over the rings for every row with samples the detector has not seen or an ack it has not been told (which may
        release a walk stalled at a full log); then status table and log start their way to pinned host memory."""
        with self._lock:
            rows = [lis for lis in self._cont_mics() if lis._cset and lis._sent != (lis._n24, lis._acked)]
            if not rows:
                return False
            n, a = list(self._rvad_n), list(self._rvad_a)
            for lis in rows:
                n[lis.row], a[lis.row] = lis._n24, lis._acked
        try:
            self._rvad.step(self._heard, n, a)
            self._rvad_n, self._rvad_a = n, a
            ticket = self._rvad.fetch()
        except Exception as e:  # noqa: BLE001  (the shared step: it fails the rows that took part in it)
            for lis in rows:
                lis._shut(e)
            return True
        with self._lock:
            for lis in rows:
                lis._sent = (n[lis.row], a[lis.row])
        self._cont_out.append((ticket, {lis.row: (lis, n[lis.row]) for lis in rows}))
        return True

    def _cont_consume(self) -> None:
        """The scheduler's thread, at the top of a round, before the controls: every table that has landed (`ready()`, no sync) becomes its
        listeners' state.  New records close the open utterance or, when an utterance began and closed between two consumed tables, make
        one that is final at once; an onset behind them makes the open one.  Every new utterance of a `barge_in` listener records the
        interrupt of the session's queued or live turn, which this same round's `_apply_controls` applies."""
        sr = int(self.engine.sample_rate)
        # tables land in the order of their steps, the status is cumulative and a record stays in the log until it is acked: the newest
        # table that has landed says everything the older ones say, so those are let go unread
        newest = next((i for i in range(len(self._cont_out) - 1, -1, -1) if self._cont_out[i][0].ready()), -1)
        if newest >= 0:
            covered = {}
            for _ in range(newest):
                old, rows = self._cont_out.popleft()
                covered.update(rows)
                old.drop()
            ticket, rows = self._cont_out.popleft()
            covered.update(rows)
            status, log = ticket.take()
            for row, (lis, n24) in covered.items():
                made, closed_now = [], []
                with self._lock:
                    if not (lis._open and self._listeners[row] is lis):
                        continue
                    c, closed, o, s = (int(v) for v in status[row])
                    fl = lis.cfg.frame_len(sr)

                    def new(onset_frame):
                        u = CSMUtterance(lis, max(0, onset_frame * fl - lis.cfg.pre_roll(sr)), onset_frame)
                        lis._utts.append(u)
                        made.append(u)
                        self._barge_in(lis)
                        return u

                    for r in range(lis._acked, closed):
                        rec = tuple(int(v) for v in log[row][r % VAD.RING_LOG])
                        u = lis._open_utt if lis._open_utt is not None else new(rec[0])
                        sp = VAD.span(lis.cfg, VAD.record_status(rec), 0, False, sr)
                        u._stop, u._final, u.forced = sp[1], True, bool(rec[3] & VAD.FORCED)
                        lis._open_utt = None
                        closed_now.append((u, rec, sp))
                    lis._acked = closed
                    if o >= 0 and lis._open_utt is None:
                        lis._open_utt = new(o)
                    lis._cst, lis._cn = (c, closed, o, s), n24
                for u in made:
                    lis._uq.put(u)
                for u, rec, sp in closed_now:
                    if _claim(u.endpoint):
                        u.endpoint.set_result(_speech_span(sp, rec[0], rec[2], lis.rate, sr, forced=u.forced))

    def _cont_encode(self, group, F: int) -> None:
        """One step of the row encoder: F frames of every utterance of `group`, read out of the rings by ONE ring read -- S[start:stop],
        and zeros, not what the ring holds there, behind `stop`.  A failure fails the group's microphones."""
        lises = [lis for lis, _ in group]

        def fill():
            x = torch.zeros((self.listen_rows, 1, F * spf), dtype=torch.float32, device=self.engine.device)
            pos, n, tot = [0] * self.listen_rows, [0] * self.listen_rows, [0] * self.listen_rows
            for lis, u in group:
                a = u._start + u.frames * spf
                b = a + F * spf if not u._final else min(a + F * spf, u._stop)
                pos[lis.row], n[lis.row], tot[lis.row] = a, b - a, F * spf
            self.engine.ring_read(self._heard, lises[0].ring_len, x.view(self.listen_rows, F * spf), pos, n, tot)
            return x

        try:
            spf = lises[0].spf
            self._encode_step([(lis.row, u) for lis, u in group], F, fill)
        except Exception as e:  # noqa: BLE001
            for lis in lises:
                lis._shut(e)

    def _cont_drop(self, lis: CSMContinuousListener, u: CSMUtterance) -> None:
        self._cont_pop(lis, u, dropped=True)
        u.endpoint.cancel()  # (no effect on one that has resolved)

    def _cont_finish(self, lis: CSMContinuousListener, u: CSMUtterance) -> None:
        """A final utterance has all its frames and its `end()`: its audio S[start:stop] leaves the ring for a session's history, the
        result resolves, and its room in the ring and the encoder row are the next one's."""
        k = u._stop - u._start

        def audio():
            out = torch.zeros((1, k), dtype=torch.float32, device=self.engine.device)
            self.engine.ring_read(self._heard[lis.row : lis.row + 1], lis.ring_len, out, [u._start], [k], [k])
            return out[0].cpu().numpy()

        self._heard_turn(u, lis, audio, dict(samples=k, sample_rate=int(self.engine.sample_rate), speech_start=u._start, speech_stop=u._stop),
                         release=lambda: self._cont_pop(lis, u))

    def _cont_pop(self, lis: CSMContinuousListener, u: CSMUtterance, dropped: bool = False) -> None:
        with self._lock:
            if lis._utts and lis._utts[0] is u:
                lis._utts.popleft()
            u.dropped, u._done = u.dropped or dropped, True
