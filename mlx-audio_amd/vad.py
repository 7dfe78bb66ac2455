"""Voice-activity endpointing for the listening edge of CSM serving: the reference's energy rule and listener loop
(mlx_audio/sts/voice_pipeline.py `_is_silent`, `_listener`) on the device, where the listeners' audio already is.

A frame of `frame_len` samples is speech iff its rms >= `threshold`; the kernel compares E = sum x^2 with thr2n = threshold^2 frame_len
(kk_vad.hip: no square root, no division).  Per stream and in frame order: a speech frame sets speaking, zeroes the silent count and is the
last speech frame (the first one is the onset); a silent frame while speaking counts up, and the frame that makes the count pass
`hang_frames` is the endpoint, behind which nothing is classified; silence before any speech is dropped.  A status is the four integers
(classified, onset, last_speech, endpoint), -1 for "none", counted in frames.

`VadConfig`: the settings, with the reference's defaults.  `span(cfg, status, n, ended)`: the one place where a status becomes samples.
`RowVad(max_rows)`: one object, one launch per step, a stream per row -- the structure of `resample.RowResampler`; `fetch()` hands the status table back without a sync.  `detect(x, cfg, rate)`:
a whole clip.  No CPU or PyTorch fallback: without the library `RowVad`, `RingVad` and `detect` raise.

A microphone that stays open: `RingVad(max_rows)` is the same detector over a ring, in 64-bit stream positions, which re-arms
behind every utterance and keeps a log of the closed ones; `utterances(cfg, x, rate, max_frames)` is the host-side definition of what it
reports.  A closed record (onset, last_speech, endpoint, forced) goes through `span` as the status (endpoint + 1, onset, last_speech, endpoint)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_FRAME = 4096  # samples per frame the kernel takes
NO_STATUS = (0, -1, -1, -1)
RING_LOG = 8  # closed records the ring detector keeps per row in front of the host's ack (KK_VAD_LOG)
NO_RING_STATUS = (0, 0, -1, -1)  # (classified, closed, onset, last_speech) of a new ring row
FORCED = 1  # flag of a record closed by max_frames


@dataclass(frozen=True)
class VadConfig:
    """frame_ms, threshold, silence_ms: the reference's frame_duration_ms = 30, silence_threshold = 0.03 and silence_duration = 1.5 s.
    pre_roll_ms: audio kept in front of the onset frame.  keep_silence_ms: trailing silence kept behind the last speech frame; None keeps
    every frame up to the endpoint frame, as the reference does."""
    frame_ms: int = 30
    threshold: float = 0.03
    silence_ms: float = 1500
    pre_roll_ms: float = 0
    keep_silence_ms: Optional[float] = None

    def __post_init__(self):
        if int(self.frame_ms) != self.frame_ms or self.frame_ms < 1:
            raise ValueError(f"frame_ms must be a positive integer, got {self.frame_ms!r}")
        t = float(self.threshold)
        if not (t >= 0.0 and t != float("inf")):
            raise ValueError(f"threshold must be finite and >= 0, got {self.threshold!r}")
        if self.silence_ms < 0 or self.pre_roll_ms < 0 or (self.keep_silence_ms is not None and self.keep_silence_ms < 0):
            raise ValueError("silence_ms, pre_roll_ms and keep_silence_ms must be >= 0")

    def frame_len(self, rate: int) -> int:
        """Samples per frame at `rate`; ValueError outside the kernel's range [1, 4096]."""
        fl = int(rate) * int(self.frame_ms) // 1000
        if not 1 <= fl <= MAX_FRAME:
            raise ValueError(f"{self.frame_ms} ms at {rate} Hz are {fl} samples per frame: the detector takes [1, {MAX_FRAME}]")
        return fl

    @property
    def hang_frames(self) -> int:
        """The reference's frames_until_silence: the endpoint is the frame that makes the silent count PASS this."""
        return int(self.silence_ms / self.frame_ms)

    def thr2n(self, rate: int) -> np.float32:
        """threshold^2 frame_len, computed in double precision and rounded once."""
        return np.float32(float(self.threshold) * float(self.threshold) * self.frame_len(rate))

    def pre_roll(self, rate: int) -> int:
        return int(self.pre_roll_ms * int(rate) / 1000)

    def keep(self, rate: int) -> int:
        """Samples kept behind the last speech frame; None: (hang_frames + 1) frames, every frame up to the endpoint frame."""
        if self.keep_silence_ms is None:
            return (self.hang_frames + 1) * self.frame_len(rate)
        return int(self.keep_silence_ms * int(rate) / 1000)


def span(cfg: VadConfig, status: Sequence[int], n: int, ended: bool = True, rate: int = 24000) -> Optional[Tuple[int, int]]:
    """(start, stop) in samples of the speech a status describes, None without an onset.  n: the samples of the stream so far; ended: no more
    will come.  With an endpoint, or once the stream has ended, the span is final; a partial last frame is never classified, which makes it
    silence.  While the stream is open and has no endpoint, `stop` is only what is certain so far: it never passes the classified frames."""
    classified, o, s, e = (int(v) for v in status)
    if o < 0:
        return None
    fl = cfg.frame_len(rate)
    start = max(0, o * fl - cfg.pre_roll(rate))
    limit = (e + 1) * fl if e >= 0 else (int(n) if ended else classified * fl)
    return start, min((s + 1) * fl + cfg.keep(rate), limit)


def record_status(rec: Sequence[int]) -> Tuple[int, int, int, int]:
    """A closed record (onset, last_speech, endpoint, flags) of the ring detector as the status `span` takes."""
    o, s, e = int(rec[0]), int(rec[1]), int(rec[2])
    return e + 1, o, s, e


def utterances(cfg: VadConfig, x, rate: int = 24000, max_frames: Optional[int] = None, energies: bool = False):
    """What the ring detector reports on a whole stream: -> (records, status).  records: one (onset, last_speech, endpoint, flags) per closed
    utterance, in frames; status: (classified, closed, onset, last_speech), the last two of the utterance still open, -1 for none.
    x: the samples at `rate` (frame energies are summed in float64), or with `energies` the per-frame energies themselves.  The rule per
    frame f: E >= thr2n is speech (NaN is silence, inf speech): speaking, silent = 0, last_speech = f, onset = f if there was none; silence
    while speaking counts up and silent > hang_frames closes the utterance at f; otherwise, while speaking, f - onset + 1 == max_frames
    closes it at f with the flag FORCED.  Closing re-arms: the next frame may be the next onset."""
    fl = cfg.frame_len(rate)
    x = np.asarray(x, np.float64)
    if not energies:
        nf = x.shape[0] // fl
        with np.errstate(all="ignore"):
            x = (x[: nf * fl].reshape(nf, fl) ** 2).sum(axis=1)
    thr, hang = float(cfg.thr2n(rate)), cfg.hang_frames
    if max_frames is not None and max_frames < 1:
        raise ValueError(f"max_frames must be >= 1, got {max_frames}")
    records: List[Tuple[int, int, int, int]] = []
    speaking, silent, onset, last = False, 0, -1, -1
    for f, e in enumerate(x.tolist()):
        close = flags = 0
        if e >= thr:
            speaking, silent, last = True, 0, f
            if onset < 0:
                onset = f
        elif speaking:
            silent += 1
            close = silent > hang
        if not close and speaking and max_frames is not None and f - onset + 1 == max_frames:
            close, flags = 1, FORCED
        if close:
            records.append((onset, last, f, flags))
            speaking, silent, onset, last = False, 0, -1, -1
    return records, (int(x.shape[0]), len(records), onset, last)


def keep_from(cfg: VadConfig, rate: int, classified: int, oldest_start: Optional[int]) -> int:
    """The first position a continuous listener's ring must still hold: the start of its oldest utterance not yet finished, and in any case
    what a new onset at frame `classified` (the next one the detector may report) would keep in front of itself."""
    k = int(classified) * cfg.frame_len(rate) - cfg.pre_roll(rate)
    return max(0, k if oldest_start is None else min(int(oldest_start), k))


def ring_max_frames(cfg: VadConfig, rate: int, ring_len: int) -> int:
    """The detector frames an utterance may span so that pre-roll + utterance fits a ring of `ring_len` samples from its start."""
    m = (int(ring_len) - cfg.pre_roll(rate)) // cfg.frame_len(rate)
    if m < 1:
        raise ValueError(f"a ring of {ring_len} samples does not hold the pre-roll and one frame of {cfg.frame_len(rate)}")
    return m


def _torch():
    import torch

    return torch


def _stream(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class StatusTicket:
    """What `RowVad.fetch` returns: the status table on its way to the host.  `ready()`: the copy has landed (`event.query()`, no sync);
    `take()`: the table as int32 numpy [max_rows, 4] -- waits if it has not landed -- after which the ticket is spent."""

    def __init__(self, owner: "RowVad", pin, event):
        self._owner, self._pin, self._event = owner, pin, event

    def ready(self) -> bool:
        return bool(self._event.query())

    def take(self) -> np.ndarray:
        self._event.synchronize()
        out = self._pin.numpy().copy()
        self._owner._pins.append(self._pin)
        self._pin = None
        return out


class RowVad:
    """`max_rows` independent streams.  `set_row(row, frame_len, thr2n, hang_frames)` starts one; `step(x, n_avail)` is ONE launch that
    classifies every row's new whole frames of x[row, :n_avail[row]] -- the row's stream from its first sample, the same buffer every step --
    and leaves {classified, onset, last_speech, endpoint} in `status[row]` (int32 [max_rows, 4] on the device).  A row's status is, bit for
    bit, that of the whole clip whatever the slicing and whatever the other rows do.  No step synchronises."""

    def __init__(self, max_rows: int, device=None):
        from ._lib import check, load

        torch = _torch()
        self.lib, self._check = load(), check
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_rows = int(max_rows)
        self._h = None
        self._rows: List[Optional[list]] = [None] * self.max_rows  # per row: [frame_len, frames handed to the device], the size of an energy row
        with torch.cuda.device(self.device):
            h = C.c_void_p()
            check(self.lib.kk_vad_create(self.max_rows, C.byref(h)), "kk_vad_create")
            self._h = h
            self.status = torch.tensor([NO_STATUS] * self.max_rows, dtype=torch.int32, device=self.device)
            self._none = self.status[0].clone()  # what a new stream's status row is set to, in stream order
        self._pins: list = []  # pinned [max_rows, 4] tables that no ticket holds

    def _handle(self):
        if self._h is None:
            from ._lib import KokoroHipError

            raise KokoroHipError("RowVad is closed")
        return self._h

    def set_row(self, row: int, frame_len: int, thr2n: float, hang_frames: int) -> None:
        """A new stream starts in `row`: zero counts, no onset; the other rows are untouched."""
        torch = _torch()
        with torch.cuda.device(self.device):
            self._check(self.lib.kk_vad_set_row(self._handle(), _stream(self.device), int(row), int(frame_len), C.c_float(float(thr2n)), int(hang_frames)),
                        "kk_vad_set_row")
            self.status[int(row)].copy_(self._none)
        self._rows[int(row)] = [int(frame_len), 0]

    def step(self, x, n_avail: Sequence[int], energy: bool = False):
        """x [max_rows, W] float32 on the device, contiguous; n_avail [max_rows] on the host.  -> None, or with `energy` a float32
        [max_rows, K] device tensor: row b's entries [0, new frames of b) are the energies of the frames this step handed to the device."""
        torch = _torch()
        h = self._handle()
        n = np.ascontiguousarray(np.asarray(n_avail, np.int32))
        if n.shape != (self.max_rows,):
            raise ValueError(f"n_avail must hold {self.max_rows} entries")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and x.shape[0] == self.max_rows and x.is_contiguous()):
            raise ValueError(f"x must be a contiguous float32 device tensor [{self.max_rows}, W]")
        e, lde = None, 0
        if energy:
            new = [max(0, int(n[b]) // st[0] - st[1]) if st is not None else 0 for b, st in enumerate(self._rows)]
            lde = max(1, max(new))
            e = torch.zeros((self.max_rows, lde), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.kk_vad_step(h, _stream(self.device), C.c_void_p(x.data_ptr()), int(x.shape[1]), n.ctypes.data_as(C.c_void_p),
                                             C.c_void_p(self.status.data_ptr()), C.c_void_p(e.data_ptr()) if e is not None else None, int(lde)), "kk_vad_step")
        for b, st in enumerate(self._rows):
            if st is not None:
                st[1] = max(st[1], int(n[b]) // st[0])
        return e

    def fetch(self) -> StatusTicket:
        """The status table as the steps so far leave it, copied behind them to pinned host memory without blocking, and an event behind the
        copy: the caller polls `ready()` and reads the table a round or two later."""
        torch = _torch()
        self._handle()
        with torch.cuda.device(self.device):
            pin = self._pins.pop() if self._pins else torch.empty((self.max_rows, 4), dtype=torch.int32, pin_memory=True)
            pin.copy_(self.status, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self.device))
        return StatusTicket(self, pin, event)

    def close(self) -> None:
        if self._h is not None:
            self.lib.kk_vad_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RingTicket:
    """What `RingVad.fetch` returns: the status table and the log on their way to the host.  `ready()`: the copy has landed (no sync);
    `take()` -> (status int64 [max_rows, 4], log int64 [max_rows, RING_LOG, 4]) -- waits if it has not landed; then the ticket is spent;
    `drop()` spends it unread."""

    def __init__(self, owner: "RingVad", pin, event):
        self._owner, self._pin, self._event = owner, pin, event

    def ready(self) -> bool:
        return bool(self._event.query())

    def take(self):
        self._event.synchronize()
        out = self._pin.numpy().copy()
        self._owner._pins.append(self._pin)
        self._pin = None
        r = self._owner.max_rows
        return out[: r * 4].reshape(r, 4), out[r * 4 :].reshape(r, RING_LOG, 4)

    def drop(self) -> None:
        """The ticket is let go unread (a newer table says all it says); its pinned buffer serves a later `fetch`, whose copy is ordered
        behind this one's on the stream."""
        self._owner._pins.append(self._pin)
        self._pin = None


class RingVad:
    """`max_rows` microphones that stay open (kk_vad_ring).  `set_row(row, frame_len, thr2n, hang_frames, max_frames, ring_len)`
    starts a stream at position 0; `step(x, n_avail, acked)` is ONE launch that classifies every row's new whole frames, where sample p of a
    row lives at x[row, p % ring_len] and n_avail counts the row's samples since set_row (64-bit).  `status[row]` = (classified, closed,
    onset, last_speech) int64 on the device; record k of a row (onset, last_speech, endpoint, flags) lives at `log[row, k % RING_LOG]`.
    `acked[row]`: the records the caller has consumed; the device stops in front of a frame while closed - acked == RING_LOG and a later
    step goes on from there.  Energies are bit-equal to the flat detector's on the same stream.  No step synchronises."""

    def __init__(self, max_rows: int, device=None):
        from ._lib import check, load

        torch = _torch()
        self.lib, self._check = load(), check
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_rows = int(max_rows)
        self._h = None
        self._fl: List[int] = [0] * self.max_rows  # per row: its frame length, the size of an energy row
        with torch.cuda.device(self.device):
            h = C.c_void_p()
            check(self.lib.kk_vad_ring_create(self.max_rows, C.byref(h)), "kk_vad_ring_create")
            self._h = h
            r = self.max_rows
            self._table = torch.zeros(r * 4 + r * RING_LOG * 4, dtype=torch.int64, device=self.device)  # status and log, one copy to the host
            self.status = self._table[: r * 4].view(r, 4)
            self.log = self._table[r * 4 :].view(r, RING_LOG, 4)
            self.status.copy_(torch.tensor([NO_RING_STATUS] * r, dtype=torch.int64))
            self._none = self.status[0].clone()
        self._pins: list = []

    def _handle(self):
        if self._h is None:
            from ._lib import KokoroHipError

            raise KokoroHipError("RingVad is closed")
        return self._h

    def set_row(self, row: int, frame_len: int, thr2n: float, hang_frames: int, max_frames: int, ring_len: int) -> None:
        """A new stream starts in `row` at position 0: zero counts, no open utterance, an empty log; the other rows are untouched."""
        torch = _torch()
        with torch.cuda.device(self.device):
            self._check(self.lib.kk_vad_ring_set_row(self._handle(), _stream(self.device), int(row), int(frame_len), C.c_float(float(thr2n)), int(hang_frames),
                                                     int(max_frames), int(ring_len)), "kk_vad_ring_set_row")
            self.status[int(row)].copy_(self._none)
            self.log[int(row)].zero_()
        self._fl[int(row)] = int(frame_len)

    def step(self, x, n_avail: Sequence[int], acked: Sequence[int], energy=False):
        """x [max_rows, W] float32 on the device, contiguous, W >= every row's ring_len; n_avail, acked [max_rows] on the host.  energy: a
        float32 device tensor [max_rows, K] that receives frame f's energy at [row, f % K], or True for a new one that holds a ring's worth of
        frames (returned)."""
        torch = _torch()
        h = self._handle()
        n = np.ascontiguousarray(np.asarray(n_avail, np.int64))
        a = np.ascontiguousarray(np.asarray(acked, np.int64))
        if n.shape != (self.max_rows,) or a.shape != (self.max_rows,):
            raise ValueError(f"n_avail and acked must hold {self.max_rows} entries")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and x.shape[0] == self.max_rows and x.is_contiguous()):
            raise ValueError(f"x must be a contiguous float32 device tensor [{self.max_rows}, W]")
        e = None
        if energy is True:
            e = torch.zeros((self.max_rows, max([1] + [int(x.shape[1]) // fl for fl in self._fl if fl])), dtype=torch.float32, device=self.device)
        elif energy is not False and energy is not None:
            e = energy
            if not (isinstance(e, torch.Tensor) and e.is_cuda and e.dtype == torch.float32 and e.ndim == 2 and e.shape[0] == self.max_rows and e.is_contiguous()):
                raise ValueError(f"energy must be a contiguous float32 device tensor [{self.max_rows}, K]")
        with torch.cuda.device(self.device):
            self._check(self.lib.kk_vad_ring_step(h, _stream(self.device), C.c_void_p(x.data_ptr()), int(x.shape[1]), n.ctypes.data_as(C.c_void_p),
                                                  a.ctypes.data_as(C.c_void_p), C.c_void_p(self.status.data_ptr()), C.c_void_p(self.log.data_ptr()),
                                                  C.c_void_p(e.data_ptr()) if e is not None else None, int(e.shape[1]) if e is not None else 0),
                        "kk_vad_ring_step")
        return e

    def fetch(self) -> RingTicket:
        """Status table and log as the steps so far leave them, copied behind them to pinned host memory without blocking, and an event
        behind the copy."""
        torch = _torch()
        self._handle()
        with torch.cuda.device(self.device):
            pin = self._pins.pop() if self._pins else torch.empty(self._table.shape, dtype=torch.int64, pin_memory=True)
            pin.copy_(self._table, non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self.device))
        return RingTicket(self, pin, event)

    def close(self) -> None:
        if self._h is not None:
            self.lib.kk_vad_ring_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def detect(x, cfg: Optional[VadConfig] = None, rate: int = 24000, device=None, energy: bool = False):
    """A whole mono clip on the device (kk_op_vad; synchronises) -> (onset, last_speech, endpoint, start, stop): the three frame indices, -1
    for "none", and the speech span in samples (start = stop = 0 without an onset).  energy: also the float32 [n // frame_len] energies of
    the frames that were classified (zeros behind an endpoint), as a sixth entry."""
    from ._lib import check, load

    torch = _torch()
    cfg = cfg if cfg is not None else VadConfig()
    x = torch.as_tensor(x)
    device = torch.device(device) if device is not None else (x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    x = x.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if x.shape[0] < 1:
        raise ValueError("detect: an empty clip")
    fl = cfg.frame_len(rate)
    st = (C.c_int32 * 4)()
    with torch.cuda.device(device):
        e = torch.zeros(max(1, x.shape[0] // fl), dtype=torch.float32, device=device) if energy else None
        check(load().kk_op_vad(_stream(device), C.c_void_p(x.data_ptr()), int(x.shape[0]), fl, C.c_float(float(cfg.thr2n(rate))), cfg.hang_frames,
                               C.cast(st, C.c_void_p), C.c_void_p(e.data_ptr()) if e is not None else None), "kk_op_vad")
    sp = span(cfg, list(st), int(x.shape[0]), True, rate) or (0, 0)
    out = (int(st[1]), int(st[2]), int(st[3]), sp[0], sp[1])
    return out + (e[: x.shape[0] // fl],) if energy else out
