"""Always-open microphones (`listen(vad=, continuous=True)`) against the scripted engine, encoder and converter of
test_csm_vad_cpu.py (no device), a numpy ring detector on the real surface (`set_row`, `step(x, n_avail, acked)`, `fetch` -> ticket of
status and log) whose tickets become ready only k rounds after their step, k in {0, 1, 3}, and numpy ring copies.  The ring is 10 detector
frames, the stream more than 5 rings.

The contract: with S everything fed, the utterances are those of `vad.utterances` (and of tests/_vad_ring_ref.py) on S, and utterance u
resolves with the codes, frames and steps -- and every sample its encoder row was fed, the zeros behind `stop` included -- of a plain
listener fed S[start_u:stop_u] and ended, whatever the slicing of `feed`, the lag and the gate.  The numpy detector and ring copies refuse
what the gate must never let happen: a frame classified, or a sample read, after its place in the ring was written again."""
import os
import queue
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _vad_ring_ref as R  # noqa: E402
from test_csm_interrupt_cpu import SPF, _batcher, _marks  # noqa: E402
from test_csm_vad_cpu import FL, HANG, LOUD, QUIET, SR, Encoder as _Encoder, Engine as _Engine, M, Ticket as _Ticket, _clip, _plain  # noqa: E402

from mlx_audio_amd import vad as VAD  # noqa: E402
from mlx_audio_amd.csm_continuous import CSMContinuousListener, CSMUtterance  # noqa: E402
from mlx_audio_amd.csm_serve import ListenResult, SpeechSpan  # noqa: E402
from mlx_audio_amd.vad import VadConfig  # noqa: E402

LMF = 80              # listen_max_frames: the ring is 240 samples = 10 detector frames
RING = LMF * SPF


def _cfg(**kw):
    cfg = VadConfig(frame_ms=1, threshold=0.03, silence_ms=HANG, **kw)
    assert cfg.frame_len(SR) == FL and cfg.hang_frames == HANG
    return cfg


class Ticket(_Ticket):
    def drop(self):
        self.table = None  # let go unread: a newer table says all it says


class NumpyRingVad:
    """The surface of `vad.RingVad`: the kernel's rule E >= thr2n on float64 energies of frames read modulo the ring, the re-arming state
    machine, the log of RING_LOG records and the stall in front of a full log."""

    def __init__(self, engine, rows):
        self.engine, self.rows, self.closed = engine, [None] * rows, False
        self.status = np.array([VAD.NO_RING_STATUS] * rows, np.int64)
        self.log = np.zeros((rows, VAD.RING_LOG, 4), np.int64)

    def set_row(self, row, frame_len, thr2n, hang, max_frames, ring_len):
        self.rows[row] = dict(fl=int(frame_len), thr=float(thr2n), hang=int(hang), mx=int(max_frames), ring=int(ring_len), n=0, a=0, speaking=False, silent=0)
        self.status[row], self.log[row] = VAD.NO_RING_STATUS, 0
        self.engine.calls.append(("rvad_set_row", row, frame_len, hang, max_frames, ring_len))

    def step(self, x, n_avail, acked):
        assert not self.closed and len(n_avail) == len(acked) == len(self.rows) == x.shape[0]
        took = []
        for r, st in enumerate(self.rows):
            if st is None:
                continue
            c, closed, o, s = (int(v) for v in self.status[r])
            n, a = int(n_avail[r]), int(acked[r])
            assert st["n"] <= n and st["a"] <= a <= closed and st["ring"] <= x.shape[1]
            assert n - st["ring"] <= c * st["fl"], "a frame the detector has not classified was overwritten in the ring"
            upto = n // st["fl"]
            if upto > c or a > st["a"]:
                took.append(r)
            st["n"], st["a"] = n, a
            xr = x[r].numpy()
            while c < upto and closed - a < VAD.RING_LOG:
                e = float((xr[(c * st["fl"] + np.arange(st["fl"])) % st["ring"]].astype(np.float64) ** 2).sum())
                close = flags = 0
                if e >= st["thr"]:
                    st["speaking"], st["silent"], s = True, 0, c
                    o = c if o < 0 else o
                elif st["speaking"]:
                    st["silent"] += 1
                    close = st["silent"] > st["hang"]
                if not close and st["speaking"] and c - o + 1 == st["mx"]:
                    close, flags = 1, 1
                if close:
                    self.log[r, closed % VAD.RING_LOG] = (o, s, c, flags)
                    closed += 1
                    st["speaking"], st["silent"], o, s = False, 0, -1, -1
                c += 1
            self.status[r] = (c, closed, o, s)
        self.engine.calls.append(("rvad_step", tuple(took)))

    def fetch(self):
        return Ticket((self.status.copy(), self.log.copy()), self.engine.lag)

    def close(self):
        self.closed = True


class Encoder(_Encoder):
    """... and `streams[row]` keeps what every earlier stream of the row was fed: one entry per `reset_row`."""

    def __init__(self, *a):
        super().__init__(*a)
        self.streams = [[] for _ in range(self.max_batch)]

    def reset_row(self, row):
        if self.fed[row]:
            self.streams[row].append(self.fed[row])
        super().reset_row(row)


class Engine(_Engine):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.rvads, self.written = [], {}

    def row_encoder(self, max_batch, max_frames, max_chunk):
        self.enc = Encoder(self, max_batch, max_frames, max_chunk)
        return self.enc

    def row_ring_vad(self, max_rows):
        self.rvads.append(NumpyRingVad(self, max_rows))
        return self.rvads[-1]

    def ring_write(self, src, ring, ring_len, pos, n):
        self.calls.append(("ring_write", tuple(n)))
        for b, k in enumerate(n):
            if k:
                assert pos[b] == self.written.get(b, 0), "the stream is written in order, every sample once"
                ring[b, (pos[b] + np.arange(k)) % ring_len] = src[b, :k]
                self.written[b] = pos[b] + k

    def ring_read(self, ring, ring_len, dst, pos, n, n_total):
        self.calls.append(("ring_read", tuple(n), tuple(n_total)))
        for b, k in enumerate(n):
            if n_total[b] == 0:
                continue
            if ring.shape[0] == self.enc.max_batch:  # (the whole buffer, not one row's view: the row is known)
                assert pos[b] + k <= self.written.get(b, 0), "samples were read that were never written"
                assert pos[b] >= self.written.get(b, 0) - ring_len, "samples were read after their place in the ring was written again"
            dst[b, :k] = ring[b, (pos[b] + np.arange(k)) % ring_len]
            dst[b, k : n_total[b]] = 0.0


def _listen_batcher(eng, rows=1, **kw):
    return _batcher(eng, listen_rows=rows, listen_chunk_frames=M, listen_max_frames=LMF, **kw)


# three utterances and an over-long one: A = frames 3..11 with a pause inside; B begins at 14; 14 loud frames from 23 are cut by the length limit
# and go on as a new utterance on the very next frame; C is a single frame
TALK = [(3, QUIET), (2, LOUD), (2, QUIET), (1, LOUD), (6, QUIET), (2, LOUD), (7, QUIET), (14, LOUD), (6, QUIET), (3, QUIET), (1, LOUD), (8, QUIET)]


def _stream(seed=1, tail=11):
    return np.concatenate([_clip(TALK, seed), np.full(tail, QUIET, np.float32)])


def _reference(S, cfg):
    """-> [(start, stop, record)] of the utterances of S, by the restated loop; `vad.utterances` must say the same."""
    mx = (RING - cfg.pre_roll(SR)) // FL
    _, records, status = R.machine(S, FL, 0.03, HANG, mx)
    assert VAD.utterances(cfg, S, SR, mx) == (records, status)
    keep = None if cfg.keep_silence_ms is None else cfg.keep(SR)
    return [R.span(rec, FL, cfg.pre_roll(SR), keep, HANG) + (rec,) for rec in records], status


def _watch(eng, bat, cfg):
    """Nothing is encoded before an onset, and no step of an utterance still open crosses B of the consumed status."""
    def check(F, active):
        for r, on in enumerate(active):
            lis = bat._listeners[r]
            if on and isinstance(lis, CSMContinuousListener):
                assert lis._utts, "encoded without an utterance"
                u = lis._utts[0]
                if not u._final:
                    c, _, o, s = lis._cst
                    assert o == u.onset_frame
                    B = min(c * FL, (s + 1) * FL + cfg.keep(SR)) - u._start
                    assert F == M and (u.frames + F) * SPF <= B, "a step of an open utterance crossed B"
    eng.on_encode = check


def _drain(lis, got, end=True):
    while True:
        try:
            u = lis.next_utterance(0)
        except queue.Empty:
            return
        if u is None:
            return
        assert isinstance(u, CSMUtterance)
        got.append((u, u.end() if end else None))


def _run(bat, lis, S, how, got, end=True):
    """Feed S: in slices of 1, 7 or 100 samples with a round behind each, or -- "at_once" -- as fast as the host queue takes it: the queue
    is filled to its cap and a round runs only when it is full."""
    if how == "at_once":
        i = 0
        while i < S.shape[0]:
            k = min(S.shape[0] - i, lis.cap - lis._qn)
            if k == 0:
                assert bat.step()
                _drain(lis, got, end)
                continue
            lis.feed(S[i : i + k])
            i += k
    else:
        k = {"ones": 1, "sevens": 7, "hundreds": 100}[how]
        for i in range(0, S.shape[0], k):
            while lis._qn + k > lis.cap:  # (the test feeds faster than any microphone: a full queue is waited for, never overrun)
                assert bat.step()
                _drain(lis, got, end)
            lis.feed(S[i : i + k])
            bat.step()
            _drain(lis, got, end)
    for _ in range(200):
        if not bat.step():
            break
        _drain(lis, got, end)
    _drain(lis, got, end)


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [0, 1, 3])
@pytest.mark.parametrize("how", ["ones", "sevens", "hundreds", "at_once"])
@pytest.mark.parametrize("kw", [{}, dict(keep_silence_ms=1.1, pre_roll_ms=0.3)], ids=["defaults", "pre-roll 7, keep 26"])
def test_every_utterance_is_a_plain_listener_fed_its_span(lag, how, kw):
    cfg = _cfg(**kw)
    S = _stream()
    assert S.shape[0] >= 5 * RING
    want, final = _reference(S, cfg)
    recs = [w[2] for w in want]
    assert len(recs) == 5 and [r[3] for r in recs] == [0, 0, 1, 0, 0] and recs[3][0] == recs[2][2] + 1 and final[2] == -1
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng)
    _watch(eng, bat, cfg)
    lis = bat.listen(vad=cfg, continuous=True)
    assert isinstance(lis, CSMContinuousListener) and lis.ring_len == RING and lis.max_frames == (RING - cfg.pre_roll(SR)) // FL
    got = []
    _run(bat, lis, S, how, got)
    lis.close()
    bat.run_until_idle()
    _drain(lis, got)
    assert lis.next_utterance(0) is None and list(lis.utterances()) == []  # the microphone has closed: nothing more comes
    assert len(got) == len(want) and bat._listeners[0] is None
    eng.enc.reset_row(0)  # (files the last stream under `streams`)
    assert len(eng.enc.streams[0]) == len(want)
    for (u, fut), (start, stop, rec), fed in zip(got, want, eng.enc.streams[0]):
        sp = u.endpoint.result(timeout=0)
        assert isinstance(sp, SpeechSpan) and (sp.start, sp.stop, sp.onset_frame, sp.endpoint_frame, sp.forced) == (start, stop, rec[0], rec[2], bool(rec[3]))
        assert u.onset == start and u.forced == bool(rec[3])
        res = fut.result(timeout=0)
        ref, ref_fed = _plain(S[start:stop])
        assert isinstance(res, ListenResult) and (res.frames, res.steps, res.samples) == (ref.frames, ref.steps, stop - start)
        assert (res.speech_start, res.speech_stop) == (start, stop) and stop - start <= RING
        np.testing.assert_array_equal(res.codes.numpy(), ref.codes.numpy())
        assert np.abs(res.codes.numpy()[0]).max() > 100  # the codes carry the samples: the comparison says something
        np.testing.assert_array_equal(np.array(fed, np.float32), ref_fed)  # every sample the row was fed, zeros behind `stop`
    assert eng.written[0] == S.shape[0] and lis.samples == S.shape[0] and lis._qn == 0
    assert len(eng.rvads) == 1 and not eng.vads and _marks(eng, "rvad_set_row") == [("rvad_set_row", 0, FL, HANG, lis.max_frames, RING)]
    bat.close()
    assert eng.rvads[0].closed


def test_launches_per_round_do_not_depend_on_the_rows():
    cfg = _cfg()
    eng = Engine(lag=1)
    bat = _listen_batcher(eng, rows=3)
    mics = [bat.listen(vad=cfg, continuous=True) for _ in range(3)]
    streams = [_stream(seed) for seed in (2, 3, 4)]
    got = [[], [], []]
    busiest = [0, 0]

    def one_round():
        mark = len(eng.calls)
        bat.step()
        for lis, g in zip(mics, got):
            _drain(lis, g)
        calls = eng.calls[mark:]
        assert len(_marks_of(calls, "convert")) <= 1 and len(_marks_of(calls, "ring_write")) <= 1 and len(_marks_of(calls, "rvad_step")) <= 1
        assert len(_marks_of(calls, "ring_read")) == len(_marks_of(calls, "encode_step")) <= 1 + (M - 1)  # an M-step and one per remainder
        busiest[0] = max([busiest[0]] + [sum(1 for k in c[1] if k) for c in _marks_of(calls, "ring_write")])
        busiest[1] = max([busiest[1]] + [len(c[2]) for c in _marks_of(calls, "encode_step")])

    for i in range(0, streams[0].shape[0], 50):
        while any(lis._qn + 50 > lis.cap for lis in mics):
            one_round()
        for lis, S in zip(mics, streams):
            lis.feed(S[i : i + 50])
        one_round()
    assert busiest == [3, 3]  # rounds in which all three rows shared the one write and the one encode step
    for lis in mics:
        lis.close()
    bat.run_until_idle()
    for lis, g, S in zip(mics, got, streams):
        _drain(lis, g)
        want, _ = _reference(S, cfg)
        assert [(u.onset, f.result(timeout=0).speech_stop) for u, f in g] == [(a, b) for a, b, _ in want]
        for (u, f), (a, b, _) in zip(g, want):
            np.testing.assert_array_equal(f.result(timeout=0).codes.numpy(), _plain(S[a:b])[0].codes.numpy())
    bat.close()


def _marks_of(calls, kind):
    return [c for c in calls if c[0] == kind]


# ---- a silent microphone, and the host queue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [0, 3])
def test_a_microphone_silent_for_ten_rings_never_fills_up(lag):
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng)
    lis = bat.listen(vad=_cfg(), continuous=True)
    g = np.random.default_rng(5)
    most = 0
    # 40 samples a round: with the status 4 rounds behind, 160 samples are in flight, within the ring of 240 -- as a real microphone's
    # samples of a few rounds are within a ring of seconds
    for _ in range(10 * RING // 40 + 1):
        lis.feed((QUIET * g.standard_normal(40)).astype(np.float32))
        bat.step()
        most = max(most, lis._qn)
    bat.run_until_idle()
    assert lis.samples > 10 * RING and eng.written[0] == lis.samples and most <= lis.cap and lis._qn == 0
    assert not eng.enc.calls and not _marks(eng, "ring_read")
    with pytest.raises(queue.Empty):
        lis.next_utterance(0)
    assert lis.cancel() and bat._listeners[0] is None
    bat.close()


def test_a_feed_beyond_the_host_cap_raises_with_nothing_changed():
    eng = Engine()
    bat = _listen_batcher(eng)
    lis = bat.listen(vad=_cfg(), continuous=True)
    assert lis.cap == RING
    a = _clip([(4, QUIET)], 3)
    lis.feed(a)
    with pytest.raises(ValueError, match="listen_max_frames"):
        lis.feed(np.zeros(RING - a.shape[0] + 1, np.float32))
    assert lis._qn == lis.samples == a.shape[0] and len(lis._q) == 1
    lis.feed(np.zeros(RING - a.shape[0], np.float32))  # exactly the cap is taken
    bat.run_until_idle()
    assert lis._qn == 0 and eng.written[0] == RING
    lis.feed(np.zeros(RING, np.float32))  # ... and drained, the queue takes a whole cap again
    with pytest.raises(ValueError, match="continuous=True needs vad"):
        bat.listen(continuous=True)
    bat.close()
    with pytest.raises(RuntimeError):
        lis.feed(a)


# ---- close(), and an utterance nobody ends ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [0, 1, 3])
@pytest.mark.parametrize("tail", [0, 11, 2 * FL + 5])
def test_close_with_an_open_utterance(lag, tail):
    cfg = _cfg()
    S = np.concatenate([_clip([(2, QUIET), (3, LOUD)]), np.full(tail, QUIET, np.float32)])
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng)
    _watch(eng, bat, cfg)
    lis = bat.listen(vad=cfg, continuous=True)
    got = []
    _run(bat, lis, S, "sevens", got)
    assert len(got) == 1 and not got[0][0].endpoint.done()
    lis.close()
    with pytest.raises(ValueError, match="closed"):
        lis.feed(S)
    bat.run_until_idle()
    u, fut = got[0]
    res = fut.result(timeout=0)
    assert u.endpoint.cancelled() and (res.speech_start, res.speech_stop) == (2 * FL, S.shape[0])  # as a one-shot listener ended there
    ref, ref_fed = _plain(S[2 * FL :])
    assert (res.frames, res.steps) == (ref.frames, ref.steps)
    np.testing.assert_array_equal(res.codes.numpy(), ref.codes.numpy())
    np.testing.assert_array_equal(np.array(eng.enc.fed[0], np.float32), ref_fed)
    assert bat._listeners[0] is None and lis.next_utterance(0) is None  # the row is freed when the utterance has resolved
    bat.close()


@pytest.mark.parametrize("lag", [0, 3])
def test_an_utterance_never_ended_is_dropped_when_the_next_one_needs_its_place(lag):
    cfg = _cfg()
    S = _stream()
    want, _ = _reference(S, cfg)
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng)
    lis = bat.listen(vad=cfg, continuous=True)
    got = []
    _run(bat, lis, S, "hundreds", got, end=False)  # nobody ends anything
    assert len(got) == len(want) and eng.written[0] == S.shape[0]  # ... and the stream still went through whole
    for u, _ in got[:-1]:
        assert u.dropped and u.endpoint.done()
        with pytest.raises(ValueError, match="dropped"):
            u.end()
    last = got[-1][0]
    assert not last.dropped and last.frames == -(-(want[-1][1] - want[-1][0]) // SPF)  # the last one keeps its place: nothing needs it
    fut = last.end()
    bat.run_until_idle()
    np.testing.assert_array_equal(fut.result(timeout=0).codes.numpy(), _plain(S[want[-1][0] : want[-1][1]])[0].codes.numpy())
    assert lis.cancel()
    bat.close()


# ---- a session ----------------------------------------------------------------------------------------------------------------------------------
def test_each_end_enters_the_history_and_barge_in_interrupts_on_the_second_onset():
    cfg = _cfg()
    eng = Engine(lag=1, max_pos=2048)
    bat = _listen_batcher(eng)
    sess = bat.session()
    first = sess.submit([3, 3, 1], max_audio_length_ms=80 * 2)
    bat.run_until_idle()
    assert first.result(timeout=0).frames == 2
    heard = []
    eng.heard_segment = lambda speaker, text, audio, f=eng.heard_segment: (heard.append(np.asarray(audio)), f(speaker, text, audio))[1]
    lis = sess.listen(1, vad=cfg, continuous=True, barge_in=True)
    A = _clip([(1, QUIET), (2, LOUD), (6, QUIET)], 6)
    lis.feed(A)
    bat.run_until_idle()
    u1 = lis.next_utterance(0)
    assert u1.endpoint.done() and bat.stats["interrupted"] == 0  # no turn was live: nothing to interrupt
    with pytest.raises(ValueError, match="text"):
        u1.end()
    f1 = u1.end([9, 9])
    assert sess.busy
    bat.run_until_idle()
    r1 = f1.result(timeout=0)
    assert not sess.busy and sess.turns[-1] == (1, [9, 9], 0) and (r1.speech_start, r1.speech_stop) == (FL, 7 * FL)
    np.testing.assert_array_equal(heard[0], A[FL : 7 * FL])  # the turn enters the history from S[start:stop], read out of the ring
    frames_before = sess.history[0].shape[0]
    turn = sess.submit([3, 2], max_audio_length_ms=80 * 60)
    for _ in range(4):
        assert bat.step()
    assert not turn.done() and sess.busy
    B = _clip([(2, LOUD), (6, QUIET)], 7)
    lis.feed(B)
    rounds = 0
    while True:
        try:
            u2 = lis.next_utterance(0)
            break
        except queue.Empty:
            assert not turn.done()
            bat.step()
            rounds += 1
    res = turn.result(timeout=0)  # the round that consumed the second onset has ended the turn
    assert res.interrupted and bat.stats["interrupted"] == 1 and rounds == 3 and u2.onset == A.shape[0]
    bat.run_until_idle()
    f2 = u2.end([7])
    bat.run_until_idle()
    r2 = f2.result(timeout=0)
    assert (r2.speech_start, r2.speech_stop) == (A.shape[0], A.shape[0] + 6 * FL) and sess.turns[-1] == (1, [7], 0)
    np.testing.assert_array_equal(heard[1], B[: 6 * FL])
    assert sess.history[0].shape[0] > frames_before + r2.frames
    lis.close()
    bat.run_until_idle()
    assert bat._listeners[0] is None
    bat.close()


# ---- beside the listeners that were there before ---------------------------------------------------------------------------------------------------
def _neighbours(with_mic, lag):
    """A plain listener in row 0 and a one-shot VAD listener in row 1, fed and ended the same way, with or without a continuous listener
    in row 2 -> the engine's calls that touch rows 0 and 1, and the two results."""
    cfg = _cfg()
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng, rows=3)
    a, b = bat.listen(), bat.listen(vad=cfg)
    mic = bat.listen(vad=cfg, continuous=True) if with_mic else None
    ca, cb, S = _clip([(4, LOUD)], 4), _clip([(2, QUIET), (2, LOUD), (5, QUIET)], 2), _stream(9)
    got = []
    for r in range(16):
        a.feed(ca[50 * r : 50 * r + 50])
        b.feed(cb[50 * r : 50 * r + 50])
        if mic is not None and mic._qn + 40 <= mic.cap:
            mic.feed(S[40 * r : 40 * r + 40])
        bat.step()
        if mic is not None:
            _drain(mic, got)
    fa, fb = a.end(), b.end()
    bat.run_until_idle()
    if mic is not None:
        _drain(mic, got)
        assert got and got[0][0].endpoint.done() and mic.cancel()

    def theirs(c):
        if c[0] in ("ring_write", "ring_read", "rvad_step", "rvad_set_row"):
            return False
        if c[0] == "encode_step":
            return c[2] != (2,)
        if c[0] == "convert":
            return any(c[4][:2])
        return c != ("enc_reset", 2)

    out = [(c[0], c[1], c[2][:2], c[3][:2], c[4][:2]) if c[0] == "convert" else c for c in eng.calls if theirs(c)]
    bat.close()
    return out, fa.result(timeout=0), fb.result(timeout=0), bool(eng.rvads)


@pytest.mark.parametrize("lag", [0, 3])
def test_a_plain_and_a_one_shot_listener_beside_a_continuous_one_keep_their_calls(lag):
    alone, ra, rb, made = _neighbours(False, lag)
    assert not made  # without a continuous listener none of the new objects is made
    beside, sa, sb, made = _neighbours(True, lag)
    assert made
    want, have = alone, beside
    assert have == want and any(c[0] == "encode_step" for c in want) and any(c[0] == "vad_step" for c in want)
    for x, y in ((ra, sa), (rb, sb)):
        assert (x.frames, x.steps, x.speech_start, x.speech_stop) == (y.frames, y.steps, y.speech_start, y.speech_stop)
        np.testing.assert_array_equal(x.codes.numpy(), y.codes.numpy())
