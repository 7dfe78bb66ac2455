"""Voice-activity endpointing and barge-in for listeners (`listen(vad=)`, `CSMSession.listen(vad=, barge_in=)`) against the
scripted engine and encoder of test_csm_listen_cpu.py (no device) and a numpy row detector whose status table becomes ready only k rounds
after its step, k in {0, 1, 3}: the lag of the non-blocking hand-back.  The detector is tests/_vad_ref.py's state machine on the real
surface (`set_row`, `step`, `fetch` -> ticket).  Checked: a VAD listener's codes, frames and steps -- and every sample its encoder row was fed,
the zeros behind `stop` included -- are those of a plain listener fed clip[start:stop] and ended, whatever the slicing and the lag; nothing
is encoded before the onset and no step of an open listener crosses B; the futures; `end()` before the endpoint and without speech; a
barge-in; and that a listener without `vad` makes no detector and no converter."""
import os
import sys
from concurrent.futures import CancelledError

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _vad_ref as V  # noqa: E402
from test_csm_formats_cpu import Converter  # noqa: E402
from test_csm_interrupt_cpu import N_CB, SPF, _batcher, _marks  # noqa: E402
from test_csm_listen_cpu import Encoder as _Encoder, Engine as _Engine  # noqa: E402

from mlx_audio_amd.csm_serve import ListenResult, SpeechSpan  # noqa: E402
from mlx_audio_amd.vad import NO_STATUS, VadConfig  # noqa: E402

M, MAX_FRAMES, SR = 3, 400, 24000
FL, HANG = 24, 3                 # 1 ms at 24 kHz: 24 samples, 8 codec frames of the scripted codec; the row ends at the 4th silent frame
QUIET, LOUD = 0.001, 0.5         # rms against the threshold 0.03


def _cfg(**kw):
    cfg = VadConfig(frame_ms=1, threshold=0.03, silence_ms=HANG, **kw)
    assert cfg.frame_len(SR) == FL and cfg.hang_frames == HANG
    return cfg


class Ticket:
    def __init__(self, table, lag):
        self.table, self.left = table, lag

    def ready(self):
        if self.left > 0:
            self.left -= 1
            return False
        return True

    def take(self):
        assert self.left == 0, "a status was read before it was ready: that is a sync"
        return self.table


class NumpyVad:
    """The surface of `vad.RowVad`: the kernel's rule E >= thr2n on float64 energies and the reference's state machine."""

    def __init__(self, engine, rows):
        self.engine, self.rows, self.closed = engine, [None] * rows, False
        self.status = np.array([NO_STATUS] * rows, np.int32)

    def set_row(self, row, frame_len, thr2n, hang):
        self.rows[row] = dict(fl=int(frame_len), thr=float(thr2n), hang=int(hang), n=0, speaking=False, silent=0)
        self.status[row] = NO_STATUS
        self.engine.calls.append(("vad_set_row", row, frame_len, hang))

    def step(self, x, n_avail):
        assert not self.closed and len(n_avail) == len(self.rows) and x.shape[0] == len(self.rows)
        took = []
        for r, st in enumerate(self.rows):
            if st is None:
                continue
            assert st["n"] <= n_avail[r] <= x.shape[1], "n_avail below the row's previous one, or beyond the buffer"
            st["n"] = n_avail[r]
            c, o, s, e = (int(v) for v in self.status[r])
            upto = n_avail[r] // st["fl"]
            if e >= 0 or upto <= c:
                continue
            took.append(r)
            en = V.energies(x[r, : upto * st["fl"]].numpy(), st["fl"])
            while c < upto and e < 0:
                if en[c] >= st["thr"]:
                    st["speaking"], st["silent"], s = True, 0, c
                    o = c if o < 0 else o
                elif st["speaking"]:
                    st["silent"] += 1
                    if st["silent"] > st["hang"]:
                        e = c
                c += 1
            self.status[r] = (c, o, s, e)
        self.engine.calls.append(("vad_step", tuple(took)))

    def fetch(self):
        return Ticket(self.status.copy(), self.engine.lag)

    def close(self):
        self.closed = True


class Encoder(_Encoder):
    """A frame's codes are [its first sample in thousandths, its index + 1]; `fed[row]` is every sample the row's stream was fed."""

    def __init__(self, *a):
        super().__init__(*a)
        self.fed = [[] for _ in range(self.max_batch)]

    def reset_row(self, row):
        super().reset_row(row)
        self.fed[row] = []

    def step(self, pcm, active):
        F = pcm.shape[2] // SPF
        if self.engine.on_encode is not None:
            self.engine.on_encode(F, active)
        codes = torch.zeros((self.max_batch, N_CB, F), dtype=torch.int32)
        rows = tuple(r for r, on in enumerate(active) if on)
        for r in rows:
            x = pcm[r, 0].tolist()
            assert self.frames[r] + F <= self.max_frames
            self.fed[r] += x
            for f in range(F):
                codes[r, 0, f], codes[r, 1, f] = int(round(x[f * SPF] * 1000)), self.frames[r] + f + 1
            self.frames[r] += F
        self.calls.append((F, rows))
        self.engine.calls.append(("encode_step", F, rows))
        return codes


class Engine(_Engine):
    def __init__(self, lag=0, **kw):
        super().__init__(**kw)
        self.lag, self.vads, self.converters, self.on_encode = lag, [], [], None

    def row_encoder(self, max_batch, max_frames, max_chunk):
        self.enc = Encoder(self, max_batch, max_frames, max_chunk)
        return self.enc

    def row_vad(self, max_rows):
        self.vads.append(NumpyVad(self, max_rows))
        return self.vads[-1]

    def pcm_converter(self):
        self.converters.append(Converter(self))
        return self.converters[-1]


def _listen_batcher(eng, rows=2, **kw):
    return _batcher(eng, listen_rows=rows, listen_chunk_frames=M, listen_max_frames=MAX_FRAMES, **kw)


def _clip(layout, seed=1):
    """layout: (frames, level) pieces of detector frames; every sample differs from its neighbours (a row fed the wrong ones shows)."""
    g = np.random.default_rng(seed)
    rms = [lv for n, lv in layout for _ in range(n)]
    return V.noise_clip(g, FL, rms)


TALK = [(3, QUIET), (2, LOUD), (2, QUIET), (3, LOUD), (9, QUIET)]  # onset 3, a pause of 2 (< hang), last speech 9, endpoint 13; 5 frames follow


def _plain(clip):
    """(ListenResult, everything the encoder row was fed) of a plain listener fed `clip` and ended, on a batcher that never saw a detector."""
    eng = Engine()
    bat = _listen_batcher(eng, rows=1)
    lis = bat.listen()
    lis.feed(clip)
    fut = lis.end()
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert not eng.vads and not eng.converters and bat._vad is None
    fed = np.array(eng.enc.fed[0], np.float32)
    bat.close()
    return res, fed


def _watch(eng, bat, cfg):
    """Every encode step of an OPEN VAD listener stays below B = min(classified fl, (last_speech + 1) fl + keep) - start of the status it
    has consumed, and none runs before an onset."""
    def check(F, active):
        for r, on in enumerate(active):
            lis = bat._listeners[r]
            if on and lis is not None and lis.vad is not None:
                c, o, s, e = lis._vst
                assert o >= 0 and lis.onset.done(), "encoded before the onset"
                if not lis._vclosed:
                    B = min(c * FL, (s + 1) * FL + cfg.keep(SR)) - lis._vstart
                    assert F == M and (lis.frames + F) * SPF <= B, "a step of an open listener crossed B"
    eng.on_encode = check


def _feed(bat, lis, clip, how):
    if how == "at_once":
        lis.feed(clip)
        return
    k = {"ones": 1, "sevens": 7, "frames": FL}[how]
    for i in range(0, clip.shape[0], k):
        lis.feed(clip[i : i + k])
        bat.step()


# ---- the span's codes are a plain listener's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [0, 1, 3])
@pytest.mark.parametrize("how", ["at_once", "sevens", "frames"])
@pytest.mark.parametrize("kw", [{}, dict(pre_roll_ms=0.3), dict(keep_silence_ms=1.1, pre_roll_ms=5)])
def test_codes_frames_and_steps_are_those_of_a_plain_listener_fed_the_span(lag, how, kw):
    cfg = _cfg(**kw)
    clip = _clip(TALK)
    flags, status = V.machine(clip, FL, 0.03, HANG)
    assert status == (14, 3, 9, 13)
    keep = None if cfg.keep_silence_ms is None else cfg.keep(SR)
    start, stop = V.span(status, clip.shape[0], FL, cfg.pre_roll(SR), keep, HANG)
    assert (start, stop) == {0: (72, 336), 7: (65, 336), 120: (0, 266)}[cfg.pre_roll(SR)]
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng, rows=1)
    _watch(eng, bat, cfg)
    lis = bat.listen(vad=cfg)
    assert lis.onset is not None and not lis.onset.done() and not lis.endpoint.done()
    _feed(bat, lis, clip, how)
    bat.run_until_idle()
    assert lis.onset.result(timeout=0) == start
    sp = lis.endpoint.result(timeout=0)
    assert isinstance(sp, SpeechSpan) and (sp.start, sp.stop, sp.onset_frame, sp.endpoint_frame) == (start, stop, 3, 13)
    assert (sp.sample_rate, sp.rate_start, sp.rate_stop) == (SR, start, stop)
    want, want_fed = _plain(clip[start:stop])
    T = -(-(stop - start) // SPF)
    assert lis.frames == T == want.frames and lis.steps == want.steps  # the whole span is encoded at the endpoint, before any `end()`
    steps_before = len(eng.enc.calls)
    fed_before = lis.samples
    lis.feed(_clip([(2, LOUD)], seed=9))  # behind the endpoint: accepted and ignored
    bat.run_until_idle()
    assert lis.samples == fed_before and len(eng.enc.calls) == steps_before
    fut = lis.end()
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert isinstance(res, ListenResult) and len(eng.enc.calls) == steps_before  # `end()` resolves without further encode steps
    assert (res.speech_start, res.speech_stop, res.frames, res.steps) == (start, stop, want.frames, want.steps)
    assert want.speech_start is None and want.speech_stop is None
    np.testing.assert_array_equal(res.codes.numpy(), want.codes.numpy())
    assert np.abs(res.codes.numpy()[0]).max() > 100  # the codes carry the samples: the comparison says something
    np.testing.assert_array_equal(np.array(eng.enc.fed[0], np.float32), want_fed)  # zeros, not the samples heard there, behind `stop`
    assert (stop - start) % SPF == 0 or want_fed[stop - start :].tolist() == [0.0] * (T * SPF - (stop - start))
    assert len(eng.vads) == 1 and len(eng.converters) == 1  # an f32 listener at the model's rate goes through the converter
    assert _marks(eng, "vad_set_row") == [("vad_set_row", 0, FL, HANG)]
    bat.close()
    assert eng.vads[0].closed


@pytest.mark.parametrize("lag", [0, 1, 3])
def test_two_listeners_and_a_neighbour_without_vad(lag):
    cfg = _cfg()
    a_clip, b_clip, c_clip = _clip(TALK, 2), _clip([(1, LOUD), (6, QUIET)], 3), _clip([(4, LOUD)], 4)
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng, rows=3)
    _watch(eng, bat, cfg)
    a, b, c = bat.listen(vad=cfg), bat.listen(vad=cfg), bat.listen()
    for i in range(0, a_clip.shape[0], 50):
        a.feed(a_clip[i : i + 50])
        b.feed(b_clip[i : i + 50])
        c.feed(c_clip[i : i + 50])
        bat.step()
    fa, fb, fc = a.end(), b.end(), c.end()
    bat.run_until_idle()
    for fut, clip, span in ((fa, a_clip, (72, 336)), (fb, b_clip, (0, 120)), (fc, c_clip, None)):
        res = fut.result(timeout=0)
        want, _ = _plain(clip if span is None else clip[span[0] : span[1]])
        assert (res.frames, res.steps) == (want.frames, want.steps) and (res.speech_start, res.speech_stop) == (span or (None, None))
        np.testing.assert_array_equal(res.codes.numpy(), want.codes.numpy())
    assert b.endpoint.result(timeout=0).endpoint_frame == 4
    bat.close()


# ---- end() --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [0, 1, 3])
@pytest.mark.parametrize("tail", [0, 11, 2 * FL + 5])
def test_end_before_the_endpoint(lag, tail):
    cfg = _cfg()
    clip = np.concatenate([_clip([(2, QUIET), (3, LOUD)]), np.full(tail, QUIET, np.float32)])
    n = clip.shape[0]
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng, rows=1)
    _watch(eng, bat, cfg)
    lis = bat.listen(vad=cfg)
    _feed(bat, lis, clip, "sevens")
    fut = lis.end()
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert lis.onset.result(timeout=0) == 2 * FL and lis.endpoint.cancelled()  # the caller was first: there was no endpoint
    assert (res.speech_start, res.speech_stop) == (2 * FL, n)  # a partial last frame is never classified: silence, and within the hang it is kept
    want, want_fed = _plain(clip[2 * FL : n])
    assert (res.frames, res.steps, res.samples) == (want.frames, want.steps, n)
    np.testing.assert_array_equal(res.codes.numpy(), want.codes.numpy())
    np.testing.assert_array_equal(np.array(eng.enc.fed[0], np.float32), want_fed)
    bat.close()


@pytest.mark.parametrize("lag", [0, 3])
def test_end_with_no_speech_fails_and_leaves_the_session_as_it_was(lag):
    eng = Engine(lag=lag)
    bat = _listen_batcher(eng, rows=1)
    sess = bat.session()
    first = sess.submit([3, 3, 1], max_audio_length_ms=80 * 2)
    bat.run_until_idle()
    assert first.result(timeout=0).frames == 2
    before = (list(sess.turns), sess.length, sess.n, sess.pending[0].tolist(), sess.history[0].tolist())
    lis = sess.listen(1, vad=_cfg())
    lis.feed(_clip([(7, QUIET)]))
    bat.run_until_idle()
    assert not eng.enc.calls and not lis.onset.done()
    fut = lis.end([9, 9])
    assert sess.busy
    bat.run_until_idle()
    with pytest.raises(ValueError, match="no speech"):
        fut.result(timeout=0)
    assert not sess.busy and (list(sess.turns), sess.length, sess.n, sess.pending[0].tolist(), sess.history[0].tolist()) == before
    assert not eng.enc.calls and lis.onset.cancelled() and lis.endpoint.cancelled()
    nxt = sess.listen(1, vad=_cfg())  # the row is free again
    assert nxt.row == 0 and nxt.cancel()
    with pytest.raises(CancelledError):
        nxt.onset.result(timeout=0)
    bat.close()


def test_a_session_hears_the_span():
    eng = Engine(lag=1)
    bat = _listen_batcher(eng, rows=1)
    sess = bat.session()
    clip = _clip(TALK, 5)
    lis = sess.listen(1, vad=_cfg())
    lis.feed(clip)
    bat.run_until_idle()
    heard = []
    eng.heard_segment = lambda speaker, text, audio, f=eng.heard_segment: (heard.append(np.asarray(audio)), f(speaker, text, audio))[1]
    fut = lis.end([9, 9])
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert sess.turns[-1] == (1, [9, 9], 0) and not sess.busy
    np.testing.assert_array_equal(heard[0], clip[72:336])  # the turn enters the history from heard[start:stop] ...
    assert sess.history[0].shape[0] == 2 + res.frames + 1 and res.frames == 88  # ... and its codes
    bat.close()


# ---- barge-in -----------------------------------------------------------------------------------------------------------------------------
def _live_turn(lag, **kw):
    eng = Engine(lag=lag, max_pos=512)  # (room for a heard turn of 56 frames)
    bat = _listen_batcher(eng, rows=1, **kw)
    sess = bat.session()
    first = sess.submit([3, 3, 1], max_audio_length_ms=80 * 2)
    bat.run_until_idle()
    assert first.result(timeout=0).frames == 2 and sess.n == 4
    turn = sess.submit([3, 2], max_audio_length_ms=80 * 30)  # L = 4 + 2 + 2 = 8
    for _ in range(4):
        assert bat.step()
    assert len(bat._rows[0].codes) == 5 and sess.busy
    return eng, bat, sess, turn


@pytest.mark.parametrize("lag", [0, 1, 3])
def test_barge_in_interrupts_the_live_turn_in_the_round_the_onset_is_consumed(lag):
    eng, bat, sess, turn = _live_turn(lag)
    lis = sess.listen(1, vad=_cfg(), barge_in=True)
    clip = _clip([(1, QUIET), (3, LOUD), (5, QUIET)], 6)
    lis.feed(clip)
    rounds = 0
    while not lis.onset.done():
        assert not turn.done()
        bat.step()
        rounds += 1
    assert rounds == lag + 2  # one round steps the detector, `lag` rounds find the status not ready, the next consumes it
    res = turn.result(timeout=0)  # ... and that same round has ended the turn
    k = 5 + rounds - 1            # a frame per round before it
    assert res.interrupted and res.frames == k and sess.turns[-1] == (0, [3, 2], k) and bat.stats["interrupted"] == 1
    assert sess.n == 8 + k - 1    # exactly k frames exist: the last was sampled and never fed, as at a limit of k
    fut = lis.end([9])
    bat.run_until_idle()
    heard = fut.result(timeout=0)
    assert (heard.speech_start, heard.speech_stop) == (FL, 8 * FL)
    nxt = sess.submit([3, 3, 4], max_audio_length_ms=80 * 2)  # the next turn is conditioned on the k emitted frames and on what was heard
    bat.run_until_idle()
    assert nxt.result(timeout=0).frames == 2
    assert _marks(eng, "admit")[-1] == ("admit", 0, 4, 8 + k - 1, 2 + (1 + heard.frames + 1) + 3)
    bat.close()


def test_without_barge_in_the_turn_is_untouched():
    eng, bat, sess, turn = _live_turn(1)
    lis = sess.listen(1, vad=_cfg())
    lis.feed(_clip([(1, QUIET), (3, LOUD), (5, QUIET)], 6))
    bat.run_until_idle()
    res = turn.result(timeout=0)
    assert lis.onset.done() and lis.endpoint.done() and not res.interrupted and res.frames == 30 and bat.stats["interrupted"] == 0
    bat.close()


def test_barge_in_on_a_queued_turn_and_the_refusals():
    eng = Engine()
    bat = _listen_batcher(eng, rows=1, max_batch=1)
    other = bat.submit(None, [3, 3, 5], max_audio_length_ms=80 * 40, voice_match=False)
    sess = bat.session()
    assert bat.step()
    turn = sess.submit([3, 2], max_audio_length_ms=80 * 3)  # queued behind `other`
    with pytest.raises(ValueError, match="barge_in needs vad"):
        sess.listen(1, barge_in=True)
    with pytest.raises(ValueError, match="session"):
        bat.listen(vad=True, barge_in=True)
    with pytest.raises(ValueError, match="VadConfig"):
        bat.listen(vad="yes")
    with pytest.raises(ValueError, match="4096"):
        bat.listen(vad=VadConfig(frame_ms=200))
    lis = sess.listen(1, vad=_cfg(), barge_in=True)
    lis.feed(_clip([(2, LOUD)]))
    for _ in range(3):
        bat.step()
    assert lis.onset.done() and turn.cancelled() and not other.done()  # an interrupt of a turn nobody has heard yet: a cancel
    assert lis.cancel()
    bat.close()


# ---- without vad nothing of this exists ------------------------------------------------------------------------------------------------------
def test_a_listener_without_vad_takes_the_path_it_took():
    eng = Engine()
    bat = _listen_batcher(eng, rows=2)
    a = bat.listen()
    clip = _clip([(3, LOUD)], 7)[: 7 * SPF + 1]
    a.feed(clip)
    fut = a.end()
    bat.run_until_idle()
    assert fut.result(timeout=0).steps == [3, 3, 2] and bat.stats["listen_rounds"] == 3
    assert bat._vad is None and not eng.vads and not eng.converters and a.onset is None and a.endpoint is None
    assert [c for c in eng.calls if c[0] != "enc_reset"] == [("encode_step", 3, (0,)), ("encode_step", 3, (0,)), ("encode_step", 2, (0,))]
    # ... also beside a detector that an earlier listener made: a round without VAD samples steps nothing of it
    v = bat.listen(vad=_cfg())
    v.feed(_clip([(2, LOUD)], 8))
    fv = v.end()
    bat.run_until_idle()
    assert fv.result(timeout=0).speech_stop == 2 * FL and len(eng.vads) == 1
    mark = len(eng.calls)
    b = bat.listen()
    b.feed(clip)
    fb = b.end()
    bat.run_until_idle()
    assert fb.result(timeout=0).steps == [3, 3, 2]
    assert [c for c in eng.calls[mark:] if c[0] != "enc_reset"] == [("encode_step", 3, (0,)), ("encode_step", 3, (0,)), ("encode_step", 2, (0,))]
    bat.close()
