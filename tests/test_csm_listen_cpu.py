"""Listening (`CSMBatcher(listen_rows=K)`, `listen()` / `CSMSession.listen()`) against a scripted engine and a scripted row
encoder that records its `step` calls (no device): the round policy -- aligned M-rounds, at most one per scheduling round, tails grouped by
equal remainder, a listener's steps [M] * (T // M) + [T % M] whatever the slicing of `feed` and the thread that feeds --, that `feed` and `end`
wake an idle worker, that `run_until_idle` drains due rounds with no live row, the session's busy rules, `stats`, and that `listen_rows=0`
leaves `step()` as it was.  The scripted encoder checks that every row is fed its own next samples from sample 0 after a reset."""
import os
import sys
import threading
from concurrent.futures import CancelledError

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_csm_interrupt_cpu import N_CB, SPF, Engine as _Engine, _batcher, _marks, _req, _text  # noqa: E402

from mlx_audio_amd.csm_serve import CSMListener, ListenResult  # noqa: E402
from mlx_audio_amd.sesame import Segment  # noqa: E402

M = 3


def _clip(tag, samples):
    """Sample i of microphone `tag` is tag * 1000 + i + 1 (never zero: zeros are padding)."""
    return (tag * 1000 + 1 + np.arange(samples)).astype(np.float32)


def _want(tag, samples):
    """Codes [N_CB, T] of the scripted encoder for that clip: frame f = [its first sample, f + 1]."""
    T = -(-samples // SPF)
    return np.array([[tag * 1000 + 1 + f * SPF for f in range(T)], [f + 1 for f in range(T)]], np.int32)


class Encoder:
    """The row encoder's surface.  A frame's codes are [its first sample, its index + 1]; every active row must be fed the samples that
    follow its last ones (or zeros: padding), starting over after `reset_row`."""

    def __init__(self, engine, max_batch, max_frames, max_chunk):
        self.engine, self.max_batch, self.max_frames, self.max_chunk = engine, max_batch, max_frames, max_chunk
        self.frames, self.next, self.calls, self.closed = [0] * max_batch, [None] * max_batch, [], False
        self.stepped = threading.Event()

    def reset_row(self, row):
        self.frames[row], self.next[row] = 0, None
        self.engine.calls.append(("enc_reset", row))

    def step(self, pcm, active):
        assert not self.closed and tuple(pcm.shape[:2]) == (self.max_batch, 1) and pcm.shape[2] % SPF == 0
        F = pcm.shape[2] // SPF
        assert 1 <= F <= self.max_chunk
        codes = torch.zeros((self.max_batch, N_CB, F), dtype=torch.int32)
        rows = tuple(r for r, on in enumerate(active) if on)
        for r in rows:
            x = pcm[r, 0].tolist()
            assert self.frames[r] + F <= self.max_frames
            for i, v in enumerate(x):
                if v != 0:
                    assert self.next[r] is None and self.frames[r] == 0 and i == 0 or v == self.next[r], "a row was not fed its own next samples"
                    self.next[r] = v + 1
            for f in range(F):
                codes[r, 0, f], codes[r, 1, f] = int(x[f * SPF]), self.frames[r] + f + 1
            self.frames[r] += F
        self.calls.append((F, rows))
        self.engine.calls.append(("encode_step", F, rows))
        self.stepped.set()
        return codes

    def close(self):
        self.closed = True


class Engine(_Engine):
    def row_encoder(self, max_batch, max_frames, max_chunk):
        self.enc = Encoder(self, max_batch, max_frames, max_chunk)
        return self.enc

    def heard_segment(self, speaker, text, audio):
        return Segment(speaker=speaker, text=text, audio=audio)

    def segment_frames(self, segment, codes=None):
        """Text frames, audio frames, EOS frame: the layout of `Model._tokenize_segment(add_eos=True)`."""
        assert segment.audio is not None and codes is not None
        tf, tm = _text(segment.text)
        T = codes.shape[1]
        af, am = np.zeros((T + 1, N_CB + 1), np.int32), np.zeros((T + 1, N_CB + 1), np.float32)
        af[:T, :N_CB], am[:, :N_CB] = np.asarray(codes).T, 1
        return np.concatenate([tf, af]), np.concatenate([tm, am])


def _listen_batcher(eng, rows=3, **kw):
    return _batcher(eng, listen_rows=rows, listen_chunk_frames=M, listen_max_frames=12, **kw)


def _check(res, tag, samples):
    assert isinstance(res, ListenResult)
    T = -(-samples // SPF)
    assert res.frames == T and res.samples == samples and res.steps == [M] * (T // M) + ([T % M] if T % M else [])
    np.testing.assert_array_equal(res.codes.numpy(), _want(tag, samples))


# ---- the round policy --------------------------------------------------------------------------------------------------------------------------
def test_aligned_rounds_at_most_one_full_round_per_scheduling_round():
    eng = Engine()
    bat = _listen_batcher(eng)
    a, b = bat.listen(), bat.listen()
    assert isinstance(a, CSMListener) and (a.row, b.row) == (0, 1)
    a.feed(_clip(1, 7 * SPF - 1))  # a long clip at once: 6 whole frames
    b.feed(_clip(2, 2 * SPF))      # not a round's worth yet
    assert not eng.enc.calls       # (the caller's thread encodes nothing)
    assert bat.step() and eng.enc.calls == [(M, (0,))]
    b.feed(_clip(2, 2 * SPF)[:0])  # (an empty slice is fine)
    b.feed((2000 + 1 + 2 * SPF + np.arange(SPF)).astype(np.float32))  # b's third frame
    assert bat.step() and eng.enc.calls[1:] == [(M, (0, 1))]  # both rows in ONE step
    assert (a.frames, b.frames) == (6, 3) and a.codes().shape == (N_CB, 6)
    assert not bat.step() and len(eng.enc.calls) == 2  # a's seventh frame is partial and a has not ended: nothing is due
    fa = a.end()
    assert bat.step() and eng.enc.calls[2:] == [(1, (0,))] and fa.done()
    _check(fa.result(timeout=0), 1, 7 * SPF - 1)
    fb = b.end()
    assert bat.step() and len(eng.enc.calls) == 3  # b had nothing left: it resolves without a step
    _check(fb.result(timeout=0), 2, 3 * SPF)
    assert not bat.step()
    assert _marks(eng, "enc_reset") == [("enc_reset", 0), ("enc_reset", 1)]
    assert bat.stats["listen_rounds"] == 3 and bat.stats["listen_frames"] == 10 and "listen_seconds" in bat.stats
    bat.close()
    assert eng.enc.closed


def test_tails_are_grouped_by_equal_remainder():
    eng = Engine()
    bat = _listen_batcher(eng)
    ls = [bat.listen() for _ in range(3)]
    sizes = [4 * SPF, 4 * SPF - 2, 8 * SPF]  # T = 4, 4, 8: remainders 1, 1, 2
    for i, (lis, n) in enumerate(zip(ls, sizes)):
        lis.feed(_clip(i + 1, n))
    futs = [lis.end() for lis in ls]
    assert bat.step()  # one full round for all three, then the tails of rows 0 and 1 in ONE step; row 2 still holds 5 frames
    assert eng.enc.calls == [(M, (0, 1, 2)), (1, (0, 1))] and futs[0].done() and futs[1].done() and not futs[2].done()
    assert bat.step()
    assert eng.enc.calls[2:] == [(M, (2,)), (2, (2,))] and futs[2].done()
    for i, (f, n) in enumerate(zip(futs, sizes)):
        _check(f.result(timeout=0), i + 1, n)
    assert not bat.step()
    bat.close()


@pytest.mark.parametrize("how", ["at_once", "slices", "thread"])
def test_the_steps_do_not_depend_on_how_the_audio_was_fed(how):
    eng = Engine()
    bat = _listen_batcher(eng, rows=1)
    lis, n = bat.listen(), 8 * SPF - 1
    clip = _clip(5, n)
    if how == "at_once":
        lis.feed(clip)
        bat.run_until_idle()
    elif how == "slices":
        for i in range(0, n, 2):
            lis.feed(clip[i : i + 2])
            bat.step()
    else:
        t = threading.Thread(target=lambda: [lis.feed(clip[i : i + 5]) for i in range(0, n, 5)])
        t.start()
        t.join()
        bat.step()
    fut = lis.end()
    bat.run_until_idle()
    _check(fut.result(timeout=0), 5, n)
    assert [c[0] for c in eng.enc.calls] == [3, 3, 2]
    bat.close()


def test_run_until_idle_drains_due_rounds_with_no_live_row():
    eng = Engine()
    bat = _listen_batcher(eng)
    lis = bat.listen()
    lis.feed(_clip(1, 10 * SPF))
    fut = lis.end()
    bat.run_until_idle()
    _check(fut.result(timeout=0), 1, 10 * SPF)
    assert not _marks(eng, "frame", "admit")
    bat.close()


def test_a_listen_round_rides_beside_a_generating_request():
    eng = Engine()
    bat = _listen_batcher(eng, max_batch=1)
    req = _req(bat, 4, 4)
    lis = bat.listen()
    lis.feed(_clip(1, 9 * SPF))
    fut = lis.end()
    bat.run_until_idle()
    assert req.result(timeout=0).codes.T.tolist() == [[4, i + 1] for i in range(4)]
    _check(fut.result(timeout=0), 1, 9 * SPF)
    kinds = [c[0] for c in eng.calls if c[0] in ("encode_step", "frame")]
    assert kinds[:4] == ["encode_step", "frame", "encode_step", "frame"]  # one full round per frame step
    bat.close()


# ---- the worker thread -------------------------------------------------------------------------------------------------------------------------
def test_feed_and_end_wake_an_idle_worker():
    eng = Engine()
    bat = _listen_batcher(eng).start()
    lis = bat.listen()
    lis.feed(_clip(1, 2 * SPF))  # nothing due: the worker sleeps on
    lis.feed(_clip(1, 4 * SPF)[2 * SPF :])
    assert eng.enc.stepped.wait(timeout=30)  # woken by `feed`
    fut = lis.end()
    _check(fut.result(timeout=30), 1, 4 * SPF)  # woken by `end`: the tail and the result
    assert eng.enc.calls == [(M, (0,)), (1, (0,))]
    bat.close()


# ---- capacity and lifecycle --------------------------------------------------------------------------------------------------------------------
def test_capacity_cancel_feed_limit_and_close():
    eng = Engine()
    bat = _listen_batcher(eng, rows=2)
    a, b = bat.listen(), bat.listen()
    with pytest.raises(ValueError, match="taken"):
        bat.listen()
    a.feed(_clip(1, 4 * SPF))
    bat.step()
    assert a.cancel() and not a.cancel()
    with pytest.raises(ValueError):
        a.feed(_clip(1, SPF))
    c = bat.listen()  # the freed row, reset before its first step
    assert c.row == 0
    c.feed(_clip(3, 11 * SPF))
    with pytest.raises(ValueError, match="listen_max_frames"):
        c.feed(_clip(3, SPF + 1))
    assert c.samples == 11 * SPF and c.frames == 0
    with pytest.raises(ValueError, match="nothing was fed"):
        b.end()
    fc = c.end()
    with pytest.raises(ValueError):
        c.end()
    bat.run_until_idle()
    _check(fc.result(timeout=0), 3, 11 * SPF)
    assert _marks(eng, "enc_reset") == [("enc_reset", 0), ("enc_reset", 0)]
    d = bat.listen()
    d.feed(_clip(4, SPF))
    fd = d.end()
    b.feed(_clip(2, SPF))
    bat.close()
    with pytest.raises(RuntimeError, match="closed"):
        fd.result(timeout=0)
    with pytest.raises(RuntimeError):
        b.feed(_clip(2, SPF))
    with pytest.raises(RuntimeError):
        bat.listen()
    with pytest.raises(ValueError, match="listen_rows"):
        _batcher(Engine()).listen()


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------------
def test_session_busy_rules_and_the_heard_turn_equals_hear():
    eng = Engine()
    bat = _listen_batcher(eng)
    sess = bat.session()
    turn = sess.submit([3, 3, 6], max_audio_length_ms=80 * 3)
    lis = sess.listen(speaker=1)  # allowed while the turn is queued
    n = 4 * SPF + 1
    lis.feed(_clip(1, n)[: 2 * SPF])
    assert bat.step() and sess.busy
    with pytest.raises(ValueError, match="queued or live"):
        lis.end([9, 9])
    lis.feed(_clip(1, n)[2 * SPF :])  # the listener stays usable
    bat.run_until_idle()
    assert turn.done() and not sess.busy and lis.frames == 3
    with pytest.raises(ValueError, match="text"):
        lis.end()
    before = (len(sess.turns), sess.length)
    other = sess.listen(speaker=2)
    other.feed(_clip(2, SPF))
    assert other.cancel() and (len(sess.turns), sess.length) == before and not sess.busy
    fut = lis.end([9, 9])
    assert sess.busy  # from end() to the result
    with pytest.raises(ValueError, match="queued or live"):
        sess.submit([3, 3, 7], max_audio_length_ms=80 * 3)
    with pytest.raises(ValueError, match="queued or live"):
        sess.hear(Segment(1, [9], np.zeros(3, np.float32)), codes=_want(1, 3))
    bat.run_until_idle()
    res = fut.result(timeout=0)
    _check(res, 1, n)
    assert not sess.busy and sess.turns[-1] == (1, [9, 9], 0)
    # the twin: the same first turn, then hear(codes=those codes)
    eng2 = Engine()
    bat2 = _listen_batcher(eng2)
    twin = bat2.session()
    twin.submit([3, 3, 6], max_audio_length_ms=80 * 3)
    bat2.run_until_idle()
    twin.hear(Segment(1, [9, 9], _clip(1, n)), codes=res.codes.numpy())
    assert twin.turns == sess.turns and twin.length == sess.length and twin.n == sess.n
    for x, y in zip(sess.pending + sess.history, twin.pending + twin.history):
        np.testing.assert_array_equal(x, y)
    nxt, nxt2 = sess.submit([3, 8], max_audio_length_ms=80 * 2), twin.submit([3, 8], max_audio_length_ms=80 * 2)
    bat.run_until_idle(); bat2.run_until_idle()
    assert nxt.result(timeout=0).codes.tolist() == nxt2.result(timeout=0).codes.tolist()
    assert _marks(eng, "admit")[-1] == _marks(eng2, "admit")[-1]
    # a cancelled end() leaves the session as it was
    late = sess.listen(1)
    late.feed(_clip(3, SPF))
    f = late.end([9])
    assert sess.busy and late.cancel() and not sess.busy
    with pytest.raises(CancelledError):
        f.result(timeout=0)
    assert sess.turns == twin.turns
    bat.close(); bat2.close()


# ---- listen_rows = 0 ---------------------------------------------------------------------------------------------------------------------------
PLAIN = [("prompts", (1, 2)), ("admit", 0, 1, 0, 3), ("admit", 1, 2, 0, 3), ("frame", (1, 2)), ("frame", (1, 2)), ("park", 1), ("prompts", (4,)),
         ("admit", 1, 4, 0, 3), ("frame", (1, 4)), ("park", 0), ("frame", (None, 4)), ("frame", (None, 4)), ("park", 1)]


def test_without_listen_rows_step_is_what_it_was():
    """The call sequence of a plain workload, as recorded on the commit before listening existed."""
    eng = Engine()
    bat = _batcher(eng)
    assert bat._enc is None and "listen_rounds" not in bat.stats
    futs = [_req(bat, 1, 4), _req(bat, 2, 3), _req(bat, 4, 4)]
    bat.run_until_idle()
    assert [f.result(timeout=0).frames for f in futs] == [4, 3, 4]
    assert eng.calls == PLAIN
    bat.close()
