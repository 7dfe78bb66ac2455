"""Multi-turn sessions (`CSMBatcher.session`, `submit(session=)`) against a scripted engine (no device): what is captured at the end
of a turn and what the next turn's prompt block starts with, for EOS-ended and limit-ended turns at both poll cadences; that `n + S` drives the
length limit, the up-shift and the bare-position move; the refusals; that a failed turn leaves the session as it was; who destroys which
prefix; and that the capture comes before the row is parked.  The engine enforces the library's rules (a capture needs a live row and
n <= the positions it holds; an admission a parked row and n + S <= P), so a scheduling mistake fails loudly here."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd.csm_serve import CSMBatcher  # noqa: E402
from mlx_audio_amd.sesame import Segment, make_sampler  # noqa: E402

N_CB = 2


class ScriptedPrefix:
    """What the scheduler reads of a prefix: its length, its origin, `close`; of a voice prefix also the frames it was made from."""

    def __init__(self, length, root, log, name):
        self.length, self.root, self.log, self.name, self.open = length, root, log, name, True
        self.tokens = np.full((length, N_CB + 1), 9, np.int32)
        self.mask = np.ones((length, N_CB + 1), np.float32)

    def close(self):
        if self.open:
            self.open = False
            self.log.append(("destroy", self.name))


def _text(ids):
    tok = np.zeros((len(ids), N_CB + 1), np.int32)
    msk = np.zeros((len(ids), N_CB + 1), np.float32)
    tok[:, -1], msk[:, -1] = ids, 1
    return tok, msk


def _audio(codes, eos=True):
    codes = np.asarray(codes, np.int32).reshape(-1, N_CB)
    n = codes.shape[0] + (1 if eos else 0)
    tok, msk = np.zeros((n, N_CB + 1), np.int32), np.zeros((n, N_CB + 1), np.float32)
    tok[: codes.shape[0], :N_CB], msk[:, :N_CB] = codes, 1
    return tok, msk


class ScriptedEngine:
    """The stream whose prompt ends with text token `tag` emits frame i = [tag, i + 1]; frame `eos_at[tag]` is all zero (EOS) and the row goes on
    behind it, as a device row does until a poll parks it.  A row's window holds its whole prompt and every frame that was fed."""

    def __init__(self, max_pos=64, eos_at=None, fail_admit=()):
        self.n_cb, self.max_pos, self.sample_rate, self.device = N_CB, max_pos, 24000, torch.device("cpu")
        self.calls, self.eos_at, self.fail_admit, self.captures = [], dict(eos_at or {}), set(fail_admit), 0

    def start(self, max_batch):
        self.max_batch, self.pad, self.P = max_batch, [self.max_pos] * max_batch, 0
        self.tag, self.local = [None] * max_batch, [0] * max_batch

    def voice_prefix(self, length):
        return ScriptedPrefix(length, self, self.calls, "voice")

    def _emit(self, tag, i):
        return [0, 0] if self.eos_at.get(tag) == i else [tag, i + 1]

    # ---- plain requests
    def prompt_length(self, context, text, speaker, voice_match):
        return len(text)

    def prompts(self, streams):
        return [_text(s.text) for s in streams]

    def prefixed_prompt(self, prefix, text, speaker):
        if prefix.root is not self:
            raise ValueError("the voice prefix was made on another engine")
        return _text(text)

    # ---- sessions
    def owns(self, prefix):
        return prefix.root is self

    def segment_frames(self, segment, codes=None):
        t = _text(segment.text)
        if codes is None:
            return t
        a = _audio(np.asarray(codes).T)
        return np.concatenate([t[0], a[0]]), np.concatenate([t[1], a[1]])

    def make_prefix(self, tokens, mask):
        self.calls.append(("make_prefix", int(tokens.shape[0])))
        return ScriptedPrefix(int(tokens.shape[0]), self, self.calls, "rebuilt")

    def session_prompt(self, sess, text, speaker):
        if sess.engine is not self:
            raise ValueError("the session belongs to another engine")
        t = _text(text)
        return np.concatenate([sess.pending[0], t[0]]), np.concatenate([sess.pending[1], t[1]])

    def capture(self, row, n):
        assert self.pad[row] < self.max_pos, "capture of a parked row"
        assert 1 <= n <= self.P - self.pad[row], "capture beyond the row's window"
        self.captures += 1
        self.calls.append(("capture", row, n))
        return ScriptedPrefix(n, self, self.calls, f"cap{self.captures}")

    # ---- the batch
    def row_state(self):
        return list(self.pad), self.P

    def park(self, row):
        self.calls.append(("park", row))
        self.pad[row], self.tag[row] = self.max_pos, None

    def shift(self, delta):
        live = [p for p in self.pad if p < self.max_pos]
        assert 0 <= self.P + delta <= self.max_pos and all(p + delta >= 0 for p in live), "shift out of the cache"
        self.calls.append(("shift", delta, self.P, min(live) if live else None))
        self.pad = [p + delta if p < self.max_pos else p for p in self.pad]
        self.P += delta

    def admit(self, row, prompt, sampler, uniforms, seed, stream_id, prefix=None):
        n = prefix.length if prefix is not None else 0
        S, tag = prompt[0].shape[0], int(prompt[0][-1, -1])
        assert self.pad[row] == self.max_pos, "admission into a live row"
        assert n + S <= self.P, "prefix + suffix longer than the position"
        assert prefix is None or (prefix.root is self and prefix.open), "a foreign or destroyed prefix reached the admission"
        if tag in self.fail_admit:
            raise RuntimeError("scripted admission failure")
        self.calls.append(("admit", row, tag, n, S, self.P, prompt[0].tolist(), prompt[1].tolist()))
        self.pad[row], self.tag[row], self.local[row] = self.P - n - S, tag, 1
        return torch.tensor(self._emit(tag, 0), dtype=torch.int32)

    def frame(self, prev, sampler, uniforms, seed, stream_ids):
        assert self.P < self.max_pos, "frame beyond the cache"
        out = []
        for r in range(self.max_batch):
            if self.tag[r] is None:
                out.append([7, 7])
            else:
                assert prev[r].tolist() == self._emit(self.tag[r], self.local[r] - 1), "a row was not fed its own last frame"
                out.append(self._emit(self.tag[r], self.local[r]))
                self.local[r] += 1
        self.calls.append(("frame", self.P))
        self.P += 1
        return torch.tensor(out, dtype=torch.int32)

    def decode(self, codes):
        return codes.to(torch.float32).sum(dim=1).repeat_interleave(3, dim=1)

    def synchronize(self):
        pass


def _batcher(engine, **kw):
    kw.setdefault("rng", "host")
    kw.setdefault("max_batch", 2)
    return CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=engine, **kw)


def _turn(bat, sess, tag, length, frames):
    fut = bat.submit(session=sess, text=[tag] * length, max_audio_length_ms=80 * frames)
    bat.run_until_idle()
    return fut


def _admits(eng):
    return [c for c in eng.calls if c[0] == "admit"]


def _state(sess):
    return sess.prefix, sess.n, sess.pending[0].tolist(), sess.pending[1].tolist(), list(sess.turns), sess.history[0].tolist()


# ---- the capture arithmetic -------------------------------------------------------------------------------------------------------------------
def _two_turns(interval, eos_at, limit):
    eng = ScriptedEngine(eos_at={1: eos_at} if eos_at is not None else None)
    bat = _batcher(eng, eos_check_interval=interval)
    sess = bat.session()
    r1 = _turn(bat, sess, 1, 4, limit).result(timeout=0)
    ran = max(c[1] for c in eng.calls if c[0] == "frame") + 1 - 4 + 1  # samples of turn 1: one from the admission, one per frame
    _turn(bat, sess, 2, 3, 2).result(timeout=0)
    return eng, sess, r1, ran


@pytest.mark.parametrize("eos_at,limit,kept,n1,carried", [
    (6, 20, 6, 4 + 6, []),          # EOS frame 6: frames 0 .. 5 are kept and were all fed -- the cache holds them, the EOS frame is what is missing
    (3, 20, 3, 4 + 3, []),          # EOS frame 3; at interval 8 the row runs 5 frames past it before the poll
    (None, 6, 6, 4 + 5, [[1, 6]]),  # the limit: the 6th kept frame was sampled but never fed
])
def test_capture_and_next_suffix_do_not_depend_on_the_poll_cadence(eos_at, limit, kept, n1, carried):
    runs = [_two_turns(interval, eos_at, limit) for interval in (1, 8)]
    for eng, sess, r1, ran in runs:
        assert r1.frames == kept
        caps = [c for c in eng.calls if c[0] == "capture"]
        assert caps[0] == ("capture", 0, n1)
        a = _admits(eng)[1]
        assert a[3] == n1 and a[4] == len(carried) + 1 + 3  # on top of the capture: what the cache lacked, the EOS frame, the text
        want = _audio(carried)  # (with the EOS frame)
        t = _text([2, 2, 2])
        assert a[6] == np.concatenate([want[0], t[0]]).tolist() and a[7] == np.concatenate([want[1], t[1]]).tolist()
        assert sess.turns == [(0, [1] * 4, kept), (0, [2] * 3, 2)]
        assert sess.n + sess.pending[0].shape[0] == sess.history[0].shape[0] == 4 + kept + 1 + 3 + 2 + 1
    assert runs[0][3] < runs[1][3] or eos_at is None  # the cadences differ in how far the row ran (the overrun case: 4 against 9 samples)
    if eos_at == 3:
        assert (runs[0][3], runs[1][3]) == (4, 9)
    assert _admits(runs[0][0])[1][6:] == _admits(runs[1][0])[1][6:]
    assert runs[0][1].history[0].tolist() == runs[1][1].history[0].tolist()


def test_history_is_the_prompt_a_plain_request_would_send():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session()
    _turn(bat, sess, 1, 2, 3)
    want = [_text([1, 1]), _audio([[1, 1], [1, 2], [1, 3]])]
    assert sess.history[0].tolist() == np.concatenate([w[0] for w in want]).tolist()
    assert sess.history[1].tolist() == np.concatenate([w[1] for w in want]).tolist()
    assert sess.n == 2 + 2 and sess.pending[0].tolist() == [[1, 3, 0], [0, 0, 0]] and sess.pending[1].tolist() == [[1, 1, 0], [1, 1, 0]]


def test_heard_turns_land_in_the_suffix_in_order():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session()
    _turn(bat, sess, 1, 2, 3)
    before = [c for c in eng.calls]
    sess.hear(Segment(speaker=1, text=[5, 5]), codes=np.array([[3, 4], [3, 4]]))  # two audio frames [3, 3], [4, 4]
    sess.hear(Segment(speaker=2, text=[6]))
    assert eng.calls == before  # nothing ran
    assert sess.turns[1:] == [(1, [5, 5], 0), (2, [6], 0)]
    _turn(bat, sess, 2, 1, 2)
    a = _admits(eng)[1]
    parts = [_audio([[1, 3]]), _text([5, 5]), _audio([[3, 3], [4, 4]]), _text([6]), _text([2])]
    assert a[3] == 4 and a[6] == np.concatenate([p[0] for p in parts]).tolist() and a[7] == np.concatenate([p[1] for p in parts]).tolist()
    assert [t[0] for t in sess.turns] == [0, 1, 2, 0] and sess.history[0].shape[0] == sess.n + sess.pending[0].shape[0]


def test_context_segments_are_heard_before_the_first_turn():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session(context=[Segment(speaker=1, text=[5, 5, 5])], speaker=3)
    assert sess.prefix is None and sess.n == 0 and sess.pending[0].shape[0] == 3
    fut = sess.submit([1, 1], max_audio_length_ms=160)
    bat.run_until_idle()
    a = _admits(eng)[0]
    assert a[3] == 0 and a[4] == 5 and fut.result(timeout=0).frames == 2 and sess.turns[-1][0] == 3  # no prefix: the plain admission
    assert bat.stats["session_admissions"] == 1 and bat.stats["prefixed_admissions"] == 0 and bat.stats["captures"] == 1


# ---- n + S drives the lengths -----------------------------------------------------------------------------------------------------------------
def test_the_limit_and_the_bare_position_move_count_prefix_and_suffix():
    eng = ScriptedEngine(max_pos=64)
    bat = _batcher(eng)
    vp = eng.voice_prefix(30)
    sess = bat.session(context=vp)
    assert sess.prefix is vp and sess.n == 30 and sess.history[0].shape[0] == 30
    with pytest.raises(ValueError, match="Inputs too long.*rebuild"):
        bat.submit(session=sess, text=[1] * 14, max_audio_length_ms=80 * 20)  # 30 + 14 + 20 >= 64
    assert not sess.busy
    fut = bat.submit(session=sess, text=[1] * 13, max_audio_length_ms=80 * 20)  # 63 < 64
    bat.run_until_idle()
    assert fut.result(timeout=0).frames == 20
    assert eng.calls[0] == ("shift", 43, 0, None) and eng.calls[1][:6] == ("admit", 0, 1, 30, 13, 43)
    assert sess.n == 43 + 19 and bat.stats["session_admissions"] == bat.stats["prefixed_admissions"] == 1


def test_up_shift_by_exactly_the_missing_slots_of_prefix_plus_suffix():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session()
    _turn(bat, sess, 1, 3, 6)  # n = 3 + 5, pending: the 6th frame and EOS
    assert (sess.n, sess.pending[0].shape[0]) == (8, 2)
    other = bat.submit(None, [4] * 3, max_audio_length_ms=80 * 30)
    bat.step(); bat.step()
    P = eng.row_state()[1]
    assert P == 5
    fut = bat.submit(session=sess, text=[2] * 4, max_audio_length_ms=80 * 3)  # 8 + 2 + 4 = 14 > 5
    bat.step()
    assert [c for c in eng.calls if c[0] == "shift"][-1][:3] == ("shift", 14 - 5, 5)
    assert _admits(eng)[-1][1:6] == (1, 2, 8, 6, 14)
    bat.run_until_idle()
    assert fut.result(timeout=0).frames == 3 and other.result(timeout=0).frames == 30


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_a_second_turn_while_one_is_queued_or_live_is_refused():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session()
    fut = bat.submit(session=sess, text=[1, 1], max_audio_length_ms=80 * 5)
    with pytest.raises(ValueError, match="queued or live"):
        bat.submit(session=sess, text=[2], max_audio_length_ms=80)
    bat.step(); bat.step()
    with pytest.raises(ValueError, match="queued or live"):
        bat.submit(session=sess, text=[2], max_audio_length_ms=80)
    with pytest.raises(ValueError, match="queued or live"):
        sess.hear(Segment(speaker=1, text=[3]))
    bat.run_until_idle()
    assert fut.result(timeout=0).frames == 5 and len(_admits(eng)) == 1
    assert _turn(bat, sess, 2, 1, 2).result(timeout=0).frames == 2


def test_a_closed_session_is_refused():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session()
    _turn(bat, sess, 1, 2, 2)
    sess.close()
    with pytest.raises(ValueError, match="closed"):
        bat.submit(session=sess, text=[2], max_audio_length_ms=80)
    assert not bat._queue


def test_a_session_of_another_engine_is_refused_at_submit():
    eng, other = ScriptedEngine(), ScriptedEngine()
    bat, bat2 = _batcher(eng), _batcher(other)
    sess = bat2.session()
    with pytest.raises(ValueError):
        bat.submit(session=sess, text=[1], max_audio_length_ms=80)
    with pytest.raises(ValueError):
        bat.session(context=other.voice_prefix(4))
    assert not bat._queue and eng.calls == [] and not sess.busy


@pytest.mark.parametrize("extra", [dict(context=["a segment"]), dict(prompt=(np.zeros((2, 3), np.int32), np.ones((2, 3), np.float32))),
                                   dict(prefix="vp"), dict(voice_match=True)])
def test_session_excludes_context_prompt_prefix_and_voice_match(extra):
    eng = ScriptedEngine()
    bat = _batcher(eng)
    sess = bat.session()
    if "prefix" in extra:
        extra = dict(prefix=eng.voice_prefix(4))
    with pytest.raises(ValueError, match="excludes"):
        bat.submit(session=sess, text=[1, 1], max_audio_length_ms=800, **extra)
    assert not bat._queue and not sess.busy and eng.calls == []


def test_a_history_that_outgrew_the_cache_points_to_rebuild_and_rebuild_helps():
    eng = ScriptedEngine(max_pos=40)
    bat = _batcher(eng)
    sess = bat.session(context=eng.voice_prefix(5))
    for tag in (1, 2):
        _turn(bat, sess, tag, 2, 8)  # 5 | 2 + 8 + EOS | 2 + 8 + EOS = 27
    assert sess.length == 27 and [c[1] for c in eng.calls if c[0] == "destroy"] == ["cap1"]
    with pytest.raises(ValueError, match="Inputs too long.*rebuild"):
        bat.submit(session=sess, text=[3, 3], max_audio_length_ms=80 * 11)  # 27 + 2 + 11 = 40
    full = sess.history[0].copy()
    sess.rebuild(keep_last_turns=1)
    assert eng.calls[-2:] == [("make_prefix", 16), ("destroy", "cap2")]
    assert sess.n == 16 and sess.pending[0].shape[0] == 0 and sess.turns == [(0, [2, 2], 8)]
    assert sess.history[0].tolist() == np.concatenate([full[:5], full[16:]]).tolist()
    assert _turn(bat, sess, 3, 2, 11).result(timeout=0).frames == 11
    assert _admits(eng)[-1][3:5] == (16, 2)
    sess.rebuild()  # the whole history
    assert eng.calls[-2][0] == "make_prefix" and eng.calls[-2][1] == sess.n == 16 + 2 + 11 + 1


# ---- a failed turn ------------------------------------------------------------------------------------------------------------------------------
def test_a_turn_that_fails_at_admission_leaves_the_session_as_it_was():
    eng = ScriptedEngine(fail_admit={2})
    bat = _batcher(eng)
    sess = bat.session()
    _turn(bat, sess, 1, 2, 3)
    sess.hear(Segment(speaker=1, text=[5]))
    before = _state(sess)
    fut = _turn(bat, sess, 2, 2, 3)
    assert isinstance(fut.exception(timeout=0), RuntimeError)
    assert _state(sess) == before and sess.prefix.open and not sess.busy
    assert _turn(bat, sess, 3, 2, 3).result(timeout=0).frames == 3  # and the next turn runs on that state
    assert _admits(eng)[-1][3] == before[1]


def test_a_turn_without_audio_leaves_the_session_as_it_was():
    eng = ScriptedEngine(eos_at={2: 0})
    bat = _batcher(eng)
    sess = bat.session()
    _turn(bat, sess, 1, 2, 3)
    before = _state(sess)
    fut = _turn(bat, sess, 2, 2, 3)
    assert isinstance(fut.exception(timeout=0), AssertionError) and _state(sess) == before and sess.prefix.open
    assert len([c for c in eng.calls if c[0] == "capture"]) == 1


# ---- who destroys what --------------------------------------------------------------------------------------------------------------------------
def test_the_sessions_own_prefixes_are_destroyed_on_replace_and_close_a_callers_never():
    eng = ScriptedEngine()
    bat = _batcher(eng)
    vp = eng.voice_prefix(6)
    sess = bat.session(context=vp)
    destroyed = lambda: [c[1] for c in eng.calls if c[0] == "destroy"]
    _turn(bat, sess, 1, 2, 3)
    assert destroyed() == [] and vp.open and sess.prefix.name == "cap1"  # the caller's prefix was replaced, not destroyed
    _turn(bat, sess, 2, 2, 3)
    assert destroyed() == ["cap1"] and sess.prefix.name == "cap2"
    sess.close()
    assert destroyed() == ["cap1", "cap2"] and vp.open and sess.prefix is None
    sess2 = bat.session(context=vp)
    sess2.close()
    assert destroyed() == ["cap1", "cap2"] and vp.open


# ---- order --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streaming", [False, True])
def test_capture_comes_before_park(streaming):
    eng = ScriptedEngine(eos_at={1: 5})

    class Dec:  # the row decoder's surface, for the streaming path
        def reset_row(self, row): pass
        def step(self, codes, active): return codes.to(torch.float32).sum(dim=1, keepdim=True).repeat_interleave(3, dim=2)
        def close(self): pass

    eng.row_decoder = lambda *a: Dec()
    bat = _batcher(eng, stream_chunk_frames=2) if streaming else _batcher(eng, eos_check_interval=2)
    sess = bat.session()
    got = (bat.submit_stream if streaming else bat.submit)(session=sess, text=[1, 1, 1], max_audio_length_ms=80 * 20)
    bat.run_until_idle()
    assert got.result(timeout=0).frames == 5
    names = [c[0] for c in eng.calls]
    i = names.index("capture")
    assert eng.calls[i] == ("capture", 0, 3 + 5) and names[i + 1] == "park" and eng.calls[i + 1] == ("park", 0)
    assert "park" not in names[:i] and sess.n == 8 and sess.pending[0].tolist() == [[0, 0, 0]]
