"""Stopping a request (`CSMBatcher.cancel` / `interrupt`, a plain `future.cancel()`) against a scripted engine (no device): where a
cancelled request leaves the scheduler and who gets its row, that a future cancelled at any stage never raises out of `step()`, how many frames an
interrupt keeps and what a plain request, a streaming request and a session's turn get back, what happens to a request held in a prefill lane,
and the worker thread.  The engine enforces the library's rules (an admission needs a parked row and a prompt that fits below the position, a
capture a live row that holds the positions, a row is fed its own last frame, the row decoder a row's own next frames from frame 0 after a
reset), so a scheduling mistake fails loudly here."""
import os
import sys
import threading
from concurrent.futures import CancelledError

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd.csm_serve import CSMBatcher  # noqa: E402
from mlx_audio_amd.sesame import make_sampler  # noqa: E402

N_CB, SPF = 2, 3


def _text(ids):
    tok = np.zeros((len(ids), N_CB + 1), np.int32)
    msk = np.zeros((len(ids), N_CB + 1), np.float32)
    tok[:, -1], msk[:, -1] = ids, 1
    return tok, msk


class Prefix:
    def __init__(self, length, root, log, name):
        self.length, self.root, self.log, self.name, self.open = length, root, log, name, True

    def close(self):
        if self.open:
            self.open = False
            self.log.append(("destroy", self.name))


class Decoder:
    """The row decoder's surface: pcm of a frame = the sum of its codes, SPF samples per frame (what `Engine.decode` gives offline)."""

    def __init__(self, engine, max_batch):
        self.engine, self.frames = engine, [0] * max_batch

    def reset_row(self, row):
        self.frames[row] = 0

    def step(self, codes, active):
        F = codes.shape[2]
        for r, on in enumerate(active):
            if on:
                tag = int(codes[r, 0, 0])
                assert tag != 0, "an EOS frame was handed to the codec"
                assert codes[r, 1].tolist() == list(range(self.frames[r] + 1, self.frames[r] + F + 1)), "a row was not fed its own next frames"
                self.engine.calls.append(("decode_step", tag, self.frames[r], F))
                self.frames[r] += F
        return codes.to(torch.float32).sum(dim=1).repeat_interleave(SPF, dim=1)[:, None, :]

    def close(self):
        pass


class Engine:
    """The stream whose prompt ends with text token `tag` emits frame i = [tag, i + 1]; frame `eos_at[tag]` is all zero (EOS) and the row goes on
    behind it.  `calls` logs what the scheduler did, in order.  busy: tags whose lane answers "not ready"; fail_prompts: tags whose `prompts`
    raises; hooks: name -> callable, run inside `prompts` / `decode` (a caller that acts between two of the scheduler's checks); gate: a
    semaphore every frame step takes one permit of (the worker thread runs only as far as the test lets it)."""

    def __init__(self, max_pos=64, eos_at=None, busy=(), fail_prompts=(), gate=None):
        self.n_cb, self.max_pos, self.sample_rate, self.device, self.samples_per_frame = N_CB, max_pos, 24000, torch.device("cpu"), SPF
        self.calls, self.eos_at, self.busy, self.fail_prompts, self.gate = [], dict(eos_at or {}), set(busy), set(fail_prompts), gate
        self.hooks, self.captures, self.lanes = {}, 0, None

    def start(self, max_batch):
        self.max_batch, self.pad, self.P = max_batch, [self.max_pos] * max_batch, 0
        self.tag, self.local = [None] * max_batch, [0] * max_batch

    def _emit(self, tag, i):
        return [0, 0] if self.eos_at.get(tag) == i else [tag, i + 1]

    def prompt_length(self, context, text, speaker, voice_match):
        return len(text)

    def prompts(self, streams):
        tags = [int(s.text[-1]) for s in streams]
        self.calls.append(("prompts", tuple(tags)))
        if "prompts" in self.hooks:
            self.hooks["prompts"]()
        if self.fail_prompts & set(tags):
            raise RuntimeError("scripted prompt failure")
        return [_text(s.text) for s in streams]

    # ---- sessions
    def owns(self, prefix):
        return prefix.root is self

    def session_prompt(self, sess, text, speaker):
        t = _text(text)
        return np.concatenate([sess.pending[0], t[0]]), np.concatenate([sess.pending[1], t[1]])

    def capture(self, row, n):
        assert self.pad[row] < self.max_pos, "capture of a parked row"
        assert 1 <= n <= self.P - self.pad[row], "capture beyond the row's window"
        self.captures += 1
        self.calls.append(("capture", row, n))
        return Prefix(n, self, self.calls, f"cap{self.captures}")

    # ---- the batch
    def row_state(self):
        return list(self.pad), self.P

    def park(self, row):
        self.calls.append(("park", row))
        self.pad[row], self.tag[row] = self.max_pos, None

    def shift(self, delta):
        live = [p for p in self.pad if p < self.max_pos]
        assert 0 <= self.P + delta <= self.max_pos and all(p + delta >= 0 for p in live), "shift out of the cache"
        self.pad = [p + delta if p < self.max_pos else p for p in self.pad]
        self.P += delta

    def _enter(self, row, tag, L):
        assert self.pad[row] == self.max_pos, "admission into a live row"
        assert L <= self.P, "the admission is longer than the position"
        self.pad[row], self.tag[row], self.local[row] = self.P - L, tag, 1
        return torch.tensor(self._emit(tag, 0), dtype=torch.int32)

    def admit(self, row, prompt, sampler, uniforms, seed, stream_id, prefix=None):
        n, S, tag = (prefix.length if prefix is not None else 0), prompt[0].shape[0], int(prompt[0][-1, -1])
        assert prefix is None or (prefix.root is self and prefix.open), "a foreign or destroyed prefix reached the admission"
        self.calls.append(("admit", row, tag, n, S))
        return self._enter(row, tag, n + S)

    def frame(self, prev, sampler, uniforms, seed, stream_ids, device_rng=False):
        if self.gate is not None:
            assert self.gate.acquire(timeout=30), "the test never let this frame run"
        assert self.P < self.max_pos, "frame beyond the cache"
        out = []
        for r in range(self.max_batch):
            if self.tag[r] is None:
                out.append([7, 7])
            else:
                assert prev[r].tolist() == self._emit(self.tag[r], self.local[r] - 1), "a row was not fed its own last frame"
                out.append(self._emit(self.tag[r], self.local[r]))
                self.local[r] += 1
        self.calls.append(("frame", tuple(self.tag)))
        self.P += 1
        return torch.tensor(out, dtype=torch.int32)

    def decode(self, codes):
        if "decode" in self.hooks:
            self.hooks["decode"]()
        return codes.to(torch.float32).sum(dim=1).repeat_interleave(SPF, dim=1)

    def row_decoder(self, max_batch, max_frames, max_chunk):
        return Decoder(self, max_batch)

    def synchronize(self):
        pass

    # ---- the lanes: a prefill starts from a reset, so a lane whose request was dropped is simply used again
    def open_lanes(self, n):
        self.lanes = [None] * n

    def prefill(self, lane, prompt, sampler, uniforms, seed, stream_id, prefix=None, timed=False):
        tag = int(prompt[0][-1, -1])
        self.calls.append(("prefill", lane, tag))
        self.lanes[lane] = h = {"tag": tag, "L": prompt[0].shape[0] + (prefix.length if prefix is not None else 0)}
        return h

    def prefill_ready(self, handle, wait=False):
        if wait:
            assert not any(t is not None for t in self.tag), "the scheduler waited for a lane while rows were live"
            self.busy.discard(handle["tag"])
            return True
        return handle["tag"] not in self.busy

    def commit(self, row, lane, handle):
        assert self.lanes[lane] is handle, "the lane does not hold this request"
        assert handle["tag"] not in self.busy, "a commit before the lane was ready"
        self.calls.append(("commit", row, handle["tag"], lane))
        self.lanes[lane] = None
        return self._enter(row, handle["tag"], handle["L"])

    def close_lanes(self):
        pass


def _batcher(eng, **kw):
    kw.setdefault("max_batch", 2)
    kw.setdefault("eos_check_interval", 8)
    return CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=eng, rng="host", **kw)


def _req(bat, tag, frames, length=3, stream=False):
    return (bat.submit_stream if stream else bat.submit)(None, [3] * (length - 1) + [tag], max_audio_length_ms=80 * frames, voice_match=False)


def _own(tag, frames):
    return [[tag, i + 1] for i in range(frames)]


def _codes(fut):
    return fut.result(timeout=0).codes.T.tolist()


def _marks(eng, *kinds):
    return [c for c in eng.calls if c[0] in kinds]


def _cancelled(fut):
    with pytest.raises(CancelledError):
        fut.result(timeout=0)
    return fut.cancelled()


# ---- cancel ------------------------------------------------------------------------------------------------------------------------------------
def test_cancel_of_a_queued_request_it_is_never_admitted_and_the_others_keep_their_order():
    eng = Engine()
    bat = _batcher(eng, max_batch=1)
    a, b, c, d = (_req(bat, tag, 3) for tag in (1, 2, 4, 5))
    assert bat.step()
    assert bat.cancel(c) and not c.done()  # the caller's thread has only recorded the wish
    assert bat.step() and _cancelled(c)
    bat.run_until_idle()
    assert [x[2] for x in _marks(eng, "admit")] == [1, 2, 5]
    assert all(4 not in x[1] for x in _marks(eng, "prompts"))  # no prompt was built for it
    assert [_codes(f) for f in (a, b, d)] == [_own(1, 3), _own(2, 3), _own(5, 3)]
    assert bat.stats["cancelled"] == 1 and bat.stats["finished"] == 3 and bat.stats["admissions"] == 3
    assert bat.cancel(a) is False and bat.cancel(c) is False and bat.interrupt(a) is False  # finished: no effect
    assert not bat._controls


def _run_with_and_without(cancel_first):
    eng = Engine()
    bat = _batcher(eng, max_batch=2)
    a = _req(bat, 1, 12) if cancel_first else None
    b, c = _req(bat, 2, 12), _req(bat, 4, 6, length=5)
    return eng, bat, a, b, c


def test_cancel_of_a_live_request_parks_its_row_and_the_next_request_takes_it_in_the_same_round():
    eng, bat, a, b, c = _run_with_and_without(True)
    for _ in range(3):
        assert bat.step()
    assert bat.cancel(a)
    before = len(eng.calls)
    assert bat.step()
    assert eng.calls[before:] == [("park", 0), ("prompts", (4,)), ("admit", 0, 4, 0, 5), ("frame", (4, 2))]
    assert _cancelled(a) and bat.stats["cancelled"] == 1 and not _marks(eng, "capture")
    bat.run_until_idle()
    _, ref, _, rb, rc = _run_with_and_without(False)
    ref.run_until_idle()
    assert _codes(b) == _codes(rb) == _own(2, 12) and _codes(c) == _codes(rc) == _own(4, 6)
    assert torch.equal(b.result(timeout=0).audio, rb.result(timeout=0).audio)
    assert bat._live() == [] and bat.stats["finished"] == 2


@pytest.mark.parametrize("stage", ["queued", "live", "prompts_raises", "lane", "decoding"])
def test_a_plain_future_cancel_at_every_stage_never_raises_out_of_step_and_the_others_finish(stage):
    """`future.cancel()` by the caller, not through the batcher.  Without the feature the scheduler's unguarded `set_exception` raises
    InvalidStateError out of `step()` (prompts_raises, lane) or the row stays live to its limit (queued: admitted anyway; live)."""
    lanes = stage == "lane"
    eng = Engine(busy={2} if lanes else (), fail_prompts={2} if stage == "prompts_raises" else ())
    bat = _batcher(eng, max_batch=2 if stage in ("live", "decoding") else 1, eos_check_interval=1, **(dict(overlap_admission=True) if lanes else {}))
    other = _req(bat, 1, 9)
    assert bat.step()
    victim = _req(bat, 2, 30 if stage != "decoding" else 4)
    if stage == "queued":
        assert victim.cancel()
    elif stage == "live":
        assert bat.step() and bat._rows[1] is not None
        assert victim.cancel()
        assert bat.step() and bat._rows[1] is None and eng.calls[-2] == ("park", 1)  # dropped at the top of the round
    elif stage == "prompts_raises":  # cancelled while its prompt is being built, which then fails: between two of the scheduler's checks
        eng.hooks["prompts"] = lambda: victim.cancel()
    elif stage == "lane":
        assert bat.step() and [s.stream_id for s in bat._inflight] == [1]
        assert victim.cancel()
        assert bat.step() and not bat._inflight and bat._lane_of == [None]
    else:  # cancelled while its frames are in the codec: between the poll's check and the result
        eng.hooks["decode"] = lambda: victim.cancel()
    last = _req(bat, 4, 3)
    bat.run_until_idle()
    assert _cancelled(victim) and _codes(other) == _own(1, 9) and _codes(last) == _own(4, 3)
    assert bat._live() == [] and not bat._queue and not bat._inflight
    if stage not in ("live", "decoding"):
        assert all(c[2] != 2 for c in _marks(eng, "admit", "commit"))  # it never had a row
    if stage == "queued":
        assert all(2 not in c[1] for c in _marks(eng, "prompts"))
    assert bat.stats["cancelled"] == (0 if stage in ("prompts_raises", "decoding") else 1)  # (those two had left the scheduler by themselves)


def test_a_cancelled_streaming_request_ends_its_iterator_with_cancelled_error():
    eng = Engine()
    bat = _batcher(eng, stream_chunk_frames=3)
    st, other = _req(bat, 1, 30, stream=True), _req(bat, 2, 8, stream=True)
    for _ in range(5):
        assert bat.step()
    assert st.cancel()
    bat.run_until_idle()
    got = []
    with pytest.raises(CancelledError):  # iterated later: the chunk it had, then the error, no hanging
        for ch in st:
            got.append((ch.first_frame, ch.frames, ch.final))
    assert got == [(0, 3, False)] and _cancelled(st.future)
    assert [(ch.first_frame, ch.frames, ch.final) for ch in other] == [(0, 3, False), (3, 3, False), (6, 2, True)]


# ---- interrupt: a plain request ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,eos,kept", [
    (dict(played_frames=4), None, 4),
    (dict(played_frames=50), None, 7),       # clamped to what was generated
    (dict(), None, 7),                       # neither: the frames generated so far
    (dict(played_frames=5), 3, 3),           # the EOS frame came before k: its index wins
    (dict(played_frames=2), 3, 2),
    (dict(played_samples=1), None, 1),       # a partly played frame counts as heard
    (dict(played_samples=2 * SPF), None, 2),
    (dict(played_samples=2 * SPF + 1), None, 3),
])
def test_interrupt_of_a_plain_request_keeps_min_of_heard_generated_eos_and_limit(kw, eos, kept):
    eng = Engine(eos_at={1: eos} if eos is not None else None)
    bat = _batcher(eng)
    a, b = _req(bat, 1, 40), _req(bat, 2, 12)
    for _ in range(6):
        assert bat.step()
    assert len(bat._rows[0].codes) == 7 and bat.stats["polls"] == 0
    assert bat.interrupt(a, **kw) and not a.done()
    before = len(eng.calls)
    assert bat.step()
    assert eng.calls[before:] == [("park", 0), ("frame", (None, 2))]  # one poll now: the row is free before this round's frame
    res = a.result(timeout=0)
    assert res.frames == kept and res.codes.T.tolist() == _own(1, kept) and res.interrupted is True
    assert res.audio.shape == (kept * SPF,) and torch.equal(res.audio, torch.tensor([float(1 + i + 1) for i in range(kept)]).repeat_interleave(SPF))
    assert bat.stats["interrupted"] == 1 and bat.stats["finished"] == 1 and bat.stats["cancelled"] == 0 and bat.stats["polls"] == 1
    assert bat.interrupt(a, played_frames=1) is False
    bat.run_until_idle()
    rb = b.result(timeout=0)
    assert _codes(b) == _own(2, 12) and rb.interrupted is False


def test_interrupt_refuses_both_counts_and_negative_ones():
    eng = Engine()
    bat = _batcher(eng)
    a = _req(bat, 1, 40)
    assert bat.step()
    with pytest.raises(ValueError, match="not both"):
        bat.interrupt(a, played_frames=2, played_samples=5)
    with pytest.raises(ValueError):
        bat.interrupt(a, played_frames=-1)
    assert not bat._controls and bat.step() and not a.done()


def test_interrupt_before_anything_was_heard_and_of_a_queued_request_is_a_cancel():
    eng = Engine()
    bat = _batcher(eng, max_batch=1)
    a, b = _req(bat, 1, 40), _req(bat, 2, 40)
    assert bat.step()
    assert bat.interrupt(a, played_frames=0) and bat.interrupt(b, played_frames=3)
    assert not bat.step()  # a's row is parked, b never enters it: nothing is left
    assert _cancelled(a) and _cancelled(b) and bat.stats["cancelled"] == 2 and bat.stats["interrupted"] == 0
    assert _marks(eng, "park") == [("park", 0)] and len(_marks(eng, "admit")) == 1


# ---- interrupt: a streaming request ----------------------------------------------------------------------------------------------------------------
def _seven_generated_six_emitted():
    """Chunks of 3 frames.  Six rounds leave the stream with 7 frames, of which the poll of round 4 confirmed 4: chunk 0 is out.  The poll that is
    due now (called here, ahead of the next round's frame) confirms 7: chunk 1 is out and frame 6 is held back -- it may be the last."""
    eng = Engine()
    bat = _batcher(eng, stream_chunk_frames=3)
    st, other = _req(bat, 1, 40, stream=True), _req(bat, 2, 11, stream=True)
    for _ in range(6):
        assert bat.step()
    bat._poll()
    s = bat._rows[0]
    assert (len(s.codes), s.emitted, s.confirmed) == (7, 6, 7)
    return eng, bat, st, other


@pytest.mark.parametrize("played,kept,tail", [
    (4, 4, [(4, 0, True)]),      # it has had more than was heard: nothing more, the iterator ends behind an empty chunk
    (None, 6, [(6, 0, True)]),   # neither count: what was emitted
    (6, 6, [(6, 0, True)]),
    (7, 7, [(6, 1, True)]),      # one more frame was heard than it has had: a last chunk of 1 frame
    (9, 7, [(6, 1, True)]),      # clamped to the 7 frames generated when the interrupt is applied
])
def test_interrupt_of_a_streaming_request(played, kept, tail):
    eng, bat, st, other = _seven_generated_six_emitted()
    assert st.interrupt(played_frames=played)
    before = len(eng.calls)
    assert bat.step()
    chunks = list(st)  # returns: the last item is final
    assert [(c.first_frame, c.frames, c.final) for c in chunks] == [(0, 3, False), (3, 3, False)] + tail
    res = st.result(timeout=0)
    whole = torch.tensor([float(1 + i + 1) for i in range(7)]).repeat_interleave(SPF)
    assert res.frames == kept and res.interrupted and res.codes.T.tolist() == _own(1, kept)
    assert res.audio.shape == (kept * SPF,) and torch.equal(res.audio, whole[: kept * SPF])
    assert chunks[-1].audio.shape == (tail[0][1] * SPF,)
    after = [c for c in eng.calls[before:] if c[0] == "decode_step" and c[1] == 1]
    assert after == ([("decode_step", 1, 6, 1)] if tail[0][1] else [])  # the codec ran only for frames that were heard and not had
    assert eng.calls[before:][-1] == ("frame", (None, 2)) and ("park", 0) in eng.calls[before:]
    assert bat.stats["interrupted"] == 1
    bat.run_until_idle()
    assert [(c.first_frame, c.frames, c.final) for c in other] == [(0, 3, False), (3, 3, False), (6, 3, False), (9, 2, True)]
    assert _codes(other.future) == _own(2, 11)


@pytest.mark.parametrize("eos,kept,chunks", [
    (5, 4, [(0, 3, False), (3, 1, True)]),  # 4 frames exist, none is the EOS frame yet: clamped to them
    (2, 2, [(0, 2, True)]),                 # the EOS frame is among them, below k: its index wins, nothing at or behind it reaches the codec
])
def test_interrupt_of_a_streaming_request_that_has_had_nothing_yet(eos, kept, chunks):
    eng = Engine(eos_at={1: eos})
    bat = _batcher(eng, stream_chunk_frames=3)
    st = _req(bat, 1, 40, stream=True)
    for _ in range(3):
        assert bat.step()
    assert len(bat._rows[0].codes) == 4 and bat._rows[0].emitted == 0
    assert st.interrupt(played_frames=9)
    assert bat.step() is False  # the only stream ended in this round's poll
    res, got = st.result(timeout=0), list(st)
    assert res.frames == kept and [(c.first_frame, c.frames, c.final) for c in got] == chunks
    assert torch.equal(res.audio, torch.cat([c.audio for c in got])) and res.audio.shape == (kept * SPF,)
    assert sum(c[3] for c in _marks(eng, "decode_step")) == kept


def test_an_interrupted_streams_last_chunk_goes_through_its_whole_step_and_is_cut_to_what_was_heard():
    """7 frames exist, 3 were emitted, 4 were heard: frames 3 .. 5 go through one step of 3 -- the step that chunk has in the uninterrupted
    stream -- and the chunk carries the first of them."""
    eng = Engine()
    bat = _batcher(eng, stream_chunk_frames=3)
    st = _req(bat, 1, 40, stream=True)
    for _ in range(6):
        assert bat.step()
    assert (len(bat._rows[0].codes), bat._rows[0].emitted) == (7, 3)
    assert st.interrupt(played_samples=3 * SPF + 1)
    assert bat.step() is False
    got = list(st)
    assert [(c.first_frame, c.frames, c.final) for c in got] == [(0, 3, False), (3, 1, True)]
    assert _marks(eng, "decode_step") == [("decode_step", 1, 0, 3), ("decode_step", 1, 3, 3)]
    res = st.result(timeout=0)
    assert res.frames == 4 and torch.equal(res.audio, torch.tensor([2.0, 3.0, 4.0, 5.0]).repeat_interleave(SPF)) and torch.equal(got[1].audio, res.audio[3 * SPF:])


# ---- sessions ----------------------------------------------------------------------------------------------------------------------------------------
def _state(sess):
    return sess.prefix, sess.n, sess.pending[0].tolist(), sess.pending[1].tolist(), sess.history[0].tolist(), sess.history[1].tolist(), list(sess.turns)


def _session_with_a_turn(steps, **kw):
    eng = Engine()
    bat = _batcher(eng, **kw)
    sess = bat.session()
    first = sess.submit([3, 3, 1], max_audio_length_ms=80 * 2)
    bat.run_until_idle()
    assert first.result(timeout=0).frames == 2 and (sess.n, sess.pending[0].shape[0]) == (3 + 1, 2)
    fut = sess.submit([3, 2], max_audio_length_ms=80 * 30)  # L = 4 + 2 + 2 = 8
    for _ in range(steps):
        assert bat.step()
    return eng, bat, sess, fut


@pytest.mark.parametrize("generated,k,positions,carried", [
    (8, 5, 8 + 5, []),         # behind the row's progress: the k kept frames were all fed, the EOS frame is what the cache lacks
    (5, 5, 8 + 4, [[2, 5]]),   # exactly k frames exist: the last was sampled and never fed, as at a limit of k
])
def test_an_interrupted_turn_is_committed_as_a_turn_of_k_frames(generated, k, positions, carried):
    eng, bat, sess, fut = _session_with_a_turn(generated - 1)
    assert len(bat._rows[0].codes) == generated and sess.busy
    assert sess.interrupt(played_frames=k)
    before = len(eng.calls)
    assert bat.step() is False  # the only stream ended in this round's poll
    assert eng.calls[before:] == [("capture", 0, positions), ("park", 0), ("destroy", "cap1")]  # capture, then park; the old capture goes at the commit
    res = fut.result(timeout=0)
    assert res.frames == k and res.interrupted and sess.turns[-1] == (0, [3, 2], k) and sess.turns[-1][2] == k and not sess.busy
    assert sess.n == positions and sess.prefix.name == "cap2"
    want = np.zeros((len(carried) + 1, N_CB + 1), np.int32)
    want[: len(carried), :N_CB] = np.asarray(carried, np.int32).reshape(-1, N_CB)
    assert sess.pending[0].tolist() == want.tolist()  # what the cache lacks, then the EOS frame
    assert sess.history[0].shape[0] == sess.n + sess.pending[0].shape[0] == 3 + 2 + 1 + 2 + k + 1  # the turn's text frames stay whole
    nxt = sess.submit([3, 3, 4], max_audio_length_ms=80 * 2)  # and the session takes the next turn, on top of the k frames
    bat.run_until_idle()
    assert nxt.result(timeout=0).frames == 2 and _marks(eng, "admit")[-1] == ("admit", 0, 4, positions, len(carried) + 1 + 3)


@pytest.mark.parametrize("how", ["session", "batcher", "future"])
@pytest.mark.parametrize("steps", [0, 4])
def test_a_cancelled_turn_leaves_the_session_as_it_was(how, steps):
    eng, bat, sess, fut = _session_with_a_turn(0)
    before = _state(sess)
    for _ in range(steps):
        assert bat.step()
    assert {"session": sess.cancel, "batcher": lambda: bat.cancel(fut), "future": fut.cancel}[how]()
    assert sess.busy  # until the scheduler has dropped the turn: its row is live
    with pytest.raises(ValueError, match="queued or live"):
        sess.submit([3, 5], max_audio_length_ms=80)
    assert bat.step() is False
    assert _cancelled(fut) and not sess.busy and _state(sess) == before and sess.prefix.open
    assert len(_marks(eng, "capture")) == 1 and _marks(eng, "destroy") == []  # the first turn's capture, and it is still the session's
    nxt = sess.submit([3, 5], max_audio_length_ms=80 * 3)
    bat.run_until_idle()
    assert nxt.result(timeout=0).frames == 3 and _marks(eng, "admit")[-1][3] == before[1] and sess.cancel() is False


def test_capture_comes_before_park_for_an_interrupted_streamed_turn():
    eng, bat, sess, _ = _session_with_a_turn(0, stream_chunk_frames=3)
    assert sess.cancel() and bat.step() is False
    st = sess.submit_stream([3, 2], max_audio_length_ms=80 * 30)
    for _ in range(7):
        assert bat.step()
    assert st.interrupt(played_frames=4)
    before = len(eng.calls)
    bat.step()
    names = [c[0] for c in eng.calls[before:]]
    assert names.index("capture") < names.index("park") and eng.calls[before:][names.index("capture")] == ("capture", 0, 8 + 4)
    assert sess.turns[-1][2] == 4 and list(st)[-1].frames == 0


# ---- prefill lanes -----------------------------------------------------------------------------------------------------------------------------------
def test_cancel_of_the_request_in_the_only_lane_frees_it_for_the_next_head_and_the_order_is_kept():
    eng = Engine(busy={2})
    bat = _batcher(eng, max_batch=1, eos_check_interval=1, overlap_admission=True, prefill_lanes=1)
    a, b, c, d = _req(bat, 1, 4), _req(bat, 2, 4), _req(bat, 4, 3), _req(bat, 5, 2)
    assert bat.step()  # A is committed, B has the lane
    assert [s.stream_id for s in bat._inflight] == [1] and len(bat._queue) == 2
    assert bat.cancel(b)
    before = len(eng.calls)
    assert bat.step()
    assert eng.calls[before:] == [("frame", (1,)), ("prompts", (4,)), ("prefill", 0, 4)] and _cancelled(b)
    assert [s.stream_id for s in bat._inflight] == [2] and bat._lane_of[0] is bat._inflight[0]
    bat.run_until_idle()
    assert [c_[2] for c_ in _marks(eng, "commit")] == [1, 4, 5] and [c_[2] for c_ in _marks(eng, "prefill")] == [1, 2, 4, 5]
    assert [_codes(f) for f in (a, c, d)] == [_own(1, 4), _own(4, 3), _own(5, 2)]
    assert bat.stats["cancelled"] == 1 and bat.stats["overlapped_admissions"] == 3
    assert bat.interrupt(c) is False


def test_interrupt_of_a_request_in_a_lane_is_a_cancel():
    eng = Engine(busy={2})
    bat = _batcher(eng, max_batch=1, eos_check_interval=1, overlap_admission=True, prefill_lanes=1)
    a, b = _req(bat, 1, 4), _req(bat, 2, 4)
    assert bat.step() and bat.interrupt(b, played_frames=2)
    bat.run_until_idle()
    assert _cancelled(b) and _codes(a) == _own(1, 4) and [c[2] for c in _marks(eng, "commit")] == [1]


# ---- the worker thread -------------------------------------------------------------------------------------------------------------------------------
def test_a_cancel_from_another_thread_reaches_the_worker_and_a_blocked_iterator_raises():
    gate = threading.Semaphore(0)
    eng = Engine(gate=gate)
    bat = _batcher(eng, max_batch=1, stream_chunk_frames=3).start()
    a, b = _req(bat, 1, 40, stream=True), _req(bat, 2, 3)
    seen = []

    def consume():
        try:
            for ch in a:
                seen.append(ch.first_frame)
        except BaseException as e:  # noqa: BLE001
            seen.append(type(e))

    reader = threading.Thread(target=consume)
    reader.start()
    gate.release(2)  # the worker runs two frames of A and then sits in the third
    assert a.cancel()  # (this thread is not the worker's)
    gate.release(1000)
    assert _own(2, 3) == b.result(timeout=30).codes.T.tolist()  # A's row went to B
    reader.join(timeout=30)
    assert not reader.is_alive() and seen[-1] is CancelledError and a.future.cancelled()
    assert bat.stats["cancelled"] == 1 and ("admit", 0, 2, 0, 3) in eng.calls
    parks = [i for i, c in enumerate(eng.calls) if c == ("park", 0)]
    assert parks and parks[0] < eng.calls.index(("admit", 0, 2, 0, 3))
    bat.close()


def test_the_idle_worker_wakes_for_a_control_alone():
    eng = Engine()
    bat = _batcher(eng).start()
    done = _req(bat, 1, 2)
    done.result(timeout=30)
    with bat._lock:  # a wish that arrives for a request the scheduler no longer has: the worker takes it and goes back to waiting
        bat._controls.append((done, "cancel", None))
        bat._wake.notify()
    nxt = _req(bat, 2, 2)
    assert nxt.result(timeout=30).frames == 2
    bat.close()
    assert not bat._controls and done.result(timeout=0).frames == 2


def test_close_with_controls_pending_returns_and_every_future_is_done():
    eng = Engine()
    bat = _batcher(eng, max_batch=2, stream_chunk_frames=3)
    a, b, c = _req(bat, 1, 40, stream=True), _req(bat, 2, 40), _req(bat, 4, 40)
    for _ in range(4):
        assert bat.step()
    assert a.cancel() and bat.interrupt(b, played_frames=2) and bat.cancel(c)
    bat.close()
    assert a.future.done() and b.done() and c.done()
    assert _cancelled(a.future) and _cancelled(c)
    with pytest.raises(RuntimeError, match="closed"):  # (no round runs any more: the interrupt is not applied)
        b.result(timeout=0)
    with pytest.raises(CancelledError):
        list(a)
    assert bat._live() == [] and not bat._controls and _marks(eng, "park")[-2:] == [("park", 0), ("park", 1)]
