"""Admissions prefilled in lanes (`CSMBatcher(overlap_admission=True, prefill_lanes=)`) against a scripted engine (no device): when
a prefill begins, that frames go on while a lane is busy, when a request is committed, FIFO order with two lanes, what a lane failure and
`close()` do to the requests a lane holds, and that nothing of this is touched with the option off.  The engine enforces the library's rules
(a commit needs a parked row, a window that fits below the position and the lane that holds that very request), so a scheduling mistake
fails loudly here."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd.csm_serve import CSMBatcher  # noqa: E402

N_CB = 2


def _text(ids):
    tok = np.zeros((len(ids), N_CB + 1), np.int32)
    msk = np.zeros((len(ids), N_CB + 1), np.float32)
    tok[:, -1], msk[:, -1] = ids, 1
    return tok, msk


class ScriptedEngine:
    """The stream whose prompt ends with text token `tag` emits frame i = [tag, i + 1].  A lane holds one prefill at a time; `busy` holds the tags
    whose lane answers "not ready" until the test takes them out.  `calls` logs what the scheduler did, in order."""

    def __init__(self, max_pos=64, busy=None, fail_prefill=(), lanes_allowed=True):
        self.n_cb, self.max_pos, self.sample_rate, self.device = N_CB, max_pos, 24000, torch.device("cpu")
        self.calls, self.busy, self.fail_prefill, self.lanes_allowed = [], set(busy or ()), set(fail_prefill), lanes_allowed
        self.lanes = None

    def start(self, max_batch):
        self.max_batch, self.pad, self.P = max_batch, [self.max_pos] * max_batch, 0
        self.tag, self.local = [None] * max_batch, [0] * max_batch

    def prompt_length(self, context, text, speaker, voice_match):
        return len(text)

    def prompts(self, streams):
        return [_text(s.text) for s in streams]

    def row_state(self):
        return list(self.pad), self.P

    def park(self, row):
        self.calls.append(("park", row))
        self.pad[row], self.tag[row] = self.max_pos, None

    def shift(self, delta):
        live = [p for p in self.pad if p < self.max_pos]
        assert 0 <= self.P + delta <= self.max_pos and all(p + delta >= 0 for p in live), "shift out of the cache"
        self.calls.append(("shift", delta))
        self.pad = [p + delta if p < self.max_pos else p for p in self.pad]
        self.P += delta

    def admit(self, row, prompt, sampler, uniforms, seed, stream_id, prefix=None):
        S, tag = prompt[0].shape[0], int(prompt[0][-1, -1])
        assert self.pad[row] == self.max_pos and S <= self.P
        self.calls.append(("admit", row, tag))
        self.pad[row], self.tag[row], self.local[row] = self.P - S, tag, 1
        return torch.tensor([tag, 1], dtype=torch.int32)

    def frame(self, prev, sampler, uniforms, seed, stream_ids, device_rng=False):
        assert self.P < self.max_pos, "frame beyond the cache"
        out = []
        for r in range(self.max_batch):
            if self.tag[r] is None:
                out.append([7, 7])
            else:
                assert prev[r].tolist() == [self.tag[r], self.local[r]], "a row was not fed its own last frame"
                self.local[r] += 1
                out.append([self.tag[r], self.local[r]])
        self.calls.append(("frame", tuple(t for t in self.tag if t is not None)))
        self.P += 1
        return torch.tensor(out, dtype=torch.int32)

    def synchronize(self):
        pass

    # ---- the lanes
    def open_lanes(self, n):
        assert self.lanes_allowed, "lanes were opened with the option off"
        self.lanes = [None] * n
        self.calls.append(("open_lanes", n))

    def prefill(self, lane, prompt, sampler, uniforms, seed, stream_id, prefix=None, timed=False):
        assert self.lanes_allowed and self.lanes[lane] is None, "a prefill into a lane that holds a request"
        S, tag = prompt[0].shape[0], int(prompt[0][-1, -1])
        if tag in self.fail_prefill:
            raise RuntimeError("scripted lane failure")
        self.calls.append(("prefill", lane, tag))
        self.lanes[lane] = h = {"tag": tag, "L": S, "lane": lane}
        return h

    def prefill_ready(self, handle, wait=False):
        assert self.lanes_allowed
        if wait:
            assert not any(t is not None for t in self.tag), "the scheduler waited for a lane while rows were live"
            self.busy.discard(handle["tag"])
            self.calls.append(("wait", handle["tag"]))
            return True
        return handle["tag"] not in self.busy

    def commit(self, row, lane, handle):
        assert self.lanes_allowed and self.lanes[lane] is handle, "the lane does not hold this request"
        assert handle["tag"] not in self.busy, "a commit before the lane was ready"
        assert self.pad[row] == self.max_pos, "commit into a live row"
        assert handle["L"] <= self.P, "the admission is longer than the position"
        self.calls.append(("commit", row, handle["tag"], lane))
        self.pad[row], self.tag[row], self.local[row] = self.P - handle["L"], handle["tag"], 1
        self.lanes[lane] = None
        return torch.tensor([handle["tag"], 1], dtype=torch.int32)

    def close_lanes(self):
        self.calls.append(("close_lanes",))

    def row_decoder(self, max_batch, max_frames, max_chunk):
        class Decoder:
            def reset_row(self, row):
                pass

            def step(self, codes, active):
                return torch.zeros((codes.shape[0], 1, 4 * codes.shape[2]))

            def close(self):
                pass

        return Decoder()


def _batcher(eng, max_batch, lanes=1, decode=False, **kw):
    return CSMBatcher(None, max_batch=max_batch, engine=eng, decode=decode, eos_check_interval=1, overlap_admission=True, prefill_lanes=lanes, **kw)


def _submit(bat, tag, n_text, frames):
    return bat.submit(None, [3] * (n_text - 1) + [tag], max_audio_length_ms=80 * frames, voice_match=False)


def _codes(fut):
    return fut.result(timeout=0).codes.T.tolist()


def _marks(calls, *kinds):
    return [c for c in calls if c[0] in kinds]


def test_a_prefill_begins_when_the_request_reaches_the_queue_head_even_without_a_free_row():
    eng = ScriptedEngine()
    bat = _batcher(eng, max_batch=1)
    a, b = _submit(bat, 11, 4, 3), _submit(bat, 12, 6, 2)
    assert bat.step()
    # round 1: A goes to the lane, nothing is live so the batcher waits for it and commits; the lane is free again and takes B in the same
    # round -- behind the frame's launch --, although the only row is now A's
    assert eng.calls == [("open_lanes", 1), ("prefill", 0, 11), ("wait", 11), ("shift", 4), ("commit", 0, 11, 0), ("frame", (11,)), ("prefill", 0, 12)]
    assert bat.stats["overlapped_admissions"] == 1 and len(bat._inflight) == 1 and not bat._queue
    bat.run_until_idle()
    assert _codes(a) == [[11, 1], [11, 2], [11, 3]] and _codes(b) == [[12, 1], [12, 2]]
    assert _marks(eng.calls, "admit") == [] and bat.stats["overlapped_admissions"] == bat.stats["admissions"] == 2


def test_frames_go_on_while_the_lane_is_busy_and_the_commit_comes_with_the_first_ready_lane_and_free_row():
    eng = ScriptedEngine(busy={12})
    bat = _batcher(eng, max_batch=2)
    a = _submit(bat, 11, 3, 9)
    assert bat.step()
    b = _submit(bat, 12, 5, 2)
    before = len(eng.calls)
    for _ in range(3):
        assert bat.step()
    eng.busy.clear()
    assert bat.step()
    # B reaches the lane in the round it arrives (behind that round's frame); two more rounds find the lane "not ready" and run A's frame
    # alone; the next commits B (a row was free all along) and steps both
    assert eng.calls[before:] == [("frame", (11,)), ("prefill", 0, 12), ("frame", (11,)), ("frame", (11,)), ("commit", 1, 12, 0), ("frame", (11, 12))]
    assert not _marks(eng.calls, "wait")[1:]  # only A's, when nothing was live
    bat.run_until_idle()
    assert _codes(b) == [[12, 1], [12, 2]] and len(_codes(a)) == 9


def test_a_ready_lane_waits_for_a_row_and_an_up_shift_comes_at_the_commit():
    eng = ScriptedEngine()
    bat = _batcher(eng, max_batch=1)
    a = _submit(bat, 11, 2, 4)
    b = _submit(bat, 12, 9, 2)  # longer than the position will be when A's row is free (2 + 3 frames): the position moves at the commit
    bat.run_until_idle()
    calls = _marks(eng.calls, "prefill", "commit", "shift", "park")
    assert calls == [("prefill", 0, 11), ("shift", 2), ("commit", 0, 11, 0), ("prefill", 0, 12), ("park", 0), ("shift", 4), ("commit", 0, 12, 0), ("park", 0)]
    assert _codes(a) == [[11, i] for i in range(1, 5)] and _codes(b) == [[12, 1], [12, 2]]


def test_fifo_order_is_kept_with_two_lanes():
    eng = ScriptedEngine(busy={12})
    bat = _batcher(eng, max_batch=3, lanes=2)
    a = _submit(bat, 11, 3, 12)
    assert bat.step()
    b, c = _submit(bat, 12, 4, 2), _submit(bat, 13, 2, 2)  # C's lane is ready at once, B's only later
    for _ in range(3):
        assert bat.step()
        assert bat.stats["overlapped_admissions"] == 1 and [s.stream_id for s in bat._inflight] == [1, 2]  # C does not overtake B
    eng.busy.clear()
    bat.run_until_idle()
    assert _marks(eng.calls, "prefill") == [("prefill", 0, 11), ("prefill", 0, 12), ("prefill", 1, 13)]
    assert _marks(eng.calls, "commit") == [("commit", 0, 11, 0), ("commit", 1, 12, 0), ("commit", 2, 13, 1)]
    for f, tag in ((b, 12), (c, 13)):
        assert _codes(f) == [[tag, 1], [tag, 2]]
    assert len(_codes(a)) == 12 and bat.stats["overlapped_admissions"] == 3


def test_a_lane_error_fails_only_that_request_and_frees_the_lane():
    eng = ScriptedEngine(fail_prefill={12})
    bat = _batcher(eng, max_batch=2)
    a, b, c = _submit(bat, 11, 3, 3), _submit(bat, 12, 3, 3), _submit(bat, 13, 3, 3)
    bat.run_until_idle()
    with pytest.raises(RuntimeError, match="scripted lane failure"):
        b.result(timeout=0)
    assert len(_codes(a)) == 3 and len(_codes(c)) == 3
    assert _marks(eng.calls, "prefill") == [("prefill", 0, 11), ("prefill", 0, 13)] and eng.lanes == [None]


def test_close_fails_the_requests_a_lane_holds():
    eng = ScriptedEngine(busy={12})
    bat = _batcher(eng, max_batch=1, lanes=1, decode=True, stream_chunk_frames=2, stream_max_frames=8)
    a = _submit(bat, 11, 3, 8)
    assert bat.step()
    held = bat.submit_stream(None, [3, 12], max_audio_length_ms=80 * 4, voice_match=False)
    queued = _submit(bat, 13, 2, 2)
    assert bat.step() and [s.stream_id for s in bat._inflight] == [1] and len(bat._queue) == 1
    bat.close()
    for f in (a, held.future, queued):
        with pytest.raises(RuntimeError, match="closed"):
            f.result(timeout=0)
    with pytest.raises(RuntimeError, match="closed"):  # the iterator ends by raising, it does not hang
        list(held)
    assert eng.calls[-1] == ("close_lanes",) and not bat._inflight


def test_with_the_option_off_the_lane_methods_are_never_called():
    eng = ScriptedEngine(lanes_allowed=False)
    bat = CSMBatcher(None, max_batch=2, engine=eng, decode=False, eos_check_interval=1)
    futs = [_submit(bat, 11 + i, 3, 2) for i in range(3)]
    bat.run_until_idle()
    bat.close()
    assert all(len(_codes(f)) == 2 for f in futs)
    assert len(_marks(eng.calls, "admit")) == 3 and not _marks(eng.calls, "open_lanes", "prefill", "commit", "wait", "close_lanes")
    assert bat.stats["overlapped_admissions"] == 0 and bat.stats["commit_seconds"] == 0.0 and bat.stats["prefill_seconds"] == 0.0
