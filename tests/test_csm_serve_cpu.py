"""The scheduler of csm_serve.CSMBatcher against a scripted engine (no device): which admit / park / shift / frame calls it makes, in which
order, and what each request gets back.  The engine enforces the library's rules (a row is admitted only while parked, S <= P, windows stay
inside the cache, no frame at P = max_pos), so a scheduling mistake fails loudly here."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd.csm_serve import CSMBatcher  # noqa: E402
from mlx_audio_amd.sesame import make_sampler  # noqa: E402

N_CB = 2


class FakeEngine:
    """Stream `tag` (the text token of its prompt's first frame) emits frame i = [tag, i + 1] -- or [0, 0] (EOS) at i = eos[tag]."""

    def __init__(self, max_pos=64, eos=None):
        self.n_cb, self.max_pos, self.sample_rate, self.device = N_CB, max_pos, 24000, torch.device("cpu")
        self.eos = eos or {}
        self.calls = []

    def start(self, max_batch):
        self.max_batch, self.pad, self.P = max_batch, [self.max_pos] * max_batch, 0
        self.tag, self.local = [None] * max_batch, [0] * max_batch

    def prompt_length(self, context, text, speaker, voice_match):
        return len(text)

    def prompts(self, streams):
        out = []
        for s in streams:
            tok = np.zeros((len(s.text), N_CB + 1), np.int32)
            tok[:, -1] = s.text
            out.append((tok, np.ones_like(tok, np.float32)))
        return out

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

    def _code(self, tag, i):
        return [0, 0] if self.eos.get(tag) == i else [tag, i + 1]

    def admit(self, row, prompt, sampler, uniforms, seed, stream_id):
        S, tag = prompt[0].shape[0], int(prompt[0][0, -1])
        assert self.pad[row] == self.max_pos, "admission into a live row"
        assert S <= self.P, "prompt longer than the position"
        self.calls.append(("admit", row, tag, S, self.P))
        self.pad[row], self.tag[row], self.local[row] = self.P - S, tag, 1
        return torch.tensor(self._code(tag, 0), dtype=torch.int32)

    def frame(self, prev, sampler, uniforms, seed, stream_ids):
        assert self.P < self.max_pos, "frame beyond the cache"
        out = []
        for r in range(self.max_batch):
            if self.tag[r] is None:
                out.append([7, 7])
            else:
                assert prev[r].tolist() == self._code(self.tag[r], self.local[r] - 1), "a row was not fed its own last frame"
                out.append(self._code(self.tag[r], self.local[r]))
                self.local[r] += 1
        self.calls.append(("frame", self.P, tuple(self.tag)))
        self.P += 1
        return torch.tensor(out, dtype=torch.int32)

    def decode(self, codes):
        return codes.to(torch.float32).sum(dim=1).repeat_interleave(3, dim=1)  # [b, 3 T]

    def synchronize(self):
        pass


def _batcher(engine, **kw):
    kw.setdefault("rng", "host")
    return CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=engine, **kw)


def _req(bat, tag, length, frames):
    return bat.submit(None, [tag] * length, max_audio_length_ms=80 * frames)


def _frames_of(res, tag):
    return res.codes.T.tolist() == [[tag, i + 1] for i in range(res.frames)]


def test_fifo_admission_and_row_reuse_only_after_park():
    eng = FakeEngine()
    bat = _batcher(eng, max_batch=2, eos_check_interval=4)
    futs = [_req(bat, t, 3 + t, f) for t, f in ((1, 5), (2, 9), (3, 4), (4, 4))]
    bat.run_until_idle()
    admits = [c for c in eng.calls if c[0] == "admit"]
    assert [c[2] for c in admits] == [1, 2, 3, 4]  # FIFO
    for c in admits[2:]:  # a reused row was parked between its two admissions
        i = eng.calls.index(c)
        before = [k for k in eng.calls[:i] if k[0] in ("admit", "park") and k[1] == c[1]]
        assert before[-1][0] == "park"
    for t, (fut, f) in enumerate(zip(futs, (5, 9, 4, 4)), start=1):
        res = fut.result(timeout=0)
        assert res.frames == f and _frames_of(res, t) and res.audio.shape == (3 * f,) and res.sample_rate == 24000
    assert bat.stats["admissions"] == 4 and bat.stats["finished"] == 4
    assert 0 < bat.occupancy <= 1


def test_eos_is_polled_every_interval_and_surplus_frames_are_trimmed():
    eng = FakeEngine(eos={1: 3, 2: 10})
    bat = _batcher(eng, max_batch=2, eos_check_interval=8)
    f1, f2 = _req(bat, 1, 4, 40), _req(bat, 2, 4, 40)
    bat.run_until_idle()
    r1, r2 = f1.result(timeout=0), f2.result(timeout=0)
    assert (r1.frames, r2.frames) == (3, 10) and _frames_of(r1, 1) and _frames_of(r2, 2)
    # stream 1 hit EOS at its frame 3 but rode along until the first poll, after 8 single-token frames; stream 2 until the second
    parks = [i for i, c in enumerate(eng.calls) if c[0] == "park"]
    frames_before = [sum(1 for c in eng.calls[:i] if c[0] == "frame") for i in parks]
    assert frames_before == [8, 16] and bat.stats["polls"] == 2


def test_per_request_frame_limits():
    eng = FakeEngine()
    bat = _batcher(eng, max_batch=3, eos_check_interval=100)
    futs = [_req(bat, t, 4, f) for t, f in ((1, 2), (2, 7), (3, 1))]
    bat.run_until_idle()
    assert [f.result(timeout=0).frames for f in futs] == [2, 7, 1]
    # a row is parked at its own limit: stream 3 after 0 single-token frames (its admission is its only frame), 1 after 1, 2 after 6
    parks = {c[1]: sum(1 for k in eng.calls[:i] if k[0] == "frame") for i, c in enumerate(eng.calls) if c[0] == "park"}
    assert parks == {2: 0, 0: 1, 1: 6}


def test_down_shift_exactly_when_the_position_reaches_the_end_by_the_smallest_live_pad():
    eng = FakeEngine(max_pos=32)
    bat = _batcher(eng, max_batch=2, eos_check_interval=100)
    futs = [_req(bat, 1, 4, 10), _req(bat, 2, 6, 14), _req(bat, 3, 5, 20), _req(bat, 4, 4, 20)]
    bat.run_until_idle()
    downs = [c for c in eng.calls if c[0] == "shift" and c[1] < 0 and c[3] is not None]  # (with no live row only the bare position moves)
    assert downs and all(c[2] == 32 and c[1] == -c[3] for c in downs)  # at P = max_pos, by min(pad[live])
    i = eng.calls.index(downs[0])
    assert eng.calls[i - 1][0] != "shift" and eng.calls[i + 1][0] == "frame"
    assert all(c[1] < 32 for c in eng.calls if c[0] == "frame")
    assert [f.result(timeout=0).frames for f in futs] == [10, 14, 20, 20]


def test_up_shift_by_the_missing_slots():
    eng = FakeEngine()
    bat = _batcher(eng, max_batch=2)
    f1 = _req(bat, 1, 3, 12)
    bat.step(); bat.step()
    assert eng.row_state() == ([0, 64], 5)
    f2 = _req(bat, 2, 11, 5)
    bat.step()
    ups = [c for c in eng.calls if c[0] == "shift"]
    assert [c[1] for c in ups] == [3, 11 - 5]  # the bare position 0 -> 3 for the first stream, then S - P
    assert ("admit", 1, 2, 11, 11) in eng.calls and eng.row_state() == ([6, 0], 12)
    bat.run_until_idle()
    assert f1.result(timeout=0).frames == 12 and f2.result(timeout=0).frames == 5


def test_over_long_requests_fail_at_submit():
    eng = FakeEngine(max_pos=32)
    bat = _batcher(eng, max_batch=2)
    with pytest.raises(ValueError, match="Inputs too long"):
        _req(bat, 1, 12, 20)  # 12 + 20 >= 32
    _req(bat, 1, 11, 20)
    with pytest.raises(ValueError):
        CSMBatcher(None, rng="device", seed=3, engine=FakeEngine()).submit(None, [1, 1], seed=4)
    assert not [c for c in eng.calls if c[0] != "start"]


def test_close_racing_submit_fails_the_future_and_never_hangs():
    eng = FakeEngine()
    bat = _batcher(eng, max_batch=2).start()
    done = _req(bat, 1, 3, 4).result(timeout=30)
    assert done.frames == 4
    futs, stop = [], threading.Event()

    def flood():
        while not stop.is_set() and len(futs) < 20000:
            futs.append(_req(bat, 2, 3, 50))

    t = threading.Thread(target=flood)
    t.start()
    while len(futs) < 50:
        pass
    bat.close()
    stop.set()
    t.join()
    late = _req(bat, 3, 3, 4)
    assert isinstance(late.exception(timeout=0), RuntimeError)
    for f in futs:  # every request resolved: a result, or the closed error -- none left pending
        assert f.done()
        assert f.exception(timeout=0) is None or isinstance(f.exception(timeout=0), RuntimeError)
    assert any(f.exception(timeout=0) is not None for f in futs)
