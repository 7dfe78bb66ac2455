"""Requests on a shared voice prefix (`CSMBatcher.submit(prefix=...)`) against a scripted engine (no device): a prefixed request counts with
prefix + suffix frames wherever the scheduler reasons about lengths (the limit at submit, the up-shift, the bare-position move), is admitted
through the prefixed admission in FIFO order among plain requests, and never reaches the engine's prompt-building / encode path.  The engine
enforces the library's rules (parked row, n + S <= P, windows inside the cache), so a scheduling mistake fails loudly here."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd.csm_serve import CSMBatcher  # noqa: E402
from mlx_audio_amd.sesame import make_sampler  # noqa: E402

N_CB = 2


class ScriptedPrefix:
    """What the scheduler reads of a sesame.VoicePrefix: its length (and the engine, its origin)."""

    def __init__(self, length, root):
        self.length, self.root = length, root


class ScriptedEngine:
    """Stream `tag` (the text token of its own first text frame) emits frame i = [tag, i + 1].  A row's window holds the WHOLE prompt: prefix and
    suffix."""

    def __init__(self, max_pos=64):
        self.n_cb, self.max_pos, self.sample_rate, self.device = N_CB, max_pos, 24000, torch.device("cpu")
        self.calls, self.built = [], []

    def start(self, max_batch):
        self.max_batch, self.pad, self.P = max_batch, [self.max_pos] * max_batch, 0
        self.tag, self.local = [None] * max_batch, [0] * max_batch

    def voice_prefix(self, length):
        return ScriptedPrefix(length, self)

    def _frames(self, ids):
        tok = np.zeros((len(ids), N_CB + 1), np.int32)
        tok[:, -1] = ids
        return tok, np.ones_like(tok, np.float32)

    # the prompt-building / encode path of plain requests
    def prompt_length(self, context, text, speaker, voice_match):
        self.built.append(("prompt_length", tuple(text)))
        return len(text)

    def prompts(self, streams):
        self.built.append(("prompts", tuple(tuple(s.text) for s in streams)))
        return [self._frames(s.text) for s in streams]

    # the one method prefixed requests need: host work only
    def prefixed_prompt(self, prefix, text, speaker):
        if prefix.root is not self:
            raise ValueError("the voice prefix was made on another engine")
        return self._frames(text)

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
        S, tag = prompt[0].shape[0], int(prompt[0][0, -1])
        assert self.pad[row] == self.max_pos, "admission into a live row"
        assert n + S <= self.P, "prefix + suffix longer than the position"
        assert prefix is None or prefix.root is self, "a prefix of another engine reached the admission"
        self.calls.append(("admit", row, tag, n, S, self.P))
        self.pad[row], self.tag[row], self.local[row] = self.P - n - S, tag, 1
        return torch.tensor([tag, 1], dtype=torch.int32)

    def frame(self, prev, sampler, uniforms, seed, stream_ids):
        assert self.P < self.max_pos, "frame beyond the cache"
        out = []
        for r in range(self.max_batch):
            if self.tag[r] is None:
                out.append([7, 7])
            else:
                assert prev[r].tolist() == [self.tag[r], self.local[r]], "a row was not fed its own last frame"
                self.local[r] += 1
                out.append([self.tag[r], self.local[r]])
        self.calls.append(("frame", self.P, tuple(self.tag)))
        self.P += 1
        return torch.tensor(out, dtype=torch.int32)

    def decode(self, codes):
        return codes.to(torch.float32).sum(dim=1).repeat_interleave(3, dim=1)

    def synchronize(self):
        pass


def _batcher(engine, **kw):
    kw.setdefault("rng", "host")
    return CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=engine, **kw)


def _plain(bat, tag, length, frames):
    return bat.submit(None, [tag] * length, max_audio_length_ms=80 * frames)


def _prefixed(bat, vp, tag, length, frames):
    return bat.submit(prefix=vp, text=[tag] * length, max_audio_length_ms=80 * frames)


def _own_frames(res, tag):
    return res.codes.T.tolist() == [[tag, i + 1] for i in range(res.frames)]


def test_the_limit_at_submit_counts_prefix_and_suffix():
    eng = ScriptedEngine(max_pos=64)
    bat = _batcher(eng, max_batch=2)
    vp = eng.voice_prefix(30)
    with pytest.raises(ValueError, match="Inputs too long"):
        _prefixed(bat, vp, 1, 14, 20)  # 30 + 14 + 20 >= 64
    fut = _prefixed(bat, vp, 1, 13, 20)  # 30 + 13 + 20 = 63 < 64
    assert not [c for c in eng.calls if c[0] != "start"]
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert res.frames == 20 and _own_frames(res, 1)
    # nothing was live: the bare position moved to the whole prompt's length, and the window starts at slot 0
    assert eng.calls[0] == ("shift", 43, 0, None) and eng.calls[1] == ("admit", 0, 1, 30, 13, 43)


def test_up_shift_by_exactly_the_missing_slots_of_prefix_plus_suffix():
    eng = ScriptedEngine()
    bat = _batcher(eng, max_batch=2)
    f1 = _plain(bat, 1, 3, 30)
    bat.step(); bat.step()
    assert eng.row_state() == ([0, 64], 5)
    vp = eng.voice_prefix(9)
    f2 = _prefixed(bat, vp, 2, 4, 5)  # n + S = 13 > P = 5
    bat.step()
    ups = [c for c in eng.calls if c[0] == "shift"]
    assert [c[1] for c in ups] == [3, 9 + 4 - 5]
    assert ("admit", 1, 2, 9, 4, 13) in eng.calls and eng.row_state() == ([8, 0], 14)
    f3 = _prefixed(bat, vp, 3, 2, 3)  # fits below the position: no shift
    bat.run_until_idle()
    assert [c[1] for c in eng.calls if c[0] == "shift"] == [3, 8]
    assert [f.result(timeout=0).frames for f in (f1, f2, f3)] == [30, 5, 3]
    assert bat.stats["prefixed_admissions"] == 2 and bat.stats["admissions"] == 3 and bat.stats["shifts_up"] == 2


def test_down_shift_is_unchanged_by_prefixed_rows():
    eng = ScriptedEngine(max_pos=32)
    bat = _batcher(eng, max_batch=2, eos_check_interval=100)
    vp = eng.voice_prefix(5)
    futs = [_prefixed(bat, vp, 1, 2, 10), _plain(bat, 2, 6, 14), _prefixed(bat, vp, 3, 3, 18), _plain(bat, 4, 4, 20)]
    bat.run_until_idle()
    downs = [c for c in eng.calls if c[0] == "shift" and c[1] < 0 and c[3] is not None]
    assert downs and all(c[2] == 32 and c[1] == -c[3] for c in downs)  # at P = max_pos, by min(pad[live]) -- a prefixed row's pad covers its prefix
    i = eng.calls.index(downs[0])
    assert eng.calls[i - 1][0] != "shift" and eng.calls[i + 1][0] == "frame"
    assert all(c[1] < 32 for c in eng.calls if c[0] == "frame")
    assert [f.result(timeout=0).frames for f in futs] == [10, 14, 18, 20]


def test_fifo_across_plain_and_prefixed_requests():
    eng = ScriptedEngine()
    bat = _batcher(eng, max_batch=2, eos_check_interval=4)
    vp = eng.voice_prefix(6)
    futs = [_plain(bat, 1, 4, 5), _prefixed(bat, vp, 2, 3, 9), _prefixed(bat, vp, 3, 2, 4), _plain(bat, 4, 5, 4), _prefixed(bat, vp, 5, 1, 3)]
    bat.run_until_idle()
    admits = [c for c in eng.calls if c[0] == "admit"]
    assert [c[2] for c in admits] == [1, 2, 3, 4, 5]
    assert [c[3] for c in admits] == [0, 6, 6, 0, 6]  # which admissions went through the prefix
    for t, (fut, f) in enumerate(zip(futs, (5, 9, 4, 4, 3)), start=1):
        res = fut.result(timeout=0)
        assert res.frames == f and _own_frames(res, t)
    assert bat.stats["admissions"] == 5 and bat.stats["prefixed_admissions"] == 3


def test_no_prompt_building_for_a_prefixed_request():
    eng = ScriptedEngine()
    bat = _batcher(eng, max_batch=2)
    vp = eng.voice_prefix(8)
    futs = [_prefixed(bat, vp, 1, 3, 4), _prefixed(bat, vp, 2, 2, 4)]
    bat.run_until_idle()
    assert eng.built == [] and all(f.result(timeout=0).frames == 4 for f in futs)
    _plain(bat, 3, 4, 2)  # (the counter does see the plain path)
    bat.run_until_idle()
    assert [b[0] for b in eng.built] == ["prompt_length", "prompts"]


@pytest.mark.parametrize("extra", [dict(context=["a segment"]), dict(prompt=(np.zeros((2, 3), np.int32), np.ones((2, 3), np.float32))),
                                   dict(voice_match=True)])
def test_prefix_excludes_context_prompt_and_voice_match(extra):
    eng = ScriptedEngine()
    bat = _batcher(eng, max_batch=2)
    with pytest.raises(ValueError):
        bat.submit(prefix=eng.voice_prefix(4), text=[1, 1], max_audio_length_ms=800, **extra)
    assert not bat._queue and not [c for c in eng.calls if c[0] != "start"]


def test_a_prefix_of_another_engine_is_refused_at_submit():
    eng, other = ScriptedEngine(), ScriptedEngine()
    bat = _batcher(eng, max_batch=2)
    with pytest.raises(ValueError):
        _prefixed(bat, other.voice_prefix(4), 1, 2, 5)
    assert not bat._queue and eng.calls == []
