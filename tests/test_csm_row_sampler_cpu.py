"""csm_serve.CSMBatcher(row_samplers=True) against a scripted engine (no device): which sampler and seed reach `admit` and `set_row_sampler`
for which row, what the frame step is asked for, which host draws are consumed, and the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_csm_serve_cpu import N_CB, FakeEngine  # noqa: E402

from mlx_audio_amd.csm_serve import CSMBatcher  # noqa: E402
from mlx_audio_amd.sesame import make_sampler  # noqa: E402


class RowEngine(FakeEngine):
    """FakeEngine with the sampler table: records what every admission and every frame was given."""

    def start(self, max_batch):
        super().start(max_batch)
        self.table = [None] * max_batch
        self.admitted, self.frames = [], []

    def admit(self, row, prompt, sampler, uniforms, seed, stream_id):
        self.admitted.append(dict(row=row, tag=int(prompt[0][0, -1]), sampler=sampler, uniforms=None if uniforms is None else np.array(uniforms), seed=seed))
        return super().admit(row, prompt, sampler, uniforms, seed, stream_id)

    def set_row_sampler(self, row, sampler, seed):
        assert self.tag[row] is not None, "the entry is written behind the row's admission"
        self.calls.append(("set_row_sampler", row, self.tag[row]))
        self.table[row] = (sampler, seed)

    def frame(self, prev, sampler, uniforms, seed, stream_ids, device_rng=False):
        self.frames.append(dict(sampler=sampler, uniforms=None if uniforms is None else np.array(uniforms), seed=seed, ids=stream_ids, device_rng=device_rng,
                                tags=tuple(self.tag)))
        return super().frame(prev, sampler, uniforms, seed, stream_ids)


GREEDY, TOPK, TOPP = make_sampler(temp=0.0), make_sampler(temp=0.8, top_k=20), make_sampler(temp=1.1, top_k=0, top_p=0.9)


def _req(bat, tag, length, frames, **kw):
    return bat.submit(None, [tag] * length, max_audio_length_ms=80 * frames, **kw)


def test_the_requests_sampler_reaches_admit_and_the_rows_entry():
    eng = RowEngine()
    bat = CSMBatcher(None, sampler=TOPK, engine=eng, rng="device", seed=9, max_batch=2, eos_check_interval=4, row_samplers=True)
    futs = [_req(bat, 1, 3, 4, sampler=GREEDY), _req(bat, 2, 4, 12, sampler=TOPP, seed=1234), _req(bat, 3, 3, 5)]  # the third: the batcher's sampler and seed
    bat.run_until_idle()
    by_tag = {a["tag"]: a for a in eng.admitted}
    assert by_tag[1]["sampler"] is GREEDY and by_tag[2]["sampler"] is TOPP and by_tag[3]["sampler"] is TOPK  # None falls back to the batcher's
    assert by_tag[1]["seed"] is None and by_tag[2]["seed"] == 1234 and by_tag[3]["seed"] == 9  # (a greedy admission draws nothing)
    assert by_tag[3]["row"] == by_tag[1]["row"]  # the reused row
    sets = [c for c in eng.calls if c[0] == "set_row_sampler"]
    assert [(c[1], c[2]) for c in sets] == [(by_tag[t]["row"], t) for t in (1, 2, 3)]  # one entry per admission, for the row it was given
    for c in sets:  # right behind its admission: no frame ran on a stale entry
        i = eng.calls.index(c)
        assert eng.calls[i - 1][0] == "admit" and eng.calls[i - 1][1] == c[1]
    assert eng.table[by_tag[3]["row"]] == (TOPK, 9) and eng.table[by_tag[2]["row"]] == (TOPP, 1234)
    # the frame step: table mode, the device generator, stream ids per row, no launch-argument sampler or seed, no uniforms
    assert eng.frames and all(f["sampler"] == "rows" and f["device_rng"] and f["seed"] is None and f["uniforms"] is None and len(f["ids"]) == 2 for f in eng.frames)
    for t, (fut, n) in enumerate(zip(futs, (4, 12, 5)), start=1):
        assert fut.result(timeout=0).frames == n


def test_a_greedy_stream_consumes_no_host_draws():
    eng = RowEngine()
    bat = CSMBatcher(None, sampler=TOPK, engine=eng, rng="host", max_batch=2, eos_check_interval=4, row_samplers=True)
    _req(bat, 1, 3, 6, sampler=GREEDY, seed=5)
    _req(bat, 2, 3, 6, sampler=TOPP, seed=6)
    bat.run_until_idle()
    by_tag = {a["tag"]: a for a in eng.admitted}
    assert by_tag[1]["uniforms"] is None and by_tag[1]["seed"] is None
    ref = np.random.default_rng(6)  # the sampled stream: one [n_cb] draw at its admission, one per frame -- the draws of its solo run
    np.testing.assert_array_equal(by_tag[2]["uniforms"], ref.uniform(size=(1, N_CB))[0].astype(np.float32))
    r1, r2 = by_tag[1]["row"], by_tag[2]["row"]
    seen = 0
    for f in eng.frames:
        assert f["sampler"] == "rows" and not f["device_rng"] and f["ids"] is None and f["uniforms"].shape == (2, N_CB)
        if f["tags"][r2] == 2:
            np.testing.assert_array_equal(f["uniforms"][r2], ref.uniform(size=(1, N_CB))[0].astype(np.float32))
            seen += 1
        np.testing.assert_array_equal(f["uniforms"][r1], np.full(N_CB, 0.5, np.float32))  # the greedy row (live or parked): a constant
    assert seen >= 5


def test_refusals_without_row_samplers_and_invalid_samplers():
    eng = RowEngine()
    plain = CSMBatcher(None, sampler=TOPK, engine=eng, rng="device", seed=9, max_batch=2)
    with pytest.raises(ValueError, match="row_samplers"):
        _req(plain, 1, 3, 4, sampler=GREEDY)
    with pytest.raises(ValueError, match="batcher's seed"):
        _req(plain, 1, 3, 4, seed=10)
    _req(plain, 1, 3, 4, seed=9)  # its own seed is fine, as before
    plain.run_until_idle()
    assert not [c for c in eng.calls if c[0] == "set_row_sampler"] and all(f["sampler"] is TOPK and f["seed"] == 9 for f in eng.frames)

    class Bad:
        temp, top_k, top_p = 0.5, 5, 1.5

    bat = CSMBatcher(None, sampler=TOPK, engine=RowEngine(), rng="host", max_batch=2, row_samplers=True)
    for bad in (Bad(), type("S", (), dict(temp=-0.1, top_k=5))(), type("S", (), dict(temp=0.5, top_k=-2))(), type("S", (), dict(temp=0.5, top_k=5, min_p=2.0))(),
                type("S", (), dict(temp=0.5, top_k=5, min_tokens_to_keep=0))(), object()):
        with pytest.raises(ValueError):
            _req(bat, 1, 3, 4, sampler=bad)
    assert not bat._queue  # refused at submit: nothing was queued
    with pytest.raises(ValueError):
        CSMBatcher(None, sampler=Bad(), engine=RowEngine(), rng="host", row_samplers=True)

