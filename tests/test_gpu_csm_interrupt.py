"""Stopping a request on the device (`CSMBatcher.cancel` / `interrupt`).  An interrupt at k frames leaves the session, and the turn
behind it, bit for bit where a limit of k frames leaves them; a turn interrupted behind its row's progress is captured the same in a busy batch
and alone; the rows beside a cancelled or an interrupted one carry the bits of their own `generate_batch([prompt])` runs and the freed row is
refilled in the round of the cancel; an interrupted stream's audio is the head of the uninterrupted stream's; a request dropped out of a
prefill lane leaves the lane to the next one.  No tolerance anywhere: every comparison is array equality.  The tiny configuration, driven
with `step()`; `stop_on_eos=False` where an accidental EOS frame would confuse the count."""
import functools
import os
import sys
from concurrent.futures import CancelledError

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import mlx_audio_amd.params as P  # noqa: E402

pytestmark = pytest.mark.gpu

TEMP, TOP_K, SEED = 0.8, 20, 1234
MAX_POS = 128
N_CB = 4


def _ccfg():
    return dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=N_CB, max_seq_len=MAX_POS)


def _bf16(w):
    return {k: torch.tensor(np.asarray(v, np.float32)).to(torch.bfloat16).float().numpy() for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _loop(wdt):
    from mlx_audio_amd.mimi import Mimi, MimiConfig
    from mlx_audio_amd.sesame import Model

    mcfg = P.mimi_tiny_config()
    cw = P.csm_synth_checkpoint(_ccfg(), 3)
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 3, encode=True))
    return Model(_ccfg(), mimi=mimi, weights=_bf16(cw) if wdt == "bfloat16" else cw, weight_dtype=wdt)


def _sampler():
    from mlx_audio_amd.sesame import make_sampler

    return make_sampler(temp=TEMP, top_k=TOP_K)


def _frames(g, n_text, n_audio):
    tok = np.zeros((n_text + n_audio, N_CB + 1), np.int32)
    msk = np.zeros((n_text + n_audio, N_CB + 1), np.float32)
    tok[:n_text, -1], msk[:n_text, -1] = g.integers(0, 300, n_text), 1
    tok[n_text:, :N_CB], msk[n_text:, :N_CB] = g.integers(1, 64, (n_audio, N_CB)), 1
    return tok, msk


def _drive(bat, fut):
    for _ in range(600):
        if fut.done():
            return
        bat.step()
    raise AssertionError("the request did not finish")


def _stream_of(bat, stream_id):
    return next((s for s in bat._live() if s.stream_id == stream_id), None)


def _step_until(bat, stream_id, frames):
    """Rounds until stream `stream_id` holds exactly `frames` frames; returns its scheduler entry."""
    for _ in range(200):
        s = _stream_of(bat, stream_id)
        if s is not None and len(s.codes) >= frames:
            assert len(s.codes) == frames
            return s
        assert bat.step()
    raise AssertionError("the stream never got there")


def _solo(loop, prompt, frames, stream_id, decode=False):
    ref = loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=_sampler(), seed=SEED, rng="device", stream_ids=[stream_id],
                              stop_on_eos=False, decode=decode)
    assert ref.frames[0] == frames
    return ref.codes[0][:, :frames].cpu().numpy(), (ref.audio[0].cpu() if decode else None)


# ---- 1. an interrupt when exactly k frames exist is a limit of k ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_interrupt_when_exactly_k_frames_exist_equals_a_limit_at_k(wdt):
    loop = _loop(wdt)
    g = np.random.default_rng(51)
    texts = [g.integers(0, 300, n).tolist() for n in (4, 3)]

    def run(interrupt):
        bat = loop.serve(max_batch=1, eos_check_interval=8, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False)
        sess = bat.session()
        fut = sess.submit(texts[0], max_audio_length_ms=80 * (40 if interrupt else 5), stream_id=50)
        if interrupt:
            _step_until(bat, 50, 5)
            assert sess.interrupt(played_frames=5) and not fut.done()
            assert bat.step() is False and fut.done()  # applied in one round; the batch of one is idle behind it
        else:
            _drive(bat, fut)
        r1 = fut.result(timeout=0)
        assert r1.frames == 5 and r1.interrupted is interrupt and sess.turns[-1][2] == 5 and not sess.busy
        state = (sess.n, sess.pending[0].copy(), sess.pending[1].copy(), sess.history[0].copy(), sess.history[1].copy())
        f2 = sess.submit(texts[1], max_audio_length_ms=80 * 8, stream_id=51)
        _drive(bat, f2)
        r2 = f2.result(timeout=0)
        stats = dict(bat.stats)
        sess.close()
        bat.close()
        return r1, state, r2, stats

    a1, a_state, a2, a_stats = run(False)
    b1, b_state, b2, b_stats = run(True)
    assert b_stats["interrupted"] == 1 and a_stats["interrupted"] == 0 and b_stats["captures"] == a_stats["captures"] == 2
    assert a_state[0] == b_state[0] and a_state[1].shape[0] == 2  # L + 4 positions; the fifth frame and the EOS frame are pending
    for x, y in zip(a_state[1:], b_state[1:]):
        np.testing.assert_array_equal(y, x)
    np.testing.assert_array_equal(b1.codes.cpu().numpy(), a1.codes.cpu().numpy())
    assert torch.equal(b1.audio, a1.audio)
    assert a2.frames == b2.frames == 8
    np.testing.assert_array_equal(b2.codes.cpu().numpy(), a2.codes.cpu().numpy())
    assert torch.equal(b2.audio, a2.audio)


# ---- 2. an interrupt behind the row's progress, busy against alone ----------------------------------------------------------------------------------
def test_interrupt_behind_the_rows_progress_is_captured_the_same_in_a_busy_batch_and_alone():
    """Turn 1 is interrupted at k = 5 when its row has generated 8 frames: the capture takes L + 5 positions, all of single-token steps behind
    the prompt.  Busy: a batch of four with plain and `prefix=` streams, the session's row at a non-zero pad, polls every 8 frames."""
    from mlx_audio_amd.sesame import Segment

    loop = _loop("float32")

    def run(busy):
        g = np.random.default_rng(52)
        texts = [g.integers(0, 300, n).tolist() for n in (4, 3)]
        ctx = [Segment(speaker=2, text=g.integers(0, 300, 4).tolist(), audio=(0.3 * g.standard_normal(1920 * 3)).astype(np.float32))]
        plain = [_frames(g, 14, 4), _frames(g, 5, 1)]
        bat = loop.serve(max_batch=4 if busy else 1, eos_check_interval=8 if busy else 1, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False)
        side, vp = [], None
        if busy:
            vp = loop.voice_prefix(ctx)
            side.append(bat.submit(None, None, prompt=plain[0], max_audio_length_ms=80 * 50, stream_id=80))
            for _ in range(3):
                assert bat.step()
            side.append(bat.submit(prefix=vp, text=g.integers(0, 300, 2).tolist(), speaker=2, max_audio_length_ms=80 * 30, stream_id=81))
            side.append(bat.submit(None, None, prompt=plain[1], max_audio_length_ms=80 * 25, stream_id=82))
        sess = bat.session()
        fut = sess.submit(texts[0], max_audio_length_ms=80 * 40, stream_id=50)
        s = _step_until(bat, 50, 8)
        pad, _ = loop.model.row_state()
        assert (pad[s.row] > 0) == busy and (s.row == 3) == busy
        L = s.length
        assert sess.interrupt(played_frames=5)
        bat.step()
        r1 = fut.result(timeout=0)
        assert r1.frames == 5 and r1.interrupted and sess.n == L + 5 and sess.pending[0].shape[0] == 1 and not sess.pending[0].any()
        f2 = sess.submit(texts[1], max_audio_length_ms=80 * 8, stream_id=51)
        _drive(bat, f2)
        r2 = f2.result(timeout=0)
        bat.run_until_idle()
        for f in side:
            assert not f.result(timeout=0).interrupted
        sess.close()
        bat.close()
        if vp is not None:
            vp.close()
        return r1, r2

    (s1, s2), (b1, b2) = run(False), run(True)
    np.testing.assert_array_equal(b1.codes.cpu().numpy(), s1.codes.cpu().numpy())
    assert s2.frames == b2.frames == 8
    np.testing.assert_array_equal(b2.codes.cpu().numpy(), s2.codes.cpu().numpy())
    assert torch.equal(b2.audio, s2.audio) and torch.equal(b1.audio, s1.audio)


# ---- 3. the neighbours ----------------------------------------------------------------------------------------------------------------------------
def test_the_rows_beside_a_cancelled_and_an_interrupted_one_are_untouched():
    loop = _loop("float32")
    g = np.random.default_rng(53)
    prompts = [_frames(g, 6, 2), _frames(g, 9, 3), _frames(g, 4, 1), _frames(g, 7, 0), _frames(g, 5, 2)]
    limits = [20, 30, 30, 14, 10]
    bat = loop.serve(max_batch=4, eos_check_interval=8, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False, decode=False)
    futs = [bat.submit(None, None, prompt=p, max_audio_length_ms=80 * f, stream_id=60 + i) for i, (p, f) in enumerate(zip(prompts, limits))]
    _step_until(bat, 61, 3)
    assert len(bat._queue) == 1 and [s.stream_id for s in bat._rows] == [60, 61, 62, 63]
    assert bat.cancel(futs[1])
    assert bat.step()
    assert futs[1].cancelled() and bat._rows[1].stream_id == 64 and bat.stats["admissions"] == 5  # the fifth request entered the row in the round of the cancel
    _step_until(bat, 62, 6)
    assert bat.interrupt(futs[2], played_frames=4)
    assert bat.step() and bat._rows[2] is None
    r2 = futs[2].result(timeout=0)
    assert r2.frames == 4 and r2.interrupted
    bat.run_until_idle()
    with pytest.raises(CancelledError):
        futs[1].result(timeout=0)
    assert bat.stats["cancelled"] == 1 and bat.stats["interrupted"] == 1 and bat.stats["finished"] == 4
    for i in (0, 3, 4):
        got = futs[i].result(timeout=0)
        want, _ = _solo(loop, prompts[i], limits[i], 60 + i)
        assert got.frames == limits[i] and not got.interrupted
        np.testing.assert_array_equal(got.codes.cpu().numpy(), want, err_msg=f"request {i}")
    want, _ = _solo(loop, prompts[2], limits[2], 62)
    np.testing.assert_array_equal(r2.codes.cpu().numpy(), want[:, :4])
    bat.close()


# ---- 4. streamed and interrupted ----------------------------------------------------------------------------------------------------------------
def test_an_interrupted_streams_audio_is_the_head_of_the_uninterrupted_streams():
    loop = _loop("float32")
    g = np.random.default_rng(54)
    prompt = _frames(g, 6, 2)

    def run(interrupt):
        bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False, stream_chunk_frames=3, stream_max_frames=16)
        st = bat.submit_stream(None, None, prompt=prompt, max_audio_length_ms=80 * 12, stream_id=50)
        if interrupt:
            s = _step_until(bat, 50, 7)
            assert s.emitted == 3
            assert st.interrupt(played_frames=4)
            bat.step()
        else:
            _drive(bat, st.future)
        spf = bat.engine.samples_per_frame
        out = list(st), st.result(timeout=0), spf
        bat.close()
        return out

    ref_chunks, ref, spf = run(False)
    chunks, res, _ = run(True)
    assert ref.frames == 12 and ref.audio.shape == (12 * spf,) and [c.frames for c in ref_chunks] == [3, 3, 3, 3]
    assert res.frames == 4 and res.interrupted and res.audio.shape == (4 * spf,)
    assert torch.equal(res.audio, ref.audio[: 4 * spf])
    np.testing.assert_array_equal(res.codes.cpu().numpy(), ref.codes[:, :4].cpu().numpy())
    assert [(c.first_frame, c.frames, c.final) for c in chunks] == [(0, 3, False), (3, 1, True)]  # no delivered chunk holds a frame >= 4
    assert torch.equal(chunks[0].audio, ref_chunks[0].audio) and torch.equal(chunks[1].audio, ref_chunks[1].audio[:spf])
    assert torch.equal(torch.cat([c.audio for c in chunks]), res.audio)


# ---- 5. a request dropped out of a prefill lane ----------------------------------------------------------------------------------------------------
def test_cancel_of_a_request_whose_prefill_is_in_the_lane():
    loop = _loop("float32")
    g = np.random.default_rng(55)
    prompts = [_frames(g, 8, 3), _frames(g, 12, 2), _frames(g, 5, 1)]
    limits = [24, 10, 9]
    bat = loop.serve(max_batch=1, eos_check_interval=8, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False, decode=False,
                     overlap_admission=True, prefill_lanes=1)
    live = bat.submit(None, None, prompt=prompts[0], max_audio_length_ms=80 * limits[0], stream_id=50)
    for _ in range(3):
        assert bat.step()
    victim = bat.submit(None, None, prompt=prompts[1], max_audio_length_ms=80 * limits[1], stream_id=51)
    assert bat.step()
    assert [s.stream_id for s in bat._inflight] == [51] and bat._inflight[0].prefill is not None  # launched in the lane, not committed: the only row is busy
    nxt = bat.submit(None, None, prompt=prompts[2], max_audio_length_ms=80 * limits[2], stream_id=52)
    assert bat.cancel(victim)
    assert bat.step()
    assert victim.cancelled() and [s.stream_id for s in bat._inflight] == [52]  # the lane went to the next head in the same round
    rows = set()
    while bat.step() or bat._queue or bat._inflight:
        rows |= {s.stream_id for s in bat._live()}
    assert rows == {50, 52} and bat.stats["admissions"] == bat.stats["overlapped_admissions"] == 2 and bat.stats["cancelled"] == 1
    for fut, i in ((live, 0), (nxt, 2)):
        got = fut.result(timeout=0)
        want, _ = _solo(loop, prompts[i], limits[i], 50 + i)
        np.testing.assert_array_equal(got.codes.cpu().numpy(), want, err_msg=f"request {i}")
    bat.close()
