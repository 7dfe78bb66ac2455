"""Live listening on a running CSM batch (csm_serve.CSMBatcher with listen_rows=K, `listen()` / `CSMSession.listen()`, Mimi.row_encoder): a
listener's codes equal a fresh batch-1 `Mimi.encode_step` stream over its zero-padded pcm in the steps [M] * (T // M) + [T % M], whatever the
slicing of its `feed` calls and whatever else listens or is generated; a generating request keeps the bits of its own `generate_batch` run;
a session's turn after a listened turn equals the turn of a twin session that did `hear(segment, codes=those codes)`.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from test_gpu_csm_serve import SEED, _check, _loop, _request, _sampler, _submit  # noqa: E402

pytestmark = pytest.mark.gpu

M, SPF, MAX_FRAMES = 3, 1920, 48


def _pcm(g, samples):
    return (0.3 * g.standard_normal(samples)).astype(np.float32)


def _steps(samples):
    T = -(-samples // SPF)
    return [M] * (T // M) + ([T % M] if T % M else [])


def _solo_codes(mimi, pcm):
    """A fresh batch-1 Mimi.encode_step stream over the zero-padded clip in the steps [M] * q + [r] -> codes [n_cb, T] (numpy)."""
    steps = _steps(pcm.shape[0])
    x = np.zeros(sum(steps) * SPF, np.float32)
    x[: pcm.shape[0]] = pcm
    mimi.close_stream()
    out, i = [], 0
    for F in steps:
        out.append(mimi.encode_step(torch.tensor(x[None, None, i * SPF : (i + F) * SPF]), max_chunk=M, max_frames=MAX_FRAMES)[0].cpu().numpy())
        i += F
    mimi.close_stream()
    return np.concatenate(out, -1)


def _drive(bat, fut):
    for _ in range(600):
        if fut.done():
            return
        bat.step()
    raise AssertionError("the request did not finish")


def _serve(loop, **kw):
    kw.setdefault("listen_rows", 2)
    return loop.serve(rng="device", sampler=_sampler(), seed=SEED, listen_chunk_frames=M, listen_max_frames=MAX_FRAMES, **kw)


def _listened(res, mimi, pcm):
    want = _solo_codes(mimi, pcm)
    assert res.steps == _steps(pcm.shape[0]) and res.frames == want.shape[1] and res.samples == pcm.shape[0]
    np.testing.assert_array_equal(res.codes.cpu().numpy(), want)
    return want


def test_two_listeners_with_different_slicings_beside_a_generating_request():
    loop = _loop("float32")
    g = np.random.default_rng(61)
    req = _request(g, 0, 5, 2, 4)
    a_pcm, b_pcm = _pcm(g, 7 * SPF), _pcm(g, 5 * SPF - 333)  # T = 7 (r = 1) in slices of 700; T = 5 (r = 2), one feed, a partial last frame
    bat = _serve(loop, max_batch=2)
    fut = _submit(bat, "device", 0, req, 10)
    a, b = bat.listen(), bat.listen(speaker=1)
    b.feed(b_pcm)
    for i in range(0, a_pcm.shape[0], 700):
        a.feed(a_pcm[i : i + 700])
        bat.step()
    assert a.frames >= M and tuple(a.codes().shape) == (loop.n_cb, a.frames)
    fa, fb = a.end(), b.end()
    _drive(bat, fa); _drive(bat, fb); _drive(bat, fut)
    mimi = loop._audio_tokenizer
    _listened(fa.result(timeout=0), mimi, a_pcm)
    _listened(fb.result(timeout=0), mimi, b_pcm)
    assert bat.stats["listen_frames"] == 12 and bat.stats["listen_rounds"] >= 4
    _check(loop, "device", [req], [10], [fut])  # the generating request: codes and waveform of its solo run, bit for bit
    bat.close()


def test_a_listened_turn_equals_a_hear_twin():
    from mlx_audio_amd.sesame import Segment

    loop = _loop("float32")
    g = np.random.default_rng(62)
    pcm = _pcm(g, 4 * SPF + 500)
    heard, said = g.integers(0, 300, 3).tolist(), g.integers(0, 300, 4).tolist()
    bat = _serve(loop, max_batch=2, listen_rows=1, stop_on_eos=False)
    sess = bat.session()
    lis = sess.listen(1)
    for i in range(0, pcm.shape[0], 2500):
        lis.feed(pcm[i : i + 2500])
    f = lis.end(heard)
    assert sess.busy
    bat.run_until_idle()
    codes = _listened(f.result(timeout=0), loop._audio_tokenizer, pcm)
    assert not sess.busy
    turn = sess.submit(said, max_audio_length_ms=80 * 6, stream_id=60)
    _drive(bat, turn)
    twin_bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False)
    twin = twin_bat.session()
    twin.hear(Segment(speaker=1, text=heard, audio=pcm), codes=codes)
    assert twin.turns == sess.turns[:1]
    turn2 = twin.submit(said, max_audio_length_ms=80 * 6, stream_id=60)
    _drive(twin_bat, turn2)
    r, r2 = turn.result(timeout=0), turn2.result(timeout=0)
    assert r.frames == r2.frames == 6
    np.testing.assert_array_equal(r.codes.cpu().numpy(), r2.codes.cpu().numpy())
    assert torch.equal(r.audio, r2.audio)
    assert sess.turns == twin.turns and sess.length == twin.length and sess.n == twin.n
    for x, y in zip(sess.history + sess.pending, twin.history + twin.pending):
        np.testing.assert_array_equal(x, y)
    sess.close(); twin.close(); bat.close(); twin_bat.close()


def test_barge_in_listen_while_the_turn_is_live_then_interrupt_and_end():
    from mlx_audio_amd.sesame import Segment

    loop = _loop("float32")
    g = np.random.default_rng(63)
    pcm = _pcm(g, 5 * SPF - 100)
    said, heard, said2 = (g.integers(0, 300, n).tolist() for n in (4, 3, 3))
    kw = dict(max_batch=1, stop_on_eos=False, stream_chunk_frames=2, stream_max_frames=32)
    bat = _serve(loop, listen_rows=1, **kw)
    sess = bat.session()
    st = sess.submit_stream(said, max_audio_length_ms=80 * 30, stream_id=50)
    for _ in range(4):
        assert bat.step()
    lis = sess.listen(1)  # the user speaks while the agent speaks
    lis.feed(pcm[: 3 * SPF + 7])
    assert bat.step() and lis.frames == M and not st.future.done()
    with pytest.raises(ValueError, match="queued or live"):
        lis.end(heard)
    lis.feed(pcm[3 * SPF + 7 :])  # the listener stays usable
    assert sess.interrupt(played_frames=2)
    _drive(bat, st.future)
    r1 = st.result(timeout=0)
    assert r1.frames == 2 and r1.interrupted
    f = lis.end(heard)
    _drive(bat, f)
    codes = _listened(f.result(timeout=0), loop._audio_tokenizer, pcm)
    nxt = sess.submit(said2, max_audio_length_ms=80 * 5, stream_id=51)
    _drive(bat, nxt)
    # the twin: a turn with a limit of 2 frames, hear(codes=...), the next turn
    twin_bat = loop.serve(rng="device", sampler=_sampler(), seed=SEED, **kw)
    twin = twin_bat.session()
    t1 = twin.submit_stream(said, max_audio_length_ms=80 * 2, stream_id=50)
    _drive(twin_bat, t1.future)
    twin.hear(Segment(speaker=1, text=heard, audio=pcm), codes=codes)
    nxt2 = twin.submit(said2, max_audio_length_ms=80 * 5, stream_id=51)
    _drive(twin_bat, nxt2)
    np.testing.assert_array_equal(r1.codes.cpu().numpy(), t1.result(timeout=0).codes.cpu().numpy())
    assert torch.equal(r1.audio, t1.result(timeout=0).audio)
    a, b = nxt.result(timeout=0), nxt2.result(timeout=0)
    assert a.frames == b.frames == 5
    np.testing.assert_array_equal(a.codes.cpu().numpy(), b.codes.cpu().numpy())
    assert torch.equal(a.audio, b.audio)
    assert sess.turns == twin.turns and sess.length == twin.length and sess.n == twin.n
    for x, y in zip(sess.history + sess.pending, twin.history + twin.pending):
        np.testing.assert_array_equal(x, y)
    sess.close(); twin.close(); bat.close(); twin_bat.close()


def test_capacity_and_lifecycle():
    loop = _loop("float32")
    g = np.random.default_rng(64)
    bat = _serve(loop, max_batch=1, listen_rows=2)
    a, b = bat.listen(), bat.listen()
    with pytest.raises(ValueError, match="taken"):
        bat.listen()
    a.feed(_pcm(g, 4 * SPF))
    assert bat.step() and a.frames == M  # row 0 holds a stream's state
    assert a.cancel()
    c = bat.listen()  # the freed row: reset before its first step
    assert c.row == 0
    pcm = _pcm(g, 4 * SPF + 1)
    c.feed(pcm)
    with pytest.raises(ValueError, match="listen_max_frames"):
        c.feed(np.zeros((MAX_FRAMES - 4) * SPF, np.float32))
    assert c.samples == pcm.shape[0]
    fc = c.end()
    bat.run_until_idle()
    _listened(fc.result(timeout=0), loop._audio_tokenizer, pcm)
    b.feed(_pcm(g, SPF))
    fb = b.end()
    bat.close()
    with pytest.raises(RuntimeError, match="closed"):
        fb.result(timeout=0)
    plain = loop.serve(max_batch=1, rng="device", sampler=_sampler(), seed=SEED)
    with pytest.raises(ValueError, match="listen_rows"):
        plain.listen()
    plain.close()
