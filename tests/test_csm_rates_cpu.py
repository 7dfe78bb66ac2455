"""Other sample rates at both audio edges of `CSMBatcher` (`listen(sample_rate=)`, `submit(..., sample_rate=)`) against a scripted
engine (no device).  The scripted resampler is a sample-and-hold on the real index arithmetic -- output n is input (n M + half) // L, zero
behind the clip -- with `ready` / `out_len` from tests/_resample_ref.py, and it refuses to be asked for an output whose inputs it does not
hold; the scripted encoder records what every row was fed.  Checked: a listener's steps and codes follow from the samples fed and never from
the slicing, the feed limit, that the chunks of a streaming request add up to `out_len`, how `played_samples` at R maps to frames, a
session's heard turn, and that without a rate no resampler is ever made."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _resample_ref as R  # noqa: E402
from test_csm_interrupt_cpu import N_CB, SPF, Engine as _Engine, _batcher, _req, _text  # noqa: E402

from mlx_audio_amd.csm_serve import ListenResult  # noqa: E402
from mlx_audio_amd.sesame import Segment  # noqa: E402

M_FRAMES, MAX_FRAMES, SR = 3, 40, 24000


def _hold(x, L, M, first, last):
    """Outputs [first, last) of the scripted resampler over the clip x."""
    half = R.half_len(L, M)
    return np.array([x[(n * M + half) // L] if (n * M + half) // L < len(x) else 0.0 for n in range(first, last)], np.float32)


def _whole(x, src, dst):
    L, M = R.ratio(src, dst)
    return _hold(np.asarray(x, np.float32), L, M, 0, R.out_len(len(x), L, M))


class Resampler:
    """The surface of `resample.RowResampler`.  A row keeps what it was fed; a step may only be asked for outputs whose inputs are held."""

    def __init__(self, engine, max_rows, max_in):
        self.engine, self.max_rows, self.max_in, self.rows, self.closed = engine, max_rows, max_in, [None] * max_rows, False

    def set_row(self, row, src, dst):
        if row in getattr(self.engine, "fail_set_row", ()):
            raise RuntimeError("scripted set_row failure")
        self.rows[row] = dict(ratio=R.ratio(src, dst), x=[], emitted=0, flushed=False)
        self.engine.calls.append(("rs_set_row", row, src, dst))

    def step(self, x, n_in, flush):
        assert not self.closed and x.shape[0] == self.max_rows and len(n_in) == len(flush) == self.max_rows
        if "rs_step" in self.engine.hooks:  # a caller's thread acts while the step runs (the scheduler holds no lock here)
            self.engine.hooks.pop("rs_step")()
        outs, n_out = [np.zeros(0, np.float32)] * self.max_rows, [0] * self.max_rows
        for r in range(self.max_rows):
            if n_in[r] == 0 and not flush[r]:
                continue
            st = self.rows[r]
            assert st is not None and not st["flushed"] and 0 <= n_in[r] <= self.max_in
            st["x"] += x[r, : n_in[r]].tolist()
            L, M = st["ratio"]
            N = len(st["x"])
            upto = R.out_len(N, L, M) if flush[r] else R.ready(N, L, M)
            assert flush[r] or upto == 0 or ((upto - 1) * M + R.half_len(L, M)) // L < N
            outs[r], n_out[r] = _hold(st["x"], L, M, st["emitted"], upto), upto - st["emitted"]
            st["emitted"], st["flushed"] = upto, bool(flush[r])
        self.engine.calls.append(("rs_step", tuple(n_in), tuple(bool(f) for f in flush)))
        y = torch.zeros((self.max_rows, max(1, max(n_out))), dtype=torch.float32)
        for r in range(self.max_rows):
            y[r, : n_out[r]] = torch.from_numpy(outs[r])
        return y, n_out

    def close(self):
        self.closed = True


class Encoder:
    """The row encoder's surface: a frame's codes are [its first sample, its index + 1]; `fed[row]` is everything the row's stream was fed."""

    def __init__(self, engine, max_batch, max_frames, max_chunk):
        self.engine, self.max_batch, self.max_frames, self.max_chunk = engine, max_batch, max_frames, max_chunk
        self.frames, self.fed, self.calls = [0] * max_batch, [[] for _ in range(max_batch)], []
        self.stepped = threading.Event()

    def reset_row(self, row):
        self.frames[row], self.fed[row] = 0, []

    def step(self, pcm, active):
        assert tuple(pcm.shape[:2]) == (self.max_batch, 1) and pcm.shape[2] % SPF == 0
        if "enc_step" in self.engine.hooks:
            self.engine.hooks.pop("enc_step")()
        F = pcm.shape[2] // SPF
        assert 1 <= F <= self.max_chunk
        codes = torch.zeros((self.max_batch, N_CB, F), dtype=torch.int32)
        rows = tuple(r for r, on in enumerate(active) if on)
        for r in rows:
            x = pcm[r, 0].tolist()
            assert self.frames[r] + F <= self.max_frames
            self.fed[r] += x
            for f in range(F):
                codes[r, 0, f], codes[r, 1, f] = int(x[f * SPF]), self.frames[r] + f + 1
            self.frames[r] += F
        self.calls.append((F, rows))
        self.stepped.set()
        return codes

    def close(self):
        pass


class Engine(_Engine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.resamplers, self.heard = [], []

    def row_encoder(self, max_batch, max_frames, max_chunk):
        self.enc = Encoder(self, max_batch, max_frames, max_chunk)
        return self.enc

    def row_resampler(self, max_rows, max_in):
        self.resamplers.append(Resampler(self, max_rows, max_in))
        return self.resamplers[-1]

    def heard_segment(self, speaker, text, audio):
        self.heard.append(np.asarray(audio))
        return Segment(speaker=speaker, text=text, audio=audio)

    def segment_frames(self, segment, codes=None):
        assert segment.audio is not None and codes is not None
        tf, tm = _text(segment.text)
        T = codes.shape[1]
        af, am = np.zeros((T + 1, N_CB + 1), np.int32), np.zeros((T + 1, N_CB + 1), np.float32)
        af[:T, :N_CB], am[:, :N_CB] = np.asarray(codes).T, 1
        return np.concatenate([tf, af]), np.concatenate([tm, am])


def _listen_batcher(eng, rows=2, **kw):
    return _batcher(eng, listen_rows=rows, listen_chunk_frames=M_FRAMES, listen_max_frames=MAX_FRAMES, **kw)


def _clip(tag, n):
    return (tag * 1000 + 1 + np.arange(n)).astype(np.float32)


def _want(clip, rate):
    """(steps, codes, the padded signal at the model's rate) of a listener fed `clip` at `rate`."""
    y = _whole(clip, rate, SR)
    T = -(-len(y) // SPF)
    pad = np.zeros(T * SPF, np.float32)
    pad[: len(y)] = y
    steps = [M_FRAMES] * (T // M_FRAMES) + ([T % M_FRAMES] if T % M_FRAMES else [])
    return steps, np.array([[int(pad[f * SPF]) for f in range(T)], [f + 1 for f in range(T)]], np.int32), pad


# ---- in: listeners ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n", [(16000, 50), (44100, 120)])
@pytest.mark.parametrize("how", ["at_once", "ones", "sevens", "thread"])
def test_steps_and_codes_do_not_depend_on_the_slicing(rate, n, how):
    eng = Engine()
    bat = _listen_batcher(eng, rows=1)
    lis = bat.listen(sample_rate=rate)
    clip = _clip(3, n)
    if how == "at_once":
        lis.feed(clip)
        bat.run_until_idle()
    elif how in ("ones", "sevens"):
        k = 1 if how == "ones" else 7
        for i in range(0, n, k):
            lis.feed(clip[i : i + k])
            bat.step()
    else:
        t = threading.Thread(target=lambda: [lis.feed(clip[i : i + 5]) for i in range(0, n, 5)])
        t.start()
        t.join()
        bat.run_until_idle()
    L, Mr = R.ratio(rate, SR)
    assert lis.frames == (R.ready(n, L, Mr) // SPF) // M_FRAMES * M_FRAMES  # open: whole rounds of the ready outputs' whole frames
    fut = lis.end()
    bat.run_until_idle()
    res = fut.result(timeout=0)
    steps, codes, pad = _want(clip, rate)
    assert isinstance(res, ListenResult) and res.sample_rate == rate and res.samples == n
    assert res.steps == steps and res.frames == sum(steps) == -(-R.out_len(n, L, Mr) // SPF)
    np.testing.assert_array_equal(res.codes.numpy(), codes)
    assert [c[0] for c in eng.enc.calls] == steps
    np.testing.assert_array_equal(np.array(eng.enc.fed[0], np.float32), pad)  # the encoder saw resample(clip), zero-padded
    assert len(eng.resamplers) == 1 and eng.resamplers[0].rows[0]["flushed"]
    bat.close()
    assert eng.resamplers[0].closed


@pytest.mark.parametrize("when", ["rs_step", "enc_step"])
def test_feed_and_end_from_another_thread_in_the_middle_of_a_round(when):
    """`feed` + `end()` land after the round's resampler step has taken its snapshot -- while that step runs, or while the round's full
    encode step runs -- and before the round plans its tails: the listener has ended but its row holds neither the rest of its samples nor
    the flush.  The round must leave it alone (no early tail step, no early result); the next round finishes it."""
    eng = Engine()
    bat = _listen_batcher(eng, rows=1)
    lis = bat.listen(sample_rate=16000)
    clip = _clip(3, 50)
    futs = []

    def late():
        lis.feed(clip[18:])
        futs.append(lis.end())

    lis.feed(clip[:18])  # ready(18) = 12 samples = 4 frames: one full step of 3 and one frame left, which an early tail step would take
    eng.hooks[when] = late
    assert bat.step()
    assert futs and not futs[0].done() and lis.frames == M_FRAMES and lis.steps == [M_FRAMES] and lis._open
    bat.run_until_idle()
    res = futs[0].result(timeout=0)
    steps, codes, pad = _want(clip, 16000)
    assert res.steps == steps == [3] * 8 + [1] and res.frames == 25 and res.samples == 50
    np.testing.assert_array_equal(res.codes.numpy(), codes)
    np.testing.assert_array_equal(np.array(eng.enc.fed[0], np.float32), pad)
    bat.close()


def test_one_rows_set_row_failure_fails_that_listener_only():
    eng = Engine()
    bat = _listen_batcher(eng, rows=2)
    a, b = bat.listen(sample_rate=16000), bat.listen(sample_rate=8000)
    a.feed(_clip(1, 40)); b.feed(_clip(2, 20))
    eng.fail_set_row = {1}
    fa, fb = a.end(), b.end()
    bat.run_until_idle()
    with pytest.raises(RuntimeError, match="scripted set_row failure"):
        fb.result(timeout=0)
    steps, codes, _ = _want(_clip(1, 40), 16000)
    assert fa.result(timeout=0).steps == steps
    np.testing.assert_array_equal(fa.result(timeout=0).codes.numpy(), codes)
    bat.close()


def test_listeners_at_two_rates_and_the_default_share_the_rounds():
    eng = Engine()
    bat = _listen_batcher(eng, rows=3)
    a, b, c = bat.listen(sample_rate=16000), bat.listen(sample_rate=44100), bat.listen()
    ca, cb, cc = _clip(1, 40), _clip(2, 100), _clip(4, 7 * SPF)
    a.feed(ca); b.feed(cb); c.feed(cc)
    assert bat.step()
    assert _marks_of(eng, "rs_step") == [("rs_step", (40, 100, 0), (False, False, False))]  # one resampler step for both rate rows
    fa, fb, fc = a.end(), b.end(), c.end()
    bat.run_until_idle()
    for fut, clip, rate in ((fa, ca, 16000), (fb, cb, 44100)):
        steps, codes, _ = _want(clip, rate)
        assert fut.result(timeout=0).steps == steps
        np.testing.assert_array_equal(fut.result(timeout=0).codes.numpy(), codes)
    rc = fc.result(timeout=0)
    assert rc.sample_rate == SR and rc.frames == 7 and rc.samples == 7 * SPF and rc.codes[0].tolist() == [4001 + f * SPF for f in range(7)]
    assert _marks_of(eng, "rs_step")[1:] == [("rs_step", (0, 0, 0), (True, True, False))]  # the flush of both, no new samples
    bat.close()


def _marks_of(eng, *kinds):
    return [c for c in eng.calls if c[0] in kinds]


def test_the_feed_limit_counts_samples_at_the_models_rate():
    eng = Engine()
    bat = _listen_batcher(eng)
    cap = MAX_FRAMES * SPF
    up, down = bat.listen(sample_rate=8000), bat.listen(sample_rate=48000)
    up.feed(_clip(1, cap // 3))  # out_len = cap exactly
    with pytest.raises(ValueError, match="listen_max_frames"):
        up.feed(_clip(1, 1))
    assert up.samples == cap // 3
    down.feed(_clip(2, 2 * cap - 1))
    down.feed(_clip(2, 1))       # out_len(2 cap) = cap
    with pytest.raises(ValueError, match="listen_max_frames"):
        down.feed(_clip(2, 1))
    assert down.samples == 2 * cap
    fu = up.end()
    bat.run_until_idle()
    assert fu.result(timeout=0).frames == MAX_FRAMES
    for bad in (24001, 7, 0, -8000):
        with pytest.raises(ValueError):
            bat.listen(sample_rate=bad)
    with pytest.raises(ValueError):
        bat.submit(None, [3, 3, 1], voice_match=False, sample_rate=24001)
    bat.close()


def test_a_sessions_heard_turn_enters_as_the_resampled_signal():
    eng = Engine()
    bat = _listen_batcher(eng)
    sess = bat.session()
    lis = sess.listen(speaker=1, sample_rate=16000)
    clip = _clip(1, 33)
    for i in range(0, 33, 4):
        lis.feed(clip[i : i + 4])
        bat.step()
    fut = lis.end([9, 9])
    bat.run_until_idle()
    res = fut.result(timeout=0)
    steps, codes, pad = _want(clip, 16000)
    np.testing.assert_array_equal(res.codes.numpy(), codes)
    np.testing.assert_array_equal(eng.heard[-1], _whole(clip, 16000, SR))  # Segment.audio: the signal at the model's rate, not padded
    eng2 = Engine()
    twin = _listen_batcher(eng2).session()
    twin.hear(Segment(1, [9, 9], _whole(clip, 16000, SR)), codes=codes)
    assert twin.turns == sess.turns and twin.length == sess.length
    for x, y in zip(sess.pending + sess.history, twin.pending + twin.history):
        np.testing.assert_array_equal(x, y)
    bat.close()


# ---- out: requests ---------------------------------------------------------------------------------------------------------------------------
def _audio24(tag, frames):
    """What the scripted codec gives for the stream `tag`: SPF samples of tag + i + 1 per frame i."""
    return np.repeat(np.array([tag + i + 1 for i in range(frames)], np.float32), SPF)


@pytest.mark.parametrize("rate", [8000, 48000, 44100])
@pytest.mark.parametrize("frames", [7, 9])  # a remainder chunk; a length that is a multiple of the chunk
def test_chunk_lengths_sum_to_out_len_and_concatenate_to_the_whole(rate, frames):
    eng = Engine()
    bat = _batcher(eng, stream_chunk_frames=3)
    st = bat.submit_stream(None, [3, 3, 5], max_audio_length_ms=80 * frames, voice_match=False, sample_rate=rate)
    other = _req(bat, 2, 5, stream=True)  # a row without a rate in the same decode rounds
    bat.run_until_idle()
    chunks = list(st)
    res = st.result(timeout=0)
    L, Mr = R.ratio(SR, rate)
    assert [c.frames for c in chunks] == [3] * (frames // 3) + ([frames % 3] if frames % 3 else []) and chunks[-1].final
    assert sum(c.audio.shape[0] for c in chunks) == R.out_len(frames * SPF, L, Mr) == res.audio.shape[0]
    assert res.sample_rate == rate and res.frames == frames
    want = _whole(_audio24(5, frames), SR, rate)
    np.testing.assert_array_equal(torch.cat([c.audio for c in chunks]).numpy(), want)
    np.testing.assert_array_equal(res.audio.numpy(), want)
    ro = other.result(timeout=0)
    assert ro.sample_rate == SR and ro.audio.shape[0] == 5 * SPF
    assert _marks_of(eng, "rs_set_row") == [("rs_set_row", 0, SR, rate)]
    assert len(eng.resamplers) == 1 and eng.resamplers[0].max_rows == 2 and eng.resamplers[0].max_in == 3 * SPF
    bat.close()


def test_a_plain_request_is_resampled_as_a_whole():
    eng = Engine()
    bat = _batcher(eng)
    fut = bat.submit(None, [3, 3, 5], max_audio_length_ms=80 * 6, voice_match=False, sample_rate=48000)
    same = bat.submit(None, [3, 3, 6], max_audio_length_ms=80 * 6, voice_match=False, sample_rate=SR)  # the model's rate: today's path
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert res.sample_rate == 48000 and res.frames == 6
    np.testing.assert_array_equal(res.audio.numpy(), _whole(_audio24(5, 6), SR, 48000))
    assert same.result(timeout=0).sample_rate == SR and same.result(timeout=0).audio.shape[0] == 6 * SPF
    # one whole-clip step with the flush on a one-row resampler the batcher keeps
    assert len(eng.resamplers) == 1 and (eng.resamplers[0].max_rows, eng.resamplers[0].max_in) == (1, 1 << 30)
    assert _marks_of(eng, "rs_set_row", "rs_step") == [("rs_set_row", 0, SR, 48000), ("rs_step", (6 * SPF,), (True,))]
    with pytest.raises(ValueError, match="decode=False"):
        _batcher(Engine(), decode=False).submit(None, [3, 3, 5], voice_match=False, sample_rate=8000)
    bat.close()


@pytest.mark.parametrize("rate,played,kept", [(48000, 14, 3), (48000, 12, 2), (8000, 2, 2), (8000, 3, 3), (None, 14, 5)])
def test_played_samples_count_at_the_requests_rate(rate, played, kept):
    """p samples at R are p * 24000 // R of the codec's; a frame that was partly played counts (SPF = 3 codec samples per frame)."""
    eng = Engine()
    bat = _batcher(eng)
    fut = bat.submit(None, [3, 3, 1], max_audio_length_ms=80 * 30, voice_match=False, sample_rate=rate)
    for _ in range(8):
        assert bat.step()
    assert bat.interrupt(fut, played_samples=played)
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert res.interrupted and res.frames == kept and res.sample_rate == (rate or SR)
    want = _audio24(1, kept) if rate is None else _whole(_audio24(1, kept), SR, rate)
    np.testing.assert_array_equal(res.audio.numpy(), want)  # the resample of the 24 kHz audio that was kept
    bat.close()


def test_an_interrupted_streaming_request_at_a_rate():
    eng = Engine()
    bat = _batcher(eng, stream_chunk_frames=3)
    st = bat.submit_stream(None, [3, 3, 1], max_audio_length_ms=80 * 40, voice_match=False, sample_rate=48000)
    for _ in range(6):
        assert bat.step()
    assert (len(bat._rows[0].codes), bat._rows[0].emitted) == (7, 3)
    assert st.interrupt(played_samples=2 * (3 * SPF + 1))  # 3 frames and one sample of the fourth, counted at 48 kHz
    bat.run_until_idle()
    got = list(st)
    assert [(c.first_frame, c.frames, c.final) for c in got] == [(0, 3, False), (3, 1, True)]
    res = st.result(timeout=0)
    want = _whole(_audio24(1, 4), SR, 48000)
    assert res.interrupted and res.frames == 4 and res.sample_rate == 48000
    np.testing.assert_array_equal(torch.cat([c.audio for c in got]).numpy(), want)  # the last chunk flushed: the chunks are the whole
    np.testing.assert_array_equal(res.audio.numpy(), want)
    # cut inside what was already emitted: the result is the resample of the kept audio, the iterator ends behind an empty chunk
    st2 = bat.submit_stream(None, [3, 3, 2], max_audio_length_ms=80 * 40, voice_match=False, sample_rate=8000)
    for _ in range(6):
        assert bat.step()
    assert bat._rows[0].emitted == 3 and st2.interrupt(played_frames=2)
    bat.run_until_idle()
    got2 = list(st2)
    assert [(c.frames, c.final) for c in got2] == [(3, False), (0, True)] and got2[-1].audio.shape[0] == 0
    r2 = st2.result(timeout=0)
    assert r2.frames == 2 and r2.sample_rate == 8000
    np.testing.assert_array_equal(r2.audio.numpy(), _whole(_audio24(2, 2), SR, 8000))
    # cut exactly where the emitted chunks end: the row is flushed and the chunk of 0 frames carries the filter's tail
    st3 = bat.submit_stream(None, [3, 3, 4], max_audio_length_ms=80 * 40, voice_match=False, sample_rate=16000)
    for _ in range(6):
        assert bat.step()
    assert bat._rows[0].emitted == 3 and st3.interrupt(played_frames=3)
    bat.run_until_idle()
    got3 = list(st3)
    assert [(c.frames, c.final) for c in got3] == [(3, False), (0, True)] and got3[-1].audio.shape[0] > 0
    want3 = _whole(_audio24(4, 3), SR, 16000)
    np.testing.assert_array_equal(torch.cat([c.audio for c in got3]).numpy(), want3)
    np.testing.assert_array_equal(st3.result(timeout=0).audio.numpy(), want3)
    bat.close()


# ---- no rate: nothing changes ----------------------------------------------------------------------------------------------------------------
def test_without_a_rate_no_resampler_is_ever_made():
    eng = Engine()
    bat = _listen_batcher(eng, stream_chunk_frames=3)
    lis = bat.listen()
    st = _req(bat, 1, 7, stream=True)
    plain = _req(bat, 2, 4)
    lis.feed(_clip(1, 5 * SPF + 1))
    fut = lis.end()
    bat.run_until_idle()
    assert fut.result(timeout=0).sample_rate == SR and fut.result(timeout=0).frames == 6
    assert st.result(timeout=0).sample_rate == SR and plain.result(timeout=0).sample_rate == SR
    assert bat.interrupt(plain) is False
    assert not eng.resamplers and not _marks_of(eng, "rs_step", "rs_set_row")
    assert bat._lrs is None and bat._ors is None and bat._crs is None and bat._heard is None
    bat.close()
