"""Streaming audio out of csm_serve.CSMBatcher (`stream_chunk_frames=N`, `submit_stream`) against a scripted engine and a scripted row
decoder (no device): which chunks a request gets, when a chunk may be decoded, how rows are reset and reused, and how a failure ends the
iterator.  The scripted decoder enforces the row decoder's rules -- a row is fed ITS OWN frames, in order, from frame 0 after a reset, never an
EOS frame -- so a scheduling mistake fails loudly here."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mlx_audio_amd.csm_serve import AudioChunk, CSMBatcher  # noqa: E402
from mlx_audio_amd.sesame import make_sampler  # noqa: E402
from test_csm_serve_cpu import FakeEngine  # noqa: E402

SPF = 3


class FakeRowDecoder:
    """pcm of a frame = the sum of its codes, SPF samples per frame (what FakeEngine.decode gives offline).  Frame i of stream `tag` is
    [tag, i + 1], so the frames a row is fed say which stream and which position they belong to."""

    def __init__(self, engine, max_batch, max_frames, max_chunk, fail_at=None):
        self.engine, self.max_batch, self.max_frames, self.max_chunk, self.fail_at = engine, max_batch, max_frames, max_chunk, fail_at
        self.frames = [0] * max_batch
        self.steps = 0
        self.closed = False

    def reset_row(self, row):
        self.engine.calls.append(("reset_row", row))
        self.frames[row] = 0

    def row_frames(self, row):
        return self.frames[row]

    def step(self, codes, active):
        assert not self.closed
        B, n_cb, F = codes.shape
        assert B == self.max_batch and len(active) == B and 1 <= F <= self.max_chunk
        self.steps += 1
        if self.fail_at is not None and self.steps >= self.fail_at:
            raise RuntimeError("scripted decoder failure")
        fed = {}
        for r in range(B):
            if not active[r]:
                continue
            tag = int(codes[r, 0, 0])
            assert tag != 0, "an EOS frame was handed to the codec"
            assert codes[r, 0].tolist() == [tag] * F and codes[r, 1].tolist() == list(range(self.frames[r] + 1, self.frames[r] + F + 1)), \
                "a row was not fed its own next frames"
            assert self.frames[r] + F <= self.engine.polled.get(tag, 0), "frames were decoded before a poll confirmed them"
            assert self.frames[r] + F <= self.max_frames
            fed[r] = (tag, self.frames[r], F)
            self.frames[r] += F
        self.engine.calls.append(("step", F, fed))
        return codes.to(torch.float32).sum(dim=1).repeat_interleave(SPF, dim=1)[:, None, :]

    def close(self):
        self.closed = True


class StreamEngine(FakeEngine):
    def __init__(self, fail_at=None, **kw):
        super().__init__(**kw)
        self.fail_at = fail_at
        self.polled = {}  # tag -> frames the last poll has seen of that stream

    def row_decoder(self, max_batch, max_frames, max_chunk):
        self.dec = FakeRowDecoder(self, max_batch, max_frames, max_chunk, self.fail_at)
        return self.dec


def _batcher(engine, N, **kw):
    bat = CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=engine, rng="host", stream_chunk_frames=N, **kw)
    poll = bat._poll

    def recording_poll():  # what a poll can have confirmed: the frames generated so far, below the EOS frame
        for s in bat._live():
            tag = int(s.text[0])
            eos = engine.eos.get(tag)
            engine.polled[tag] = min(len(s.codes), eos if eos is not None and eos < len(s.codes) else len(s.codes), s.max_frames)
        engine.calls.append(("poll",))
        poll()

    bat._poll = recording_poll
    return bat


def _stream(bat, tag, length, frames):
    return bat.submit_stream(None, [tag] * length, max_audio_length_ms=80 * frames)


def _expected_audio(tag, first, frames):
    return torch.tensor([float(tag + i + 1) for i in range(first, first + frames)]).repeat_interleave(SPF)


@pytest.mark.parametrize("frames", [1, 3, 4, 8, 10, 13])
def test_chunk_boundaries_and_final_flags(frames):
    """N = 4: chunk k is frames [4k, 4k + 4), the last chunk the remainder; a length that is a multiple of N ends on a full final chunk."""
    N = 4
    eng = StreamEngine()
    bat = _batcher(eng, N, max_batch=2)
    st = _stream(bat, 5, 3, frames)
    bat.run_until_idle()
    chunks = list(st)
    want = [(k * N, min(N, frames - k * N)) for k in range((frames + N - 1) // N)]
    assert all(isinstance(c, AudioChunk) for c in chunks)
    assert [(c.first_frame, c.frames) for c in chunks] == want
    assert [c.final for c in chunks] == [False] * (len(want) - 1) + [True]
    for c in chunks:
        assert torch.equal(c.audio, _expected_audio(5, c.first_frame, c.frames))
    res = st.result(timeout=0)
    assert res.frames == frames and res.codes.T.tolist() == [[5, i + 1] for i in range(frames)]
    assert torch.equal(res.audio, torch.cat([c.audio for c in chunks])) and res.audio.shape == (SPF * frames,)
    assert [c[1] for c in eng.calls if c[0] == "step"] == [n for _, n in want]  # the decoder saw the step sizes N, ..., r
    assert bat.stats["chunks"] == len(want) and st.first_audio_seconds is not None


def test_eos_in_the_middle_of_a_chunk_emits_nothing_at_or_after_it():
    eng = StreamEngine(eos={1: 6, 2: 4, 3: 0})
    bat = _batcher(eng, 4, max_batch=3)
    a, b, c = _stream(bat, 1, 3, 40), _stream(bat, 2, 3, 40), _stream(bat, 3, 3, 40)
    bat.run_until_idle()
    ca, cb = list(a), list(b)
    assert [(x.first_frame, x.frames, x.final) for x in ca] == [(0, 4, False), (4, 2, True)]
    assert [(x.first_frame, x.frames, x.final) for x in cb] == [(0, 4, True)]  # EOS at a chunk boundary: the full chunk is the final one
    assert a.result(timeout=0).frames == 6 and b.result(timeout=0).frames == 4
    assert a.result(timeout=0).audio.shape == (SPF * 6,)
    with pytest.raises(AssertionError, match="No audio generated"):  # EOS as the very first frame: no chunk, the iterator raises
        list(c)
    assert sum(n for call in eng.calls if call[0] == "step" for (_, _, n) in call[2].values()) == 10  # 6 + 4 frames reached the codec, no more


def test_a_ready_chunk_waits_for_the_poll_that_confirms_it():
    """One stream, N = 4.  After the admission and three frames the stream holds its first four frames, but no poll has run: nothing is
    decoded.  The poll comes after N single-token frames and finds five frames: chunk 0 is confirmed (and known not to be the last)."""
    eng = StreamEngine()
    bat = _batcher(eng, 4, max_batch=1)
    st = _stream(bat, 1, 3, 20)
    for _ in range(4):
        assert bat.step()
    assert len(bat._rows[0].codes) == 5 and bat.stats["polls"] == 0
    assert not [c for c in eng.calls if c[0] == "step"] and st._q.empty()
    bat.step()
    kinds = [c[0] for c in eng.calls if c[0] in ("poll", "step")]
    assert kinds == ["poll", "step"] and st._q.qsize() == 1
    first = st._q.queue[0]
    assert (first.first_frame, first.frames, first.final) == (0, 4, False)
    bat.run_until_idle()
    # every decode in the whole run came right behind a poll (the scripted decoder checked each against what that poll had seen)
    for i, c in enumerate(eng.calls):
        if c[0] == "step":
            j = i
            while eng.calls[j][0] in ("step", "park"):
                j -= 1
            assert eng.calls[j][0] == "poll"
    assert [(c.first_frame, c.frames) for c in st] == [(0, 4), (4, 4), (8, 4), (12, 4), (16, 4)]


def test_streaming_and_plain_requests_share_a_batch_and_rounds_are_grouped():
    eng = StreamEngine()
    bat = _batcher(eng, 4, max_batch=3)
    s1, plain, s2 = _stream(bat, 1, 3, 10), bat.submit(None, [2] * 4, max_audio_length_ms=80 * 9), _stream(bat, 3, 5, 14)
    bat.run_until_idle()
    assert any(c[0] == "frame" and set(c[2]) == {1, 2, 3} for c in eng.calls)  # all three in one frame step
    p = plain.result(timeout=0)
    assert p.frames == 9 and torch.equal(p.audio, _expected_audio(2, 0, 9))  # the offline decode, as before
    for st, tag, f in ((s1, 1, 10), (s2, 3, 14)):
        chunks = list(st)
        assert sum(c.frames for c in chunks) == f and chunks[-1].final
        assert torch.equal(st.result(timeout=0).audio, _expected_audio(tag, 0, f))
    steps = [c for c in eng.calls if c[0] == "step"]
    assert any(len(c[2]) == 2 for c in steps)  # rows whose chunk is ready at the same poll are decoded together
    assert all(len({n for (_, _, n) in c[2].values()}) == 1 for c in steps)
    assert not [c for c in eng.calls if c[0] == "reset_row" and c[1] == p.row]  # the plain request's row was never the codec's business


def test_row_reuse_resets_the_decoder_row_before_the_new_streams_first_step():
    eng = StreamEngine()
    bat = _batcher(eng, 4, max_batch=1)
    a, b = _stream(bat, 1, 3, 6), _stream(bat, 2, 3, 5)
    bat.run_until_idle()
    assert a.result(timeout=0).row == b.result(timeout=0).row == 0
    row0 = [(c[0], c[2][0][0] if c[0] == "step" else None) for c in eng.calls if c[0] == "reset_row" or (c[0] == "step" and 0 in c[2])]
    assert row0 == [("reset_row", None), ("step", 1), ("step", 1), ("reset_row", None), ("step", 2), ("step", 2)]
    admits = [i for i, c in enumerate(eng.calls) if c[0] == "admit"]
    resets = [i for i, c in enumerate(eng.calls) if c[0] == "reset_row"]
    assert len(admits) == len(resets) == 2 and all(r == a_ + 1 for a_, r in zip(admits, resets))  # at admission
    assert [c.frames for c in b] == [4, 1]


def test_a_failing_decode_ends_the_iterator_with_the_error_and_spares_the_others():
    eng = StreamEngine(fail_at=2)
    bat = _batcher(eng, 4, max_batch=2)
    st, plain = _stream(bat, 1, 3, 12), bat.submit(None, [2] * 4, max_audio_length_ms=80 * 9)
    bat.run_until_idle()
    got = []
    with pytest.raises(RuntimeError, match="scripted decoder failure"):
        for c in st:
            got.append(c)
    assert [(c.first_frame, c.frames, c.final) for c in got] == [(0, 4, False)]
    with pytest.raises(RuntimeError, match="scripted decoder failure"):
        st.result(timeout=0)
    assert plain.result(timeout=0).frames == 9
    assert eng.pad == [eng.max_pos] * 2  # the failed stream's row was parked


def test_close_ends_the_iterator_by_raising_never_by_hanging():
    eng = StreamEngine()
    bat = _batcher(eng, 4, max_batch=2)
    live, queued_ = _stream(bat, 1, 3, 40), None
    for _ in range(6):
        bat.step()
    bat2 = [_stream(bat, t, 3, 40) for t in (2, 3)]  # one more live, one still queued
    bat.step()
    queued_ = bat2[1]
    bat.close()
    assert eng.dec.closed
    got = []
    with pytest.raises(RuntimeError, match="closed"):
        for c in live:
            got.append(c)
    assert [(c.first_frame, c.final) for c in got] == [(0, False)]
    for st in bat2:
        with pytest.raises(RuntimeError, match="closed"):
            list(st)
    late = _stream(bat, 4, 3, 4)
    with pytest.raises(RuntimeError, match="closed"):
        list(late)
    assert queued_.future.done()


def test_background_thread_delivers_chunks_to_a_waiting_consumer():
    eng = StreamEngine()
    bat = _batcher(eng, 4, max_batch=2).start()
    try:
        st = _stream(bat, 1, 3, 10)
        chunks = list(st)  # blocks on the queue until the scheduler thread has produced the final chunk
        assert [(c.first_frame, c.frames, c.final) for c in chunks] == [(0, 4, False), (4, 4, False), (8, 2, True)]
        assert torch.equal(st.result(timeout=30).audio, torch.cat([c.audio for c in chunks]))
    finally:
        bat.close()


def test_refusals_at_submit():
    eng = StreamEngine()
    plain = CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=eng, rng="host")
    with pytest.raises(ValueError, match="stream_chunk_frames"):
        plain.submit_stream(None, [1] * 3, max_audio_length_ms=800)
    bat = _batcher(StreamEngine(), 4, max_batch=2, stream_max_frames=20)
    with pytest.raises(ValueError, match="stream_max_frames"):
        _stream(bat, 1, 3, 21)
    with pytest.raises(ValueError, match="Inputs too long"):
        _stream(bat, 1, 50, 20)
    _stream(bat, 1, 3, 20)
    with pytest.raises(ValueError):
        CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=StreamEngine(), stream_chunk_frames=0)
    with pytest.raises(ValueError):
        CSMBatcher(None, sampler=make_sampler(temp=0.0), engine=StreamEngine(), stream_chunk_frames=4, decode=False)
