"""Streaming audio out of a running CSM batch (csm_serve.CSMBatcher with stream_chunk_frames=N, submit_stream, Mimi.row_decoder): requests of
different lengths, admitted at different times, into reused rows, beside a plain request.  Every stream's codes are those of its own
`generate_batch([prompt])` run, its chunks concatenate to -- bit for bit -- a batch-1 `Mimi.decode_step` stream over those codes in steps
of N, ..., r, and a plain `submit` in the same batch still gets the offline `Mimi.decode` bits.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from test_gpu_csm_serve import SEED, _loop, _request, _sampler, _solo  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4


def _solo_stream(mimi, codes, steps):
    """a fresh batch-1 Mimi.decode_step stream over codes [n_cb, T] in the given step sizes -> [T * spf]"""
    mimi.close_stream()
    out, i = [], 0
    for F in steps:
        out.append(mimi.decode_step(codes[None, :, i : i + F], max_chunk=max(steps), max_frames=64)[0, 0].clone())
        i += F
    mimi.close_stream()
    return torch.cat(out)


@pytest.mark.parametrize("rng", ["host", "device"])
def test_chunks_of_a_running_batch_equal_solo_decode_step_streams(rng):
    loop = _loop("float32")
    g = np.random.default_rng(15)
    reqs = [_request(g, 0, 5, 3, 4), _request(g, 1, 5, 1, 6, voice_match=True), _request(g, 2, 4, 2, 3), _request(g, 3, 3, 2, 2),
            _request(g, 4, 4, 1, 3)]
    frames = [14, 9, 11, 6, 4]      # kN + r, kN + r, (plain), reused row, exactly N
    streaming = [True, True, False, True, True]
    bat = loop.serve(max_batch=3, rng=rng, sampler=_sampler(), seed=SEED, stream_chunk_frames=N, stream_max_frames=32)

    def submit(i):
        fn = bat.submit_stream if streaming[i] else bat.submit
        return fn(max_audio_length_ms=80 * frames[i], seed=(100 + i) if rng == "host" else None, stream_id=50 + i, **reqs[i])

    handles = {0: submit(0), 1: submit(1)}
    for _ in range(3):
        assert bat.step()
    handles[2] = submit(2)  # admitted beside two running streams, at another phase of the chunk cadence
    for _ in range(2):
        assert bat.step()
    handles[3], handles[4] = submit(3), submit(4)  # queued: they reuse the rows of the streams that end first
    bat.run_until_idle()
    assert bat.stats["admissions"] == 5 and bat.stats["chunks"] >= 4
    rows = [handles[i].result(timeout=0).row for i in range(5)]
    assert len(set(rows)) < 5  # rows were reused
    mimi = loop._audio_tokenizer
    for i in range(5):
        if not streaming[i]:
            continue
        res = handles[i].result(timeout=0)
        ref = _solo(loop, reqs[i], frames[i], rng, 100 + i, 50 + i)
        n = int(ref.frames[0])
        assert res.frames == n, i
        np.testing.assert_array_equal(res.codes.cpu().numpy(), ref.codes[0][:, :n].cpu().numpy(), err_msg=f"stream {i}")
        chunks = list(handles[i])
        steps = [N] * (n // N) + ([n % N] if n % N else [])
        assert [(c.first_frame, c.frames) for c in chunks] == [(sum(steps[:k]), steps[k]) for k in range(len(steps))], i
        assert [c.final for c in chunks] == [False] * (len(steps) - 1) + [True], i
        cat = torch.cat([c.audio for c in chunks])
        want = _solo_stream(mimi, ref.codes[0][:, :n], steps)
        assert torch.equal(cat, want), f"stream {i}: chunks differ from the solo decode_step stream"
        assert torch.equal(res.audio, cat), i
        assert handles[i].first_audio_seconds is not None
    # the plain request: frames, codes and the OFFLINE decode's waveform, as without streaming
    got = handles[2].result(timeout=0)
    ref = _solo(loop, reqs[2], frames[2], rng, 102, 52)
    assert got.frames == ref.frames[0]
    np.testing.assert_array_equal(got.codes.cpu().numpy(), ref.codes[0][:, : ref.frames[0]].cpu().numpy())
    assert torch.equal(got.audio, ref.audio[0])
    bat.close()


def test_submit_stream_needs_a_streaming_batcher():
    loop = _loop("float32")
    bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED)
    with pytest.raises(ValueError, match="stream_chunk_frames"):
        bat.submit_stream(max_audio_length_ms=800, **_request(np.random.default_rng(1), 0, 3, 0, 3))
    bat.close()
