"""A sampler (and a seed) per request in one running batch (csm_serve.CSMBatcher(row_samplers=True), submit(sampler=, seed=)): a greedy
request, a top-k one and a top-p one share a max_batch = 2 engine, the third in the first one's row, and each carries, bit for bit, the frames,
codes and waveform of its own `generate_batch([prompt], sampler=its own, ...)` run.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from test_gpu_csm_serve import SEED, _loop, _request  # noqa: E402
from test_gpu_csm_stream import _solo_stream  # noqa: E402

pytestmark = pytest.mark.gpu


def _samplers():
    from mlx_audio_amd.sesame import make_sampler

    return [make_sampler(temp=0.0), make_sampler(temp=0.8, top_k=20), make_sampler(temp=1.1, top_k=0, top_p=0.9)]


def _solo(loop, prompt, frames, rng, sampler, seed, sid):
    if rng == "host":
        return loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=sampler, seed=seed)
    return loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=sampler, seed=seed, rng="device", stream_ids=[sid])


def _prompt(loop, req):
    return loop.prompt_frames(req["context"], req["text"], req["speaker"], voice_match=req["voice_match"])


def _same(got, ref, tag, audio=True):
    assert got.frames == ref.frames[0], tag
    np.testing.assert_array_equal(got.codes.cpu().numpy(), ref.codes[0][:, : ref.frames[0]].cpu().numpy(), err_msg=tag)
    if audio:
        assert torch.equal(got.audio, ref.audio[0]), tag


@pytest.mark.parametrize("rng", ["host", "device"])
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_three_samplers_in_one_batch_equal_their_solo_runs(wdt, rng):
    loop = _loop(wdt)
    g = np.random.default_rng(31)
    reqs = [_request(g, 0, 5, 2, 4), _request(g, 1, 4, 1, 6, voice_match=True), _request(g, 2, 3, 2, 3)]
    frames = [6, 16, 9]  # the greedy request ends first: the top-p one is admitted into its row beside the running top-k one
    sps = _samplers()
    bat = loop.serve(max_batch=2, rng=rng, sampler=sps[1], seed=SEED, row_samplers=True)
    # host: a generator seed per request; device: the batcher's seed (None), streams differ by their ids
    futs = [bat.submit(max_audio_length_ms=80 * frames[i], seed=(100 + i) if rng == "host" else None, stream_id=50 + i, sampler=sps[i], **reqs[i])
            for i in range(3)]
    bat.run_until_idle()
    res = [f.result(timeout=0) for f in futs]
    assert res[2].row == res[0].row != res[1].row and bat.stats["admissions"] == 3
    for i in range(3):
        ref = _solo(loop, _prompt(loop, reqs[i]), frames[i], rng, sps[i], (100 + i) if rng == "host" else SEED, 50 + i)
        _same(res[i], ref, f"request {i}")


def test_default_sampler_and_a_prefixed_request():
    """None = the batcher's sampler; a request on a voice prefix beside a plain one, each with a sampler of its own."""
    loop = _loop("bfloat16")
    g = np.random.default_rng(32)
    sps = _samplers()
    ctx = _request(g, 1, 5, 3, 2)["context"]
    reqs = [dict(context=ctx, text=g.integers(0, 300, 4).tolist(), speaker=1, voice_match=False), _request(g, 0, 4, 1, 3),
            dict(context=ctx, text=g.integers(0, 300, 2).tolist(), speaker=1, voice_match=False)]
    frames = [8, 12, 7]
    vp = loop.voice_prefix(ctx)
    bat = loop.serve(max_batch=2, rng="device", sampler=sps[2], seed=SEED, row_samplers=True)
    futs = [bat.submit(prefix=vp, text=reqs[0]["text"], speaker=1, max_audio_length_ms=80 * frames[0], stream_id=60, sampler=sps[1]),
            bat.submit(max_audio_length_ms=80 * frames[1], stream_id=61, sampler=sps[0], **reqs[1]),
            bat.submit(prefix=vp, text=reqs[2]["text"], speaker=1, max_audio_length_ms=80 * frames[2], stream_id=62)]  # the batcher's sampler
    bat.run_until_idle()
    assert bat.stats["prefixed_admissions"] == 2
    for i, sp in enumerate((sps[1], sps[0], sps[2])):
        ref = _solo(loop, _prompt(loop, reqs[i]), frames[i], "device", sp, SEED, 60 + i)
        _same(futs[i].result(timeout=0), ref, f"request {i}")
    vp.close()


def test_streamed_chunks_with_a_sampler_per_request():
    loop = _loop("float32")
    g = np.random.default_rng(33)
    sps = _samplers()
    reqs = [_request(g, 0, 4, 2, 3), _request(g, 1, 5, 1, 4)]
    frames, N = [10, 8], 3
    bat = loop.serve(max_batch=2, rng="host", sampler=sps[1], row_samplers=True, stream_chunk_frames=N, stream_max_frames=32)
    hs = [bat.submit_stream(max_audio_length_ms=80 * frames[i], seed=200 + i, stream_id=70 + i, sampler=sps[2 - i], **reqs[i]) for i in range(2)]
    bat.run_until_idle()
    mimi = loop._audio_tokenizer
    for i in range(2):
        res = hs[i].result(timeout=0)
        ref = _solo(loop, _prompt(loop, reqs[i]), frames[i], "host", sps[2 - i], 200 + i, 70 + i)
        _same(res, ref, f"request {i}", audio=False)
        n = int(ref.frames[0])
        steps = [N] * (n // N) + ([n % N] if n % N else [])
        cat = torch.cat([c.audio for c in hs[i]])
        assert torch.equal(cat, _solo_stream(mimi, ref.codes[0][:, :n], steps)), i
        assert torch.equal(res.audio, cat), i
    bat.close()


def test_a_seed_per_request_on_the_device_generator():
    loop = _loop("bfloat16")
    g = np.random.default_rng(34)
    sps = _samplers()
    reqs = [_request(g, 0, 5, 2, 3), _request(g, 1, 3, 1, 5)]
    frames, seeds = [9, 11], [2**35 + 3, 77]
    bat = loop.serve(max_batch=2, rng="device", sampler=sps[1], seed=SEED, row_samplers=True)
    futs = [bat.submit(max_audio_length_ms=80 * frames[i], seed=seeds[i], stream_id=80, sampler=sps[1 + i], **reqs[i]) for i in range(2)]
    bat.run_until_idle()
    for i in range(2):
        ref = _solo(loop, _prompt(loop, reqs[i]), frames[i], "device", sps[1 + i], seeds[i], 80)
        _same(futs[i].result(timeout=0), ref, f"request {i}")
    # without the option the same request is refused, as before
    plain = loop.serve(max_batch=2, rng="device", sampler=sps[1], seed=SEED)
    with pytest.raises(ValueError):
        plain.submit(max_audio_length_ms=800, seed=seeds[0], **reqs[0])
    with pytest.raises(ValueError):
        plain.submit(max_audio_length_ms=800, sampler=sps[0], **reqs[0])
