"""PCM formats on a running CSM batch (csm_serve.CSMBatcher: `listen(format=)`, `submit(..., format=)`) on the tiny CSM and Mimi
configurations.  In: a listener fed bytes carries, as integers, the codes of an f32 twin fed `pcm.decode(the bytes)` at the same rate, beside a
generating request.  Out: the chunks of a request with a format concatenate, element for element, to `pcm.encode` of the audio the same request
yields at the same rate without one.  The host rules come from tests/_pcm_ref.py.  No tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _pcm_ref as P  # noqa: E402
from test_gpu_csm_listen import SPF, _drive, _pcm, _serve  # noqa: E402
from test_gpu_csm_serve import SEED, _check, _loop, _request, _sampler, _submit  # noqa: E402

from mlx_audio_amd import pcm  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 24000
MICS = [(8000, "mulaw", 3000), (16000, "s16le", 6100), (SR, "s16le", 4 * SPF + 11), (SR, None, 3 * SPF + 5)]  # (rate, format, samples fed)


def _listen_all(loop, clips, formatted):
    """The four microphones beside a generating request: fed the stored bytes (`formatted`) or, as f32 twins, the decoded floats."""
    g = np.random.default_rng(81)
    req = _request(g, 0, 5, 2, 4)
    bat = _serve(loop, max_batch=2, listen_rows=4)
    fut = _submit(bat, "device", 0, req, 10)
    mics = []
    for (rate, fmt, _), stored in zip(MICS, clips):
        lis = bat.listen(sample_rate=rate, format=fmt if formatted else None)
        mics.append((lis, stored.tobytes() if formatted and fmt is not None else P.decode(stored, fmt or "f32"), stored.itemsize if formatted and fmt else 1))
    assert bat._cvt is None and bat._lrs is None
    for k in range(4):  # four uneven pieces each, a round between
        for lis, data, unit in mics:
            n = len(data) // unit
            cuts = [0, n // 7, n // 2 + 1, n - 3, n]
            lis.feed(data[cuts[k] * unit : cuts[k + 1] * unit])
        bat.step()
    futs = [lis.end() for lis, _, _ in mics]
    for f in futs + [fut]:
        _drive(bat, f)
    made = (bat._cvt is not None, bat._lrs is not None)
    out = [f.result(timeout=0) for f in futs]
    _check(loop, "device", [req], [10], [fut])  # the generating request: codes and waveform of its solo run, bit for bit
    bat.close()
    return out, made


def test_listeners_in_mulaw_s16le_and_f32_carry_the_codes_of_their_f32_twins():
    loop = _loop("float32")
    g = np.random.default_rng(80)
    clips = [P.encode(_pcm(g, n), fmt or "f32") for _, fmt, n in MICS]
    got, made = _listen_all(loop, clips, True)
    want, twin_made = _listen_all(loop, clips, False)
    assert made == (True, True) and twin_made == (False, True)  # the converter serves the formatted row at the model's rate only
    for (rate, fmt, n), r, w in zip(MICS, got, want):
        assert (r.format, w.format) == (fmt or "f32", "f32") and r.sample_rate == w.sample_rate == rate
        assert r.samples == w.samples == n and r.steps == w.steps and r.frames == w.frames > 0
        np.testing.assert_array_equal(r.codes.cpu().numpy(), w.codes.cpu().numpy())
    with pytest.raises(ValueError, match="whole number"):
        bat = _serve(loop, max_batch=2, listen_rows=1)
        try:
            bat.listen(format="s16le").feed(b"\x00\x01\x02")
        finally:
            bat.close()


def test_streams_in_mulaw_at_8k_and_s16le_at_24k_and_a_plain_request_in_s16le_at_48k_equal_the_encoded_f32_runs():
    loop = _loop("float32")
    g = np.random.default_rng(82)
    reqs = [_request(g, 0, 5, 2, 4), _request(g, 1, 4, 0, 5), _request(g, 0, 3, 0, 4)]
    kw = dict(max_batch=3, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False, stream_chunk_frames=2, stream_max_frames=16)

    def run(formatted):
        f = (lambda name: name) if formatted else (lambda name: None)
        bat = loop.serve(**kw)
        a = bat.submit_stream(max_audio_length_ms=80 * 7, stream_id=50, sample_rate=8000, format=f("mulaw"), **reqs[0])
        b = bat.submit_stream(max_audio_length_ms=80 * 6, stream_id=51, format=f("s16le"), **reqs[1])
        c = bat.submit(max_audio_length_ms=80 * 5, stream_id=52, sample_rate=48000, format=f("s16le"), **reqs[2])
        for h in (a.future, b.future, c):
            _drive(bat, h)
        out = list(a), a.result(timeout=0), list(b), b.result(timeout=0), c.result(timeout=0), bat._cvt is not None
        bat.close()
        return out

    ca, ra, cb, rb, rc, made = run(True)
    fa, wa, fb, wb, wc, twin_made = run(False)
    assert made and not twin_made
    for chunks, res, ref_chunks, ref, fmt in ((ca, ra, fa, wa, "mulaw"), (cb, rb, fb, wb, "s16le")):
        want = torch.from_numpy(P.encode(ref.audio.cpu().numpy(), fmt))
        assert res.format == fmt and ref.format == "f32" and res.sample_rate == ref.sample_rate and res.frames == ref.frames
        assert [(c.first_frame, c.frames, c.final, c.audio.shape[0]) for c in chunks] == [(c.first_frame, c.frames, c.final, c.audio.shape[0]) for c in ref_chunks]
        assert all(c.format == fmt and c.audio.dtype == pcm.torch_dtype(fmt) and c.audio.is_cuda for c in chunks)
        assert torch.equal(torch.cat([c.audio for c in chunks]).cpu(), want) and torch.equal(res.audio.cpu(), want)
        print(f"{fmt}: {len(torch.unique(want))} distinct codes in {want.shape[0]} samples")
        assert len(torch.unique(want)) > 16  # the comparison says something: the audio is not silence or the clamp
        np.testing.assert_array_equal(res.codes.cpu().numpy(), ref.codes.cpu().numpy())
    assert rc.format == "s16le" and rc.sample_rate == 48000 and rc.audio.dtype == torch.int16 and rc.audio.shape[0] == 2 * 5 * SPF
    assert torch.equal(rc.audio.cpu(), torch.from_numpy(P.encode(wc.audio.cpu().numpy(), "s16le")))


def test_a_heard_turn_in_mulaw_equals_its_hear_twin():
    from mlx_audio_amd import resample as RS
    from mlx_audio_amd.sesame import Segment

    loop = _loop("float32")
    g = np.random.default_rng(83)
    stored = P.encode(_pcm(g, 3000), "mulaw")  # 9 000 samples at 24 kHz: T = 5
    heard, said = g.integers(0, 300, 3).tolist(), g.integers(0, 300, 4).tolist()
    bat = _serve(loop, max_batch=2, listen_rows=1, stop_on_eos=False)
    sess = bat.session()
    lis = sess.listen(1, sample_rate=8000, format="mulaw")
    data = stored.tobytes()
    for i in range(0, len(data), 850):
        lis.feed(data[i : i + 850])
    f = lis.end(heard)
    bat.run_until_idle()
    res = f.result(timeout=0)
    assert res.format == "mulaw" and res.samples == 3000 and res.frames == 5
    turn = sess.submit(said, max_audio_length_ms=80 * 6, stream_id=60)
    _drive(bat, turn)
    x24 = RS.resample(torch.from_numpy(P.decode(stored, "mulaw")), 8000, SR).cpu().numpy()  # what the turn's Segment holds
    twin_bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False)
    twin = twin_bat.session()
    twin.hear(Segment(speaker=1, text=heard, audio=x24), codes=res.codes.cpu().numpy())
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
