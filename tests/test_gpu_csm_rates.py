"""Other sample rates on a running CSM batch (csm_serve.CSMBatcher: `listen(sample_rate=)`, `submit(..., sample_rate=)`) on the
tiny CSM and Mimi configurations.  In: a listener fed at R carries, as integers, the codes of a fresh batch-1 `Mimi.encode_step` stream over
`resample(clip, R, 24000)` zero-padded, in the steps its length fixes, whatever the slicing and whatever else listens or is generated.  Out: the
chunks of a request at R concatenate, bit for bit, to `resample(a, 24000, R)` of the audio `a` the same request yields at 24 kHz.  No tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _resample_ref as R  # noqa: E402
from test_gpu_csm_listen import M, MAX_FRAMES, SPF, _drive, _pcm, _serve, _solo_codes, _steps  # noqa: E402
from test_gpu_csm_serve import SEED, _check, _loop, _request, _sampler, _submit  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 24000


def _at_24k(pcm, rate):
    return RS.resample(torch.from_numpy(pcm), rate, SR).cpu().numpy()


def _listened(res, mimi, pcm, rate):
    """The integer-codes contract of a listener fed `pcm` at `rate`."""
    x = pcm if rate == SR else _at_24k(pcm, rate)
    assert x.shape[0] == R.out_len(pcm.shape[0], *R.ratio(rate, SR))
    want = _solo_codes(mimi, x)
    assert res.sample_rate == rate and res.samples == pcm.shape[0]
    assert res.steps == _steps(x.shape[0]) and res.frames == want.shape[1]
    np.testing.assert_array_equal(res.codes.cpu().numpy(), want)
    return want, x


def test_listeners_at_16k_44k1_and_the_default_rate_beside_a_generating_request():
    loop = _loop("float32")
    g = np.random.default_rng(71)
    req = _request(g, 0, 5, 2, 4)
    a_pcm, b_pcm, c_pcm = _pcm(g, 8000), _pcm(g, 17000), _pcm(g, 4 * SPF + 11)  # 24 kHz: 12 000 (T = 7), 9 252 (T = 5), T = 5
    bat = _serve(loop, max_batch=2, listen_rows=3)
    fut = _submit(bat, "device", 0, req, 10)
    a, b, c = bat.listen(sample_rate=16000), bat.listen(speaker=1, sample_rate=44100), bat.listen(speaker=2)
    assert bat._lrs is None
    c.feed(c_pcm)
    b.feed(b_pcm[:4411])
    for i in range(0, a_pcm.shape[0], 700):  # a in slices of 700 with a round between, b in three uneven pieces
        a.feed(a_pcm[i : i + 700])
        if i == 2800:
            b.feed(b_pcm[4411:4412])
        if i == 5600:
            b.feed(b_pcm[4412:])
        bat.step()
    assert a.frames >= M and tuple(a.codes().shape) == (loop.n_cb, a.frames)
    fa, fb, fc = a.end(), b.end(), c.end()
    for f in (fa, fb, fc, fut):
        _drive(bat, f)
    mimi = loop._audio_tokenizer
    _listened(fa.result(timeout=0), mimi, a_pcm, 16000)
    _listened(fb.result(timeout=0), mimi, b_pcm, 44100)
    _listened(fc.result(timeout=0), mimi, c_pcm, SR)
    assert bat.stats["listen_frames"] == 7 + 5 + 5
    _check(loop, "device", [req], [10], [fut])  # the generating request: codes and waveform of its solo run, bit for bit
    with pytest.raises(ValueError, match="listen_max_frames"):
        d = bat.listen(sample_rate=8000)
        d.feed(np.zeros(MAX_FRAMES * SPF // 3 + 1, np.float32))
    bat.close()


def test_a_stream_at_8k_and_a_plain_request_at_48k_are_the_resampled_24k_run():
    loop = _loop("float32")
    g = np.random.default_rng(72)
    reqs = [_request(g, 0, 5, 2, 4), _request(g, 1, 4, 0, 5)]
    kw = dict(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False, stream_chunk_frames=2, stream_max_frames=16)

    def run(rate_stream, rate_plain):
        bat = loop.serve(**kw)
        st = bat.submit_stream(max_audio_length_ms=80 * 7, stream_id=50, sample_rate=rate_stream, **reqs[0])
        fut = bat.submit(max_audio_length_ms=80 * 5, stream_id=51, sample_rate=rate_plain, **reqs[1])
        _drive(bat, st.future); _drive(bat, fut)
        chunks = list(st)
        made = bat._ors is not None
        bat.close()
        return chunks, st.result(timeout=0), fut.result(timeout=0), made

    chunks, rs, rp, made = run(8000, 48000)
    ref_chunks, ref_s, ref_p, ref_made = run(None, None)
    assert made and not ref_made
    assert ref_s.frames == rs.frames == 7 and ref_p.frames == rp.frames == 5 and (ref_s.sample_rate, rs.sample_rate, rp.sample_rate) == (SR, 8000, 48000)
    np.testing.assert_array_equal(rs.codes.cpu().numpy(), ref_s.codes.cpu().numpy())
    assert [c.frames for c in chunks] == [c.frames for c in ref_chunks] == [2, 2, 2, 1] and chunks[-1].final
    want = RS.resample(ref_s.audio, SR, 8000)
    assert want.shape[0] == R.out_len(7 * SPF, 1, 3) == sum(c.audio.shape[0] for c in chunks)
    assert torch.equal(torch.cat([c.audio for c in chunks]), want) and torch.equal(rs.audio, want)
    assert torch.equal(rp.audio, RS.resample(ref_p.audio, SR, 48000)) and rp.audio.shape[0] == 2 * 5 * SPF


def test_a_listened_turn_at_16k_equals_a_hear_twin():
    from mlx_audio_amd.sesame import Segment

    loop = _loop("float32")
    g = np.random.default_rng(73)
    pcm = _pcm(g, 6000)  # 9 000 samples at 24 kHz: T = 5
    heard, said = g.integers(0, 300, 3).tolist(), g.integers(0, 300, 4).tolist()
    bat = _serve(loop, max_batch=2, listen_rows=1, stop_on_eos=False)
    sess = bat.session()
    lis = sess.listen(1, sample_rate=16000)
    for i in range(0, pcm.shape[0], 1700):
        lis.feed(pcm[i : i + 1700])
    f = lis.end(heard)
    bat.run_until_idle()
    codes, x24 = _listened(f.result(timeout=0), loop._audio_tokenizer, pcm, 16000)
    turn = sess.submit(said, max_audio_length_ms=80 * 6, stream_id=60)
    _drive(bat, turn)
    twin_bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, stop_on_eos=False)
    twin = twin_bat.session()
    twin.hear(Segment(speaker=1, text=heard, audio=x24), codes=codes)
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
