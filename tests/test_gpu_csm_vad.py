"""Voice-activity endpointing on a running CSM batch (`listen(vad=)`, `CSMSession.listen(vad=, barge_in=True)`) on the tiny CSM
and Mimi checkpoints of the listen tests.  An f32 listener at 24 kHz, an s16le one at 16 kHz and a mu-law one at 8 kHz each hear about 0.3 s
of near-silence, 0.5 s of noise speech and silence to the endpoint, fed in odd slices beside a generating request.  With
heard = resample(pcm.decode(bytes)) -- what the listener's device buffer holds -- `speech_start` / `speech_stop` are those of
tests/_vad_ref.py on heard, and the codes equal, as integers, those of a plain listener fed heard[start:stop] and ended.  No tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _pcm_ref as P  # noqa: E402
import _vad_ref as V  # noqa: E402
from test_gpu_csm_listen import _drive, _serve  # noqa: E402
from test_gpu_csm_serve import SEED, _check, _loop, _request, _sampler, _submit  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402
from mlx_audio_amd.vad import VadConfig  # noqa: E402

pytestmark = pytest.mark.gpu

SR, FL, HANG = 24000, 720, 10
CFG = VadConfig(silence_ms=300)  # 30 ms frames, threshold 0.03: the reference's; a short hang keeps the clips short
MICS = [(SR, None), (16000, "s16le"), (8000, "mulaw")]
QUIET, SPEECH, TAIL = 10, 17, 14  # detector frames: 0.3 s, 0.51 s, and silence past the 11th silent frame


def _clip(g, rate):
    """float32 at `rate`: the three pieces, each a whole number of detector frames at every rate used"""
    n = [k * FL * rate // SR for k in (QUIET, SPEECH, TAIL)]
    return np.concatenate([0.002 * g.standard_normal(n[0]), 0.3 * g.standard_normal(n[1]), 0.002 * g.standard_normal(n[2])]).astype(np.float32)


def _until(bat, fut):
    for _ in range(600):
        if fut.done():
            return
        bat.step()
    raise AssertionError("the future did not resolve")


def _plain_codes(loop, heard):
    """The result of a plain f32 listener at the model's rate fed `heard` and ended, on a batcher of its own."""
    bat = _serve(loop, max_batch=1, listen_rows=1)
    lis = bat.listen()
    lis.feed(heard)
    fut = lis.end()
    _until(bat, fut)
    res = fut.result(timeout=0)
    assert bat._vad is None and res.speech_start is None
    bat.close()
    return res


def test_three_vad_listeners_beside_a_generating_request():
    assert CFG.frame_len(SR) == FL and CFG.hang_frames == HANG
    loop = _loop("float32")
    g = np.random.default_rng(91)
    req = _request(g, 0, 5, 2, 4)
    bat = _serve(loop, max_batch=2, listen_rows=3)
    fut = _submit(bat, "device", 0, req, 10)
    mics = []
    for rate, fmt in MICS:
        stored = P.encode(_clip(g, rate), fmt or "f32")
        lis = bat.listen(sample_rate=rate, format=fmt, vad=CFG)
        mics.append((lis, stored, stored.tobytes() if fmt else stored, stored.itemsize if fmt else 1))
    assert bat._vad is None
    piece = [1777, 1234, 999]  # samples per feed: no multiple of a frame at any rate
    at = [0, 0, 0]
    while any(at[i] < mics[i][1].shape[0] for i in range(3)):
        for i, (lis, stored, data, unit) in enumerate(mics):
            lis.feed(data[at[i] * unit : (at[i] + piece[i]) * unit])
            at[i] += piece[i]
        bat.step()
    for lis, _, _, _ in mics:
        _until(bat, lis.endpoint)
    assert bat._vad is not None
    ends = [lis.end() for lis, _, _, _ in mics]
    for f in ends + [fut]:
        _drive(bat, f)
    for (rate, fmt), (lis, stored, _, _), f in zip(MICS, mics, ends):
        res = f.result(timeout=0)
        x = torch.from_numpy(P.decode(stored, fmt or "f32"))
        heard = (RS.resample(x, rate, SR) if rate != SR else x).cpu().numpy()
        flags, status = V.machine(heard, FL, CFG.threshold, HANG)
        assert status[1] == QUIET and status[3] == QUIET + SPEECH + HANG, (rate, status)  # the clip is what its layout says, at every rate
        start, stop = V.span(status, heard.shape[0], FL, 0, None, HANG)
        assert (res.speech_start, res.speech_stop) == (start, stop) and lis.onset.result(timeout=0) == start
        sp = lis.endpoint.result(timeout=0)
        assert (sp.start, sp.stop, sp.onset_frame, sp.endpoint_frame, sp.sample_rate) == (start, stop, status[1], status[3], rate)
        want = _plain_codes(loop, heard[start:stop])
        assert (res.frames, res.steps) == (want.frames, want.steps) and res.frames == -(-(stop - start) // 1920)
        np.testing.assert_array_equal(res.codes.cpu().numpy(), want.codes.cpu().numpy())
    _check(loop, "device", [req], [10], [fut])  # the generating request: codes and waveform of its solo run, bit for bit
    bat.close()


def test_barge_in_ends_the_sessions_live_streaming_turn():
    loop = _loop("float32")
    g = np.random.default_rng(92)
    said, heard_text = g.integers(0, 300, 4).tolist(), g.integers(0, 300, 3).tolist()
    bat = _serve(loop, listen_rows=1, max_batch=1, stop_on_eos=False, stream_chunk_frames=2, stream_max_frames=32)
    sess = bat.session()
    st = sess.submit_stream(said, max_audio_length_ms=80 * 30, stream_id=50)
    for _ in range(6):
        assert bat.step()
    assert not st.future.done()
    lis = sess.listen(1, vad=CFG, barge_in=True)  # the user speaks while the agent speaks
    clip = np.concatenate([0.3 * g.standard_normal(3 * FL), 0.002 * g.standard_normal((HANG + 2) * FL)]).astype(np.float32)
    lis.feed(clip)
    _until(bat, lis.onset)
    assert lis.onset.result(timeout=0) == 0 and st.future.done()  # the round that saw the onset ended the turn
    r = st.result(timeout=0)
    assert r.interrupted and 1 <= r.frames < 30 and sess.turns[-1][2] == r.frames
    _until(bat, lis.endpoint)
    f = lis.end(heard_text)
    _drive(bat, f)
    res = f.result(timeout=0)
    assert (res.speech_start, res.speech_stop) == (0, (3 + HANG + 1) * FL) and sess.turns[-1] == (1, heard_text, 0) and not sess.busy
    sess.close(); bat.close()
