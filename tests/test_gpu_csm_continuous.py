"""Always-open microphones on a running CSM batch (`listen(vad=, continuous=True)`) on the tiny CSM and Mimi checkpoints of
the listen tests, with listen_max_frames = 16: the ring is 30 720 samples (42.67 detector frames) and every stream is three rings long.
An f32 listener at 24 kHz, an s16le one at 16 kHz and a mu-law one at 8 kHz each hear three utterances on ONE microphone, fed in odd
slices beside a generating request.  With S = resample(pcm.decode(bytes)), the spans are those of tests/_vad_ring_ref.py (and of
`vad.utterances`) on S, and every utterance's codes equal, as integers, those of a plain listener fed S[start:stop] and ended.  No tolerance."""
import os
import queue
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _pcm_ref as P  # noqa: E402
import _vad_ring_ref as R  # noqa: E402
from test_gpu_csm_listen import M, SPF, _drive  # noqa: E402
from test_gpu_csm_serve import SEED, _check, _loop, _request, _sampler, _submit  # noqa: E402
from test_gpu_csm_vad import _plain_codes  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402
from mlx_audio_amd import vad as VAD  # noqa: E402
from mlx_audio_amd.csm_continuous import CSMContinuousListener  # noqa: E402

pytestmark = pytest.mark.gpu

SR, FL, HANG, LMF = 24000, 720, 10, 16
RING = LMF * SPF
CFG = VAD.VadConfig(silence_ms=300)  # 30 ms frames, threshold 0.03: the reference's; a short hang keeps the clips short
MICS = [(SR, None), (16000, "s16le"), (8000, "mulaw")]
QUIET, SPEECH, TAIL = 12, 10, 21  # detector frames per utterance: 43, so three of them are 129 frames = 92 880 samples > 3 rings


def _serve(loop, **kw):
    return loop.serve(rng="device", sampler=_sampler(), seed=SEED, listen_chunk_frames=M, listen_max_frames=LMF, **kw)


def _stream(g, rate):
    """float32 at `rate`: three utterances, every piece a whole number of detector frames at every rate used"""
    n = [k * FL * rate // SR for k in (QUIET, SPEECH, TAIL)]
    one = lambda: np.concatenate([0.002 * g.standard_normal(n[0]), 0.3 * g.standard_normal(n[1]), 0.002 * g.standard_normal(n[2])])  # noqa: E731
    return np.concatenate([one(), one(), one()]).astype(np.float32)


def _drain(lis, got, text=None):
    while True:
        try:
            u = lis.next_utterance(0)
        except queue.Empty:
            return
        if u is None:
            return
        got.append((u, u.end(text)))


def test_three_microphones_three_utterances_each_beside_a_generating_request():
    assert CFG.frame_len(SR) == FL and CFG.hang_frames == HANG and RING % FL != 0
    loop = _loop("float32")
    g = np.random.default_rng(93)
    req = _request(g, 0, 5, 2, 4)
    bat = _serve(loop, max_batch=2, listen_rows=3)
    fut = _submit(bat, "device", 0, req, 10)
    mics = []
    for rate, fmt in MICS:
        stored = P.encode(_stream(g, rate), fmt or "f32")
        lis = bat.listen(sample_rate=rate, format=fmt, vad=CFG, continuous=True)
        assert isinstance(lis, CSMContinuousListener) and lis.ring_len == RING and lis.max_frames == RING // FL
        mics.append((lis, stored, stored.tobytes() if fmt else stored, stored.itemsize if fmt else 1, []))
    assert bat._rvad is None and bat._vad is None
    piece = [1777, 1234, 999]  # samples per feed: no multiple of a frame at any rate
    at = [0, 0, 0]
    for _ in range(4000):
        if not any(at[i] < mics[i][1].shape[0] for i in range(3)):
            break
        for i, (lis, stored, data, unit, got) in enumerate(mics):
            k = min(piece[i], stored.shape[0] - at[i])
            if k and lis._qn + k <= lis.cap:  # (a full host queue is waited for: the test feeds faster than a microphone)
                lis.feed(data[at[i] * unit : (at[i] + k) * unit])
                at[i] += k
            _drain(lis, got)
        bat.step()
    assert at == [m[1].shape[0] for m in mics] and bat._rvad is not None and bat._vad is None
    for lis, _, _, _, _ in mics:
        lis.close()
    for _ in range(600):
        if all(bat._listeners[r] is None for r in range(3)):
            break
        bat.step()
        for lis, _, _, _, got in mics:
            _drain(lis, got)
    assert all(bat._listeners[r] is None for r in range(3))
    _drive(bat, fut)
    for (rate, fmt), (lis, stored, _, _, got) in zip(MICS, mics):
        x = torch.from_numpy(P.decode(stored, fmt or "f32"))
        S = (RS.resample(x, rate, SR) if rate != SR else x).cpu().numpy()
        assert S.shape[0] >= 3 * RING and lis._n24 == S.shape[0]
        flags, records, status = R.machine(S, FL, CFG.threshold, HANG, RING // FL)
        assert VAD.utterances(CFG, S, SR, RING // FL) == (records, status)
        per = QUIET + SPEECH + TAIL
        assert records == [(k * per + QUIET, k * per + QUIET + SPEECH - 1, k * per + QUIET + SPEECH + HANG, 0) for k in range(3)], (rate, records)
        assert len(got) == 3 and lis.next_utterance(0) is None
        for (u, f), rec in zip(got, records):
            start, stop = R.span(rec, FL, 0, None, HANG)
            sp = u.endpoint.result(timeout=0)
            assert (sp.start, sp.stop, sp.onset_frame, sp.endpoint_frame, sp.sample_rate, sp.forced) == (start, stop, rec[0], rec[2], rate, False)
            res = f.result(timeout=0)
            assert u.onset == start and (res.speech_start, res.speech_stop, res.samples) == (start, stop, stop - start)
            want = _plain_codes(loop, S[start:stop])
            assert (res.frames, res.steps) == (want.frames, want.steps) and res.frames == -(-(stop - start) // SPF)
            np.testing.assert_array_equal(res.codes.cpu().numpy(), want.codes.cpu().numpy())
    _check(loop, "device", [req], [10], [fut])  # the generating request: codes and waveform of its solo run, bit for bit
    bat.close()


def test_barge_in_ends_the_live_streaming_turn_on_the_second_utterance():
    loop = _loop("float32")
    g = np.random.default_rng(94)
    said, t1, t2 = g.integers(0, 300, 4).tolist(), g.integers(0, 300, 3).tolist(), g.integers(0, 300, 2).tolist()
    bat = _serve(loop, listen_rows=1, max_batch=1, stop_on_eos=False, stream_chunk_frames=2, stream_max_frames=32)
    sess = bat.session()
    lis = sess.listen(1, vad=CFG, continuous=True, barge_in=True)
    clip = lambda: np.concatenate([0.3 * g.standard_normal(3 * FL), 0.002 * g.standard_normal((HANG + 2) * FL)]).astype(np.float32)  # noqa: E731
    a, b = clip(), clip()
    got = []
    lis.feed(a)  # the first utterance: nobody speaks yet, nothing to interrupt
    for _ in range(600):
        _drain(lis, got, t1)
        if got:
            break
        bat.step()
    _drive(bat, got[0][1])
    r1 = got[0][1].result(timeout=0)
    assert (r1.speech_start, r1.speech_stop) == (0, (3 + HANG + 1) * FL) and sess.turns[-1] == (1, t1, 0) and not sess.busy
    st = sess.submit_stream(said, max_audio_length_ms=80 * 30, stream_id=50)
    for _ in range(6):
        assert bat.step()
    assert not st.future.done()
    lis.feed(b)  # the user speaks again while the agent speaks
    u2 = None
    for _ in range(600):
        try:
            u2 = lis.next_utterance(0)
            break
        except queue.Empty:
            assert not st.future.done()
            bat.step()
    assert u2 is not None and u2.onset == a.shape[0] and st.future.done()  # the round that saw the second onset ended the turn
    r = st.result(timeout=0)
    assert r.interrupted and 1 <= r.frames < 30 and sess.turns[-1][2] == r.frames
    for _ in range(600):
        if u2.endpoint.done():
            break
        bat.step()
    f2 = u2.end(t2)
    _drive(bat, f2)
    r2 = f2.result(timeout=0)
    assert (r2.speech_start, r2.speech_stop) == (a.shape[0], a.shape[0] + (3 + HANG + 1) * FL) and sess.turns[-1] == (1, t2, 0) and not sess.busy
    lis.close()
    for _ in range(100):
        if bat._listeners[0] is None:
            break
        bat.step()
    assert bat._listeners[0] is None
    sess.close(); bat.close()
