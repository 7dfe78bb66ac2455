"""Speech to text on a running CSM batch (`serve(stt=)`, `listen(transcribe=)`) on the tiny CSM and Mimi checkpoints of the listen
tests and a Whisper model of the serve tests' SHAPE_A (W = 200 frames: a window holds 2 s).  A listener's transcript equals, field by field
with ==, `whisper_model.decode(window, options)` for its window alone, the window being the composition of the existing ops
    mel_windows([log_mel_spectrogram(resample(heard[start:stop], 24000, 16000), 80, padding=W * 160)], [0], [W], W)[0]
on the reconstructed heard = resample(pcm.decode(bytes)); its `ListenResult`, onset, endpoint and codes equal those of the same listener on
a batcher without `stt=`; the generating request keeps the bits of its solo run.  No tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _pcm_ref as P  # noqa: E402
import _vad_ring_ref as VR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402
from test_gpu_csm_continuous import _drain  # noqa: E402
from test_gpu_csm_listen import M, SPF, _drive, _serve  # noqa: E402
from test_gpu_csm_serve import SEED, _check, _loop, _request, _sampler, _submit  # noqa: E402
from test_gpu_csm_vad import CFG, FL, HANG, SR, _clip, _until  # noqa: E402
from test_gpu_whisper_serve import _model, _same  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402
from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

pytestmark = pytest.mark.gpu

W = 200
MICS = [(SR, None, True), (16000, "s16le", True), (8000, "mulaw", False)]  # (rate, format, vad): the third is closed by `end()`
OPTS = [dict(sample_len=5, language=4), dict(sample_len=7, language=None), dict(sample_len=9, language=2, without_timestamps=True)]
PIECE = [1779, 1186, 593]  # samples per feed: the same 74.125 ms at every rate and no multiple of a frame at any


def _window(x):
    """the definition: a span's samples at the model's rate (device or host) -> its Whisper window"""
    a = RS.resample(torch.as_tensor(x).cuda().clone(), SR, 16000)
    mel = whisper.log_mel_spectrogram(a, 80, padding=W * 160).contiguous()
    return whisper.mel_windows([mel], [0], [W], W)[0]


def _heard(stored, rate, fmt):
    x = torch.from_numpy(P.decode(stored, fmt or "f32"))
    return (RS.resample(x, rate, SR) if rate != SR else x).cpu().numpy()


def _spy(bat, stt):
    """-> (cuts, embeds): per span launch the listen rows it took, per encoder call its windows"""
    cuts, embeds = [], []
    cut, embed = bat.engine.span_windows, stt.engine.embed_audio
    rows = lambda spans: [next(r for r in range(bat.listen_rows) if bat._heard[r].data_ptr() == sp[0].data_ptr()) for sp in spans]  # noqa: E731
    bat.engine.span_windows = lambda spans, *a: (cuts.append(rows(spans)), cut(spans, *a))[1]
    stt.engine.embed_audio = lambda mel: (embeds.append(int(mel.shape[0])), embed(mel))[1]
    return cuts, embeds


def _three_mics(loop, stored, req, stt):
    """The scenario, with `stt` or (None) on a batcher that never heard of it -> (listeners, their results, the request's future, batcher)"""
    kw = {} if stt is None else {"stt": stt}
    bat = _serve(loop, max_batch=2, listen_rows=3, **kw)
    fut = _submit(bat, "device", 0, req, 10)
    mics = []
    for (rate, fmt, vad), s, o in zip(MICS, stored, OPTS):
        extra = {} if stt is None else {"transcribe": o if vad else WD.DecodingOptions(**o)}  # (a dict and the options object are both taken)
        lis = bat.listen(sample_rate=rate, format=fmt, vad=CFG if vad else None, **extra)
        mics.append((lis, s, s.tobytes() if fmt else s, s.itemsize if fmt else 1))
    return bat, fut, mics


def _feed_all(bat, mics):
    at = [0, 0, 0]
    while any(at[i] < mics[i][1].shape[0] for i in range(3)):
        for i, (lis, stored, data, unit) in enumerate(mics):
            lis.feed(data[at[i] * unit : (at[i] + PIECE[i]) * unit])
            at[i] += PIECE[i]
        bat.step()


def test_three_microphones_beside_a_generating_request_and_a_window_of_the_callers_own():
    loop = _loop("float32")
    d, wm = _model("a")
    assert 2 * d.n_audio_ctx == W and d.n_mels == 80
    g = np.random.default_rng(95)
    req = _request(g, 0, 5, 2, 4)
    stored = [P.encode(_clip(g, rate), fmt or "f32") for rate, fmt, _ in MICS]
    own_feats, own_opts = T.features(d, 1, 41)[0], WD.DecodingOptions(sample_len=11, language=1)
    with wm.serve(max_rows=3, eos_check_interval=4) as stt:
        bat, fut, mics = _three_mics(loop, stored, req, stt)
        assert bat._stt is stt and all(m[0].transcript is not None and not m[0].transcript.done() for m in mics)
        cuts, embeds = _spy(bat, stt)
        own = stt.submit(own_feats, own_opts)  # the caller's own window shares the batch: the CSM scheduler steps it
        _feed_all(bat, mics)
        for lis, _, _, _ in mics[:2]:
            _until(bat, lis.endpoint)
        ends = [lis.end() for lis, _, _, _ in mics]
        for f in ends + [fut, own] + [m[0].transcript for m in mics]:
            _drive(bat, f)
        got = [(f.result(timeout=0), m[0].transcript.result(timeout=0)) for f, m in zip(ends, mics)]
        onsets = [(m[0].onset.result(timeout=0), m[0].endpoint.result(timeout=0)) for m in mics[:2]]
        assert sorted(len(c) for c in cuts) in ([1, 2], [3]) and embeds == [len(c) for c in cuts], (cuts, embeds)
        assert any(c[:2] == [0, 1] for c in cuts), "the two detectors' endpoints fall in one round: one span launch and one encoder call for both"
        assert bat.stats["stt_windows"] == 3 and bat.stats["stt_cuts"] == len(cuts)
        _check(loop, "device", [req], [10], [fut])  # the generating request: codes and waveform of its solo run, bit for bit
        bat.close()
        assert not stt.closed
        # every transcript is the solo decode of its window, field by field
        _same(own.result(timeout=0), wm.decode(own_feats, own_opts))
        for (rate, fmt, vad), s, o, (res, tr) in zip(MICS, stored, OPTS, got):
            heard = _heard(s, rate, fmt)
            start, stop = (res.speech_start, res.speech_stop) if vad else (0, heard.shape[0])
            assert 0 <= start < stop <= heard.shape[0] and (vad or res.speech_start is None)
            _same(tr, wm.decode(_window(heard[start:stop]), WD.DecodingOptions(**o)))
        assert len(got[0][1].tokens) <= 5
    # the same three microphones on a batcher without `stt=`: result, onset, endpoint and codes are those
    bat, fut, mics = _three_mics(loop, stored, req, None)
    assert bat._stt is None and all(m[0].transcript is None for m in mics)
    _feed_all(bat, mics)
    for lis, _, _, _ in mics[:2]:
        _until(bat, lis.endpoint)
    ends = [lis.end() for lis, _, _, _ in mics]
    for f in ends + [fut]:
        _drive(bat, f)
    for f, (res, _) in zip(ends, got):
        want = f.result(timeout=0)
        assert (res.frames, res.steps, res.samples, res.sample_rate, res.format, res.speech_start, res.speech_stop) == \
               (want.frames, want.steps, want.samples, want.sample_rate, want.format, want.speech_start, want.speech_stop)
        np.testing.assert_array_equal(res.codes.cpu().numpy(), want.codes.cpu().numpy())
    assert onsets == [(m[0].onset.result(timeout=0), m[0].endpoint.result(timeout=0)) for m in mics[:2]]
    bat.close()


def test_a_continuous_microphone_transcribes_every_utterance_a_forced_one_included():
    LMF = 16
    ring = LMF * SPF  # 30 720 samples: 42 detector frames and two thirds
    loop = _loop("float32")
    d, wm = _model("a")
    g = np.random.default_rng(96)
    piece = lambda q, s, t: [0.002 * g.standard_normal(q * FL), 0.3 * g.standard_normal(s * FL), 0.002 * g.standard_normal(t * FL)]  # noqa: E731
    S = np.concatenate(piece(12, 10, 21) + piece(12, 10, 21) + piece(5, 50, 14)).astype(np.float32)  # the third speaks past the length limit
    flags, records, status = VR.machine(S, FL, CFG.threshold, HANG, ring // FL)
    assert len(records) == 4 and [r[3] for r in records] == [0, 0, 1, 0] and S.shape[0] > 3 * ring
    opts = dict(sample_len=6, language=None)
    with wm.serve(max_rows=2, eos_check_interval=4) as stt:
        bat = loop.serve(rng="device", sampler=_sampler(), seed=SEED, listen_chunk_frames=M, listen_max_frames=LMF, max_batch=1, listen_rows=1, stt=stt,
                         stt_rounds_per_round=2)
        cuts, embeds = _spy(bat, stt)
        lis = bat.listen(vad=CFG, continuous=True, transcribe=opts)
        got, at = [], 0
        for _ in range(4000):
            if at >= S.shape[0]:
                break
            k = min(1777, S.shape[0] - at)
            if lis._qn + k <= lis.cap:
                lis.feed(S[at : at + k])
                at += k
            _drain(lis, got)
            bat.step()
        lis.close()
        for _ in range(600):
            if bat._listeners[0] is None and all(u.transcript.done() for u, _ in got):
                break
            bat.step()
            _drain(lis, got)
        assert bat._listeners[0] is None and len(got) == 4 and sum(len(c) for c in cuts) == 4 and embeds == [len(c) for c in cuts]
        bat.close()
        for (u, f), rec in zip(got, records):
            start, stop = VR.span(rec, FL, 0, None, HANG)
            res = f.result(timeout=0)
            assert (res.speech_start, res.speech_stop) == (start, stop) and u.endpoint.result(timeout=0).forced == bool(rec[3])
            _same(u.transcript.result(timeout=0), wm.decode(_window(S[start:stop]), WD.DecodingOptions(**opts)))
        assert any(VR.span(r, FL, 0, None, HANG)[0] // ring != (VR.span(r, FL, 0, None, HANG)[1] - 1) // ring for r in records), "a span wraps the ring's end"


def test_an_utterance_longer_than_a_window_fails_its_transcript_alone():
    loop = _loop("float32")
    d, wm = _model("a")
    g = np.random.default_rng(97)
    pcm = (0.3 * g.standard_normal(48001)).astype(np.float32)  # 32 001 samples at 16 kHz: one more than W * 160
    with wm.serve(max_rows=2) as stt:
        bat = _serve(loop, max_batch=1, listen_rows=2, stt=stt)
        long_, ok = bat.listen(transcribe=dict(language=4, sample_len=4)), bat.listen(transcribe=dict(language=4, sample_len=4))
        long_.feed(pcm)
        ok.feed(pcm[:48000])
        f1, f2 = long_.end([1, 2, 3]), ok.end()
        for f in (f1, f2, ok.transcript):
            _drive(bat, f)
        with pytest.raises(ValueError, match="32001 samples at 16 kHz"):
            long_.transcript.result(timeout=0)
        assert f1.result(timeout=0).frames == 26 and f2.result(timeout=0).frames == 25  # `end(text)` resolves as before
        _same(ok.transcript.result(timeout=0), wm.decode(_window(pcm[:48000]), WD.DecodingOptions(language=4, sample_len=4)))
        bat.close()


def test_a_session_hears_a_turn_nobody_typed():
    loop = _loop("float32")
    d, wm = _model("a")
    g = np.random.default_rng(98)
    clip, said = _clip(g, SR), g.integers(0, 300, 4).tolist()
    opts = dict(sample_len=6, language=4, without_timestamps=True)
    stt_text = lambda r: [t % 300 for t in r.tokens]  # noqa: E731  (ids the tiny text vocabulary holds)
    with wm.serve(max_rows=2) as stt:
        bat = _serve(loop, max_batch=1, listen_rows=1, stop_on_eos=False, stt=stt, stt_text=stt_text)
        sess = bat.session()
        lis = sess.listen(1, vad=CFG, transcribe=opts)
        for i in range(0, clip.shape[0], 2500):
            lis.feed(clip[i : i + 2500])
        f = lis.end()  # no text: the heard turn waits for the transcript
        assert sess.busy
        _drive(bat, f)
        res, tr = f.result(timeout=0), lis.transcript.result(timeout=0)
        assert not sess.busy and len(tr.tokens) >= 1
        turn = sess.submit(said, max_audio_length_ms=80 * 4, stream_id=60)
        _drive(bat, turn)
        solo = wm.decode(_window(clip[res.speech_start : res.speech_stop]), WD.DecodingOptions(**opts))
        _same(tr, solo)
        # the twin: no Whisper anywhere, the text typed
        twin_bat = _serve(loop, max_batch=1, listen_rows=1, stop_on_eos=False)
        twin = twin_bat.session()
        tl = twin.listen(1, vad=CFG)
        tl.feed(clip)
        f2 = tl.end(stt_text(solo))
        _drive(twin_bat, f2)
        turn2 = twin.submit(said, max_audio_length_ms=80 * 4, stream_id=60)
        _drive(twin_bat, turn2)
        assert sess.turns == twin.turns and sess.turns[0] == (1, stt_text(solo), 0) and sess.length == twin.length and sess.n == twin.n
        for x, y in zip(sess.history + sess.pending, twin.history + twin.pending):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(res.codes.cpu().numpy(), f2.result(timeout=0).codes.cpu().numpy())
        np.testing.assert_array_equal(turn.result(timeout=0).codes.cpu().numpy(), turn2.result(timeout=0).codes.cpu().numpy())
        sess.close(); twin.close(); bat.close(); twin_bat.close()
        # without stt_text the refusal stands
        bat = _serve(loop, max_batch=1, listen_rows=1, stt=stt)
        lis = bat.session().listen(1, vad=CFG, transcribe=opts)
        lis.feed(clip[:5000])
        with pytest.raises(ValueError, match="needs its text"):
            lis.end()
        bat.close()
