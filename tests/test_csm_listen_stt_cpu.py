"""Speech to text for listeners (`CSMBatcher(stt=)`, `listen(transcribe=)`) with fake engines on both sides (no device): the
scripted CSM engine, encoder, detectors and ring copies of test_csm_continuous_cpu.py with a `span_windows` that records what it was asked
to cut, and the scripted Whisper engine of test_whisper_serve_cpu.py with an `embed_audio`.  A fake window is its span's (ring length, start,
samples, first sample); the fake features carry a tag that says which span of which cut they came from, and the pick at which the row ends.
Checked: the refusals, the stepping rule, one cut per round in row order, cancel before and after the cut, close, a session's `end()` without
text, and that a batcher without `stt=` makes nothing of it."""
import os
import sys
from concurrent.futures import CancelledError

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_text_ref as T  # noqa: E402
from test_csm_continuous_cpu import LMF, Engine as _Engine, _cfg, _drain  # noqa: E402
from test_csm_interrupt_cpu import SPF, _batcher  # noqa: E402
from test_csm_vad_cpu import LOUD, QUIET, M, _clip  # noqa: E402
from test_whisper_serve_cpu import FakeEngine as _Whisper  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd.whisper_decoding import DecodingOptions, DecodingResult  # noqa: E402
from mlx_audio_amd.whisper_serve import WhisperBatcher  # noqa: E402

DIMS = T.dims(128, 2, 2, 51865, 2)  # W = 4 frames: a window holds 640 samples at 16 kHz, 960 of the scripted engine's 24 kHz
TALK = [(3, QUIET), (2, LOUD), (2, QUIET), (3, LOUD), (9, QUIET)]  # test_csm_vad_cpu: the span is heard[72:336]
END_AT = 5  # every fake transcript is [1001 .. 1004]


class Engine(_Engine):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.cuts = []  # per span_windows call: [(ring length, start, samples)]

    def span_windows(self, spans, W, n_mels):
        assert (W, n_mels) == (2 * DIMS.n_audio_ctx, DIMS.n_mels)
        self.cuts.append([(int(r), int(s), int(n)) for _, r, s, n in spans])
        self.calls.append(("span_windows", len(spans)))
        out = np.zeros((len(spans), 4), np.float32)
        for i, (buf, r, s, n) in enumerate(spans):
            assert buf.ndim == 1
            out[i] = (r, s, n, float(buf[s % r if r else s]))
        return out


class Whisper(_Whisper):
    def __init__(self):
        super().__init__()
        self.dims, self.windows, self.end_at = DIMS, [], END_AT  # windows: every fake window that was encoded, by tag

    def embed_audio(self, win):
        self.log.append(("embed_audio", len(win)))
        x = np.zeros((len(win), DIMS.n_audio_ctx, DIMS.n_audio_state), np.float32)
        for i, w in enumerate(win):
            x[i, 0, 0], x[i, 0, 1] = self.end_at, len(self.windows)
            self.windows.append(tuple(float(v) for v in w))
        return x


def _pair(rows=2, lag=0, lmf=400, **kw):
    eng, wh = Engine(lag=lag), Whisper()
    stt = WhisperBatcher(engine=wh, max_rows=4, eos_check_interval=2)
    bat = _batcher(eng, listen_rows=rows, listen_chunk_frames=M, listen_max_frames=lmf, stt=stt, **kw)
    return eng, wh, stt, bat


def _tokens(res):
    assert isinstance(res, DecodingResult)
    return res.tokens


WANT = [1000 + k for k in range(1, END_AT)]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    bat = _batcher(Engine(), listen_rows=1, listen_chunk_frames=M, listen_max_frames=400)
    with pytest.raises(ValueError, match="stt="):
        bat.listen(transcribe=True)
    with pytest.raises(ValueError, match="stt="):
        bat.session().listen(1, vad=_cfg(), transcribe=DecodingOptions(language=0))
    assert bat.listen(transcribe=None).transcript is None  # (the row is taken, nothing else happened)
    bat.close()
    with pytest.raises(ValueError, match="stt_text needs stt="):
        _batcher(Engine(), listen_rows=1, stt_text=lambda r: r.tokens)
    started = WhisperBatcher(engine=Whisper(), max_rows=2).start()
    with pytest.raises(ValueError, match="start"):
        _batcher(Engine(), listen_rows=1, stt=started)
    started.close()
    eng, wh, stt, bat = _pair()
    with pytest.raises(ValueError, match="stt_rounds_per_round"):
        _batcher(Engine(), listen_rows=1, stt=stt, stt_rounds_per_round=0)
    for bad, exc in ((dict(temperature=0.5), NotImplementedError), (dict(beam_size=2), NotImplementedError), (dict(best_of=2), ValueError),
                     (DecodingOptions(prompt="text"), ValueError), (3, ValueError), ("en", ValueError)):
        with pytest.raises(exc):
            bat.listen(transcribe=bad)
    assert all(lis is None for lis in bat._listeners)  # a refused listen takes no row
    a, b = bat.listen(transcribe=True), bat.listen(vad=_cfg(), transcribe=dict(language=1, sample_len=7))
    assert a._topts == DecodingOptions() and b._topts.language == 1 and b._topts.sample_len == 7
    assert a._dev and not a.transcript.done() and not b.transcript.done()  # f32 at the model's rate: still read from the device buffer
    bat.close()
    stt.close()


# ---- stepping -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_round", [1, 3])
def test_at_most_n_stt_rounds_per_scheduling_round_and_none_when_idle(per_round):
    eng, wh, stt, bat = _pair(stt_rounds_per_round=per_round)
    assert not bat.step() and not wh.log  # idle: `stt` is not stepped
    x = np.zeros((DIMS.n_audio_ctx, DIMS.n_audio_state), np.float32)
    x[0, 0] = 9
    mine = stt.submit(x, language=0, sample_len=20)  # a window of the caller's own shares the batch
    stepped, step = [], stt.step
    stt.step = lambda: (stepped.append(1), step())[1]
    rounds = 0
    while not mine.done():
        before = len(stepped)
        assert bat.step() is True  # `stt` has work: due work
        assert 1 <= len(stepped) - before <= per_round
        rounds += 1
        assert rounds < 50
    assert _tokens(mine.result(timeout=0)) == [1000 + k for k in range(1, 9)]
    assert bat.stats["stt_rounds"] == len(stepped) > sum(e[0] == "forward" for e in wh.log) >= 9 and rounds >= 9 // per_round
    n = len(wh.log)
    assert bat.step() is False and len(wh.log) == n and not eng.cuts  # idle again
    bat.close()
    stt.close()


def test_the_worker_wakes_for_a_window_the_caller_submits():
    eng, wh, stt, bat = _pair()
    bat.start()
    x = np.zeros((DIMS.n_audio_ctx, DIMS.n_audio_state), np.float32)
    x[0, 0] = 3
    assert _tokens(stt.submit(x, language=0, sample_len=20).result(timeout=30)) == [1001, 1002]
    bat.close()
    assert not stt.closed and stt.on_submit is None
    stt.close()


# ---- one cut per round, in row order ----------------------------------------------------------------------------------------------------------
def test_a_rounds_spans_are_cut_together_and_submitted_in_row_order():
    talk = _clip([(1, QUIET), (2, LOUD), (6, QUIET)], 2)

    def run(end_b_before_round):
        """-> the rounds until the first cut; the listener without a detector is ended just before round `end_b_before_round`"""
        eng, wh, stt, bat = _pair(rows=3, lmf=LMF)  # (the ring of the continuous microphone is 240 samples)
        cfg = _cfg()
        mic = bat.listen(vad=cfg, continuous=True, transcribe=dict(language=0, sample_len=9))             # row 0
        a = bat.listen(vad=cfg, transcribe=dict(language=1, sample_len=8))                                 # row 1
        b = bat.listen(transcribe=DecodingOptions(language=2, sample_len=7))                               # row 2: no detector, `end()` closes it
        for lis in (mic, a, b):
            lis.feed(talk)
        fb, k = None, 0
        while not eng.cuts:
            if k == end_b_before_round:
                fb = b.end()
            assert bat.step() and k < 20
            k += 1
        return eng, wh, stt, bat, mic, a, b, fb, k

    *_, bat0, _, _, _, _, k = run(None)  # the detectors' endpoints are consumed in round k - 1 ...
    bat0.close()
    eng, wh, stt, bat, mic, a, b, fb, k2 = run(k - 1)  # ... so `end()` just before it closes the third span in the same round
    assert k2 == k and k > 1
    assert eng.cuts == [[(LMF * SPF, 24, 144), (0, 24, 144), (0, 0, talk.shape[0])]], "one launch for the round's three spans, in row order"
    assert [e for e in wh.log if e[0] == "embed_audio"] == [("embed_audio", 3)]
    assert wh.windows == [(LMF * SPF, 24.0, 144.0, float(talk[24])), (0.0, 24.0, 144.0, float(talk[24])), (0.0, 0.0, float(talk.shape[0]), float(talk[0]))]
    bat.run_until_idle()
    assert [e[2] for e in wh.log if e[0] == "admit"] == [0, 1, 2]  # submitted in row order
    got = []
    _drain(mic, got, end=False)
    assert len(got) == 1
    for h in (got[0][0], a, b):
        assert _tokens(h.transcript.result(timeout=0)) == WANT
    assert bat.stats["stt_cuts"] == 1 and bat.stats["stt_windows"] == 3
    assert [h._topts.language for h in (got[0][0], a, b)] == [0, 1, 2]  # the options are each listener's own
    assert fb.result(timeout=0).frames == -(-talk.shape[0] // SPF)
    assert a.end().done() is False
    bat.run_until_idle()
    mic.cancel()
    bat.close()
    stt.close()


def test_a_transcribing_listener_hears_what_a_plain_one_hears():
    res = []
    for kw in ({}, {"transcribe": dict(language=0)}):
        eng, wh, stt, bat = _pair(rows=1)
        lis = bat.listen(vad=_cfg(), **kw)
        clip = _clip(TALK, 5)
        for i in range(0, clip.shape[0], 7):
            lis.feed(clip[i : i + 7])
            bat.step()
        bat.run_until_idle()
        fut = lis.end()
        bat.run_until_idle()
        res.append((fut.result(timeout=0), lis.onset.result(timeout=0), lis.endpoint.result(timeout=0)))
        if kw:
            assert _tokens(lis.transcript.result(timeout=0)) == WANT and eng.cuts == [[(0, 72, 264)]]
        else:
            assert lis.transcript is None and not eng.cuts and not wh.log
        bat.close()
        stt.close()
    (r0, o0, e0), (r1, o1, e1) = res
    assert (o0, e0) == (o1, e1) and (r0.frames, r0.steps, r0.samples, r0.speech_start, r0.speech_stop) == (r1.frames, r1.steps, r1.samples, r1.speech_start, r1.speech_stop)
    np.testing.assert_array_equal(r0.codes.numpy(), r1.codes.numpy())


def test_no_speech_and_a_span_longer_than_a_window_fail_the_transcript_alone():
    eng, wh, stt, bat = _pair(rows=2)
    quiet, long_ = bat.listen(vad=_cfg(), transcribe=True), bat.listen(transcribe=dict(language=0))
    quiet.feed(_clip([(8, QUIET)], 3))
    long_.feed(np.full(961, 0.25, np.float32))  # 961 samples at 24 kHz are 641 at 16 kHz: one more than a window of 4 frames holds
    fq, fl = quiet.end(), long_.end()
    bat.run_until_idle()
    with pytest.raises(ValueError, match="no speech"):
        quiet.transcript.result(timeout=0)
    with pytest.raises(ValueError, match="no speech"):
        fq.result(timeout=0)
    with pytest.raises(ValueError, match="641 samples at 16 kHz"):
        long_.transcript.result(timeout=0)
    assert fl.result(timeout=0).frames == -(-961 // SPF)  # everything else about it went on as before
    assert not eng.cuts and not wh.log
    ok = bat.listen(transcribe=dict(language=0))
    ok.feed(np.full(960, 0.25, np.float32))
    ok.end()
    bat.run_until_idle()
    assert _tokens(ok.transcript.result(timeout=0)) == WANT and eng.cuts == [[(0, 0, 960)]]
    bat.close()
    stt.close()


# ---- cancel and close -------------------------------------------------------------------------------------------------------------------------
def test_cancel_before_and_after_the_cut():
    eng, wh, stt, bat = _pair(rows=2)
    early, late = bat.listen(transcribe=dict(language=0)), bat.listen(vad=_cfg(), transcribe=dict(language=0))
    early.feed(_clip(TALK, 1))
    late.feed(_clip(TALK, 2))
    bat.step()
    assert early.cancel() and early.transcript.cancelled()  # before the cut: its window is never made
    while not eng.cuts:
        assert bat.step()
    assert eng.cuts == [[(0, 72, 264)]] and not late.transcript.done()
    assert late.cancel() and late.transcript.cancelled()  # after the cut: the request runs out (or leaves the queue) and is dropped
    bat.run_until_idle()
    with pytest.raises(CancelledError):
        late.transcript.result(timeout=0)
    assert not wh.rows and not any(r is not None for r in stt._rows) and not stt._queue and not bat._stt_owed
    nxt = bat.listen(transcribe=dict(language=0))  # rows and batch go on
    nxt.feed(_clip(TALK, 3))
    nxt.end()
    bat.run_until_idle()
    assert _tokens(nxt.transcript.result(timeout=0)) == WANT
    bat.close()
    stt.close()


def test_close_fails_owed_transcripts_and_leaves_stt_open():
    eng, wh, stt, bat = _pair(rows=3)
    wh.end_at = 0  # a transcript that takes its whole sample_len: longer than the listener's last encode steps
    cut, uncut, open_ = (bat.listen(vad=_cfg(), transcribe=dict(language=0, sample_len=200)) for _ in range(3))
    cut.feed(_clip(TALK, 1))
    while not eng.cuts:
        assert bat.step()
    res = cut.end()
    while not res.done():
        assert bat.step()
    assert res.done() and not cut.transcript.done()  # the listener has resolved and left; Whisper still owes its transcript
    uncut.feed(_clip(TALK, 2)[:200])
    bat.step()
    bat.close()
    for lis in (cut, uncut, open_):
        with pytest.raises(RuntimeError, match="CSMBatcher is closed"):
            lis.transcript.result(timeout=0)
    assert not stt.closed and stt.on_submit is None
    x = np.zeros((DIMS.n_audio_ctx, DIMS.n_audio_state), np.float32)
    x[0, 0] = 2
    mine = stt.submit(x, language=0)  # `stt` is the caller's again
    stt.run_until_idle()
    assert _tokens(mine.result(timeout=0)) == [1001]
    stt.close()


# ---- a session's turn without typed text ------------------------------------------------------------------------------------------------------
def test_a_session_ends_without_text_when_stt_text_is_given():
    eng, wh, stt, bat = _pair(rows=1, stt_text=lambda r: [t - 1000 for t in r.tokens])
    sess = bat.session()
    lis = sess.listen(1, vad=_cfg(), transcribe=dict(language=0))
    lis.feed(_clip(TALK, 5))
    fut = lis.end()  # before the endpoint has even been seen: the turn waits for the span, its codes and its transcript
    assert sess.busy
    bat.run_until_idle()
    res = fut.result(timeout=0)
    assert sess.turns[-1] == (1, [1, 2, 3, 4], 0) and not sess.busy
    assert sess.history[0].shape[0] == 4 + res.frames + 1 and res.frames == 88
    # a continuous microphone's utterance likewise
    mic = sess.listen(1, vad=_cfg(), continuous=True, transcribe=dict(language=0))
    mic.feed(_clip([(1, QUIET), (2, LOUD), (6, QUIET)], 2))
    got = []
    for _ in range(20):
        bat.step()
        _drain(mic, got, end=True)
    bat.run_until_idle()
    assert len(got) == 1 and got[0][1].result(timeout=0).frames == 48 and sess.turns[-1] == (1, [1, 2, 3, 4], 0) and len(sess.turns) == 2
    mic.cancel()
    bat.close()
    stt.close()


def test_without_stt_text_the_refusal_stands():
    eng, wh, stt, bat = _pair(rows=1)
    sess = bat.session()
    lis = sess.listen(1, vad=_cfg(), transcribe=True)
    lis.feed(_clip(TALK, 5))
    with pytest.raises(ValueError, match="needs its text"):
        lis.end()
    assert not sess.busy
    fut = lis.end([9, 9])
    bat.run_until_idle()
    assert fut.result(timeout=0).frames == 88 and sess.turns[-1] == (1, [9, 9], 0)
    bat.close()
    stt.close()


def test_a_failed_transcript_fails_the_turn_and_leaves_the_session_as_it_was():
    eng, wh, stt, bat = _pair(rows=1, stt_text=lambda r: r.tokens)
    sess = bat.session()
    lis = sess.listen(1, transcribe=dict(language=0))
    lis.feed(np.full(961, 0.25, np.float32))  # longer than a window
    fut = lis.end()
    bat.run_until_idle()
    with pytest.raises(ValueError, match="16 kHz"):
        fut.result(timeout=0)
    assert not sess.busy and sess.turns == [] and sess.length == 0
    bat.close()
    stt.close()


# ---- feature off ------------------------------------------------------------------------------------------------------------------------------
def test_a_batcher_without_stt_makes_nothing_of_it():
    eng = Engine()
    bat = _batcher(eng, listen_rows=2, listen_chunk_frames=M, listen_max_frames=400)
    assert bat._stt is None and bat._stt_text is None and bat._stt_rounds is None and bat._stt_due is None and bat._stt_owed is None
    assert not any(k.startswith("stt") for k in bat.stats)
    plain, vad = bat.listen(), bat.listen(vad=_cfg())
    for lis in (plain, vad):
        assert lis.transcript is None and lis._topts is None and lis._twf is None
        lis.feed(_clip(TALK, 4))
    assert not plain._dev  # a plain f32 listener at the model's rate still feeds the encoder from the host
    fp = plain.end()
    bat.run_until_idle()
    fv = vad.end()
    bat.run_until_idle()
    assert fp.result(timeout=0).frames == 152 and fv.result(timeout=0).frames == 88
    assert not eng.cuts and not [c for c in eng.calls if c[0] == "span_windows"]
    bat.close()


def test_the_c_entry_refuses_before_it_launches():
    import ctypes as C

    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 27
    one = C.c_void_p(16)  # never dereferenced: every call below is refused on the host

    def call(R=1, buf_len=(1000,), ring=(0,), pos=(0,), n=(100,), W=200, L=2, M=3, T=31, n_mels=80, tab=one):
        k = max(len(n), 1)
        i32 = lambda v: (C.c_int32 * k)(*v)  # noqa: E731
        i64 = lambda v: (C.c_int64 * k)(*v)  # noqa: E731
        return lib.kk_op_log_mel_spans(None, R, (C.c_void_p * k)(*[16] * k), i64(buf_len), i32(ring), i64(pos), i32(n), W, L, M, tab, T, n_mels, one, one, one, one, one)

    for kw, msg in ((dict(R=0), b"outside [1, 32]"), (dict(R=33), b"outside [1, 32]"), (dict(W=2), b"W = 2"), (dict(n_mels=64), b"80 or 128"),
                    (dict(n=(0,)), b"n = 0"), (dict(n=(48001,), buf_len=(50000,)), b"row 0: 48001 samples are 32001 at 16 kHz"),
                    (dict(pos=(901,)), b"does not lie in its buffer"), (dict(pos=(-1,)), b"negative position"),
                    (dict(ring=(50,)), b"does not lie in its buffer"), (dict(ring=(2000,), n=(100,)), b"does not lie in its buffer"),
                    (dict(T=30), b"the taps of 2 / 3"), (dict(tab=None), b"the taps of 2 / 3"), (dict(L=1, M=6, T=121), b"1 / 6 is not served"),
                    (dict(L=0), b"must be >= 1")):
        assert call(**kw) != 0, kw
        assert msg in lib.kk_last_error(), (kw, lib.kk_last_error())
    with pytest.raises(ValueError, match="row 1"):
        whisper.check_spans([(None, 0, 0, 48000), (None, 0, 5, 48001)], 200, 24000)
    with pytest.raises(ValueError, match="1 / 6"):
        whisper.span_ratio(96000)
    with pytest.raises(ValueError, match="160 / 441"):
        whisper.span_ratio(44100)
    assert [whisper.span_ratio(r) for r in (8000, 12000, 16000, 24000, 32000, 48000)] == [(2, 1), (4, 3), (1, 1), (2, 3), (1, 2), (1, 3)]
