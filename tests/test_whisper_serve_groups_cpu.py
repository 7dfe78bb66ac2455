"""Groups in the scheduler of whisper_serve.WhisperBatcher on a fake engine (no GPU): a group waits for its G rows at the head of the queue,
leaves all of them in one round, at the poll or at its own limit; the refusals at submit; the routing of beam_transcribe's windows; the refusals that
stay pinned; and the group entries of the C ABI on a handle without device state."""
import ctypes as C
import os
import sys
from concurrent.futures import Future

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_whisper_serve_cpu import DIMS, TOK, serve, window  # noqa: E402

from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd import whisper_transcribe as WT  # noqa: E402


def test_a_group_waits_for_its_rows_and_nothing_overtakes_it():
    """max_rows 4: two single requests run; a beam of 3 is the head of the queue with 2 rows free and waits; the single request behind it waits too, though
    a row is free for it; when the first single request retires the group takes rows 0, 2, 3, and the last request is admitted only behind it"""
    eng, s = serve(max_rows=4, eos_check_interval=1)
    a = s.submit(window(2, 0), language=0, sample_len=20)
    b = s.submit(window(6, 1), language=0, sample_len=20)
    g = s.submit_beam(window(3, 2), language=0, sample_len=20, beam_size=3)
    c = s.submit(window(2, 3), language=0, sample_len=20)
    s.step()
    assert [e[:2] for e in eng.log if e[0].startswith("admit")] == [("admit", 0), ("admit", 1)]
    s.run_until_idle()
    admits = [e for e in eng.log if e[0].startswith("admit")]
    assert admits == [("admit", 0, 0), ("admit", 1, 1), ("admit_group", (0, 2, 3), 2, True), ("admit", 0, 3)]
    assert admits[2][1][0] == 0  # the leader is the lowest free row
    assert eng.log.index(("read", 0, 0)) < eng.log.index(admits[2]) < eng.log.index(("read_group", (0, 2, 3), 2)) < eng.log.index(admits[3])
    r = g.result(timeout=1)
    assert r.tokens == [1001, 1002, 0] and r.avg_logprob == -1.0 / 4 and r.temperature == 0.0 and r.no_speech_prob == 0.25  # the ranker's choice among 3 finished
    assert len(a.result(1).tokens) == 1 and len(b.result(1).tokens) == 5 and len(c.result(1).tokens) == 1
    st = s.stats
    assert (st.admissions, st.groups, st.group_rows, st.groups_retired, st.retired) == (4, 1, 3, 1, 4)


def test_a_group_leaves_all_its_rows_in_one_round_at_the_poll_or_at_its_limit():
    eng, s = serve(max_rows=6, eos_check_interval=4)
    g1 = s.submit_beam(window(2, 0), language=0, sample_len=30, beam_size=3)      # complete at pick 2: found by the poll behind round 4
    g2 = s.submit_group(window(0, 1), language=0, sample_len=3, temperature=0.5, best_of=2, seed=5, stream=9)  # never ends: its own limit, 3 picks
    s.run_until_idle()
    reads = [e for e in eng.log if e[0] == "read_group"]
    assert reads == [("read_group", (3, 4), 1), ("read_group", (0, 1, 2), 0)]
    assert eng.counts == {1: 3, 0: 4} and s.stats.polls == 1 and not eng.rows and not eng.groups
    fw = [e[1] for e in eng.log if e[0] == "forward"]
    n = len(WD.initial_tokens(TOK, WD.DecodingOptions(language=0), DIMS.n_text_ctx, 30))
    assert [it[:4] for it in fw[0]] == [(r, 0, n, 0) for r in range(5)] and [it[4:] for it in fw[0]] == [(0, 1), (-1, 0), (-1, 0), (0, 1), (-1, 0)]
    assert [it[:4] for it in fw[1]] == [(r, n, 1, -1) for r in range(5)]
    assert [it[0] for it in fw[3]] == [0, 1, 2]  # round 4: the plain group has left, all of it
    picks = [e[1] for e in eng.log if e[0] == "pick"]
    assert picks[0] == (0, 1, 2, 3, 4) and picks[3] == (0, 1, 2)
    assert eng.groups == {} and g2.result(1).tokens == [1001, 1002, 1003] and g2.result(1).temperature == 0.5
    assert g1.result(1).tokens == [1001, 0]
    assert [e for e in eng.log if e[0] == "admit_group"] == [("admit_group", (0, 1, 2), 0, True), ("admit_group", (3, 4), 1, False)]


def test_the_groups_draws_and_its_detection_round():
    eng, s = serve(max_rows=4, eos_check_interval=8)
    g = s.submit_group(window(0, 0), sample_len=2, temperature=0.5, best_of=3, seed=11, stream=7)  # language None
    s.run_until_idle()
    fw = [e[1] for e in eng.log if e[0] == "forward"]
    assert fw[0] == ((0, 0, 1, 0, 0, 0),) and [it[0] for it in fw[1]] == [0, 1, 2]  # [sot] on the leader alone, then every row prefills
    assert [e for e in eng.log if e[0] == "detect_group"] == [("detect_group", (0, 1, 2), 1)]
    r = g.result(1)
    assert r.language == TOK.language_tokens[3] and r.language_probs[TOK.language_tokens[3]] == 0.5 and s.stats.detections == 1
    # (the draws: row g on stream * best_of + g)
    eng2, s2 = serve(max_rows=4)
    s2.submit_group(window(0, 0), language=0, sample_len=2, temperature=0.5, best_of=3, seed=11, stream=7)
    s2.step()
    assert eng2.groups[0]["draws"] == [(0.5, 11, 21), (0.5, 11, 22), (0.5, 11, 23)] and eng2.groups[0]["beam"] is False


def test_prefill_cost_counts_every_row_of_a_group():
    eng, s = serve(max_rows=8, eos_check_interval=8, max_round_tokens=30)
    prompt = list(range(6))  # 1 + 6 + 3 = 10 initial tokens
    s.submit_beam(window(0, 0), language=0, sample_len=2, beam_size=2, prompt=prompt)   # 20 tokens
    s.submit_beam(window(0, 1), language=0, sample_len=2, beam_size=2, prompt=prompt)   # 20 more: the next round
    s.run_until_idle()
    fw = [e[1] for e in eng.log if e[0] == "forward"]
    assert [[it[2] for it in items] for items in fw[:2]] == [[10, 10], [1, 1, 10, 10]]


def test_a_cancelled_queued_group_never_takes_rows():
    eng, s = serve(max_rows=2, eos_check_interval=1)
    a = s.submit(window(3, 0), language=0)
    g = s.submit_beam(window(2, 1), language=0, beam_size=2)
    c = s.submit(window(2, 2), language=0)
    assert s.step() and g.cancel() and not a.cancel()
    s.run_until_idle()
    assert [e[:3] for e in eng.log if e[0].startswith("admit")] == [("admit", 0, 0), ("admit", 1, 2)] and g.cancelled()
    assert len(c.result(1).tokens) == 1 and s.stats.groups == 0


def test_group_refusals_at_submit():
    eng, s = serve(max_rows=4)
    with pytest.raises(ValueError, match="a group of 5 rows does not fit max_rows = 4"):
        s.submit_beam(window(), language=0, beam_size=5)
    with pytest.raises(ValueError, match="a group of 5 rows does not fit max_rows = 4"):
        s.submit_group(window(), language=0, temperature=0.5, best_of=5)
    with pytest.raises(ValueError, match="fewer than beam_size = 4.*depends on when the poll runs"):
        s.submit_beam(window(), language=0, beam_size=4, patience=0.5)
    with pytest.raises(ValueError, match="must fit 32 bits"):
        s.submit_group(window(), language=0, temperature=0.5, best_of=3, stream=(2 ** 32) // 3)
    s.submit_group(window(), language=0, temperature=0.5, best_of=3, stream=(2 ** 32) // 3 - 1).cancel()
    with pytest.raises(ValueError, match="best_of >= 2"):
        s.submit_group(window(), language=0, temperature=0.5, best_of=1)
    with pytest.raises(ValueError, match="temperature 0"):
        s.submit_beam(window(), language=0, beam_size=2, temperature=0.5)
    with pytest.raises(ValueError, match="beam search needs beam_size"):
        s.submit_beam(window(), WD.DecodingOptions(language=0))
    with pytest.raises(ValueError, match="finite temperature > 0"):
        s.submit_group(window(), language=0, best_of=None, temperature=0.0)
    assert not [e for e in eng.log if e[0] != "close"]


def test_the_pinned_refusals_still_hold():
    eng, s = serve(max_rows=4)
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
        s.submit(window(), beam_size=4)
    with pytest.raises(NotImplementedError, match="temperature > 0 is not yet implemented"):
        s.submit(window(), temperature=0.5)
    with pytest.raises(NotImplementedError, match="best_of groups are not built in the batcher: submit_sampled takes best_of None or 1"):
        s.submit_sampled(window(), language=0, temperature=0.5, best_of=2)
    for kw, word in ((dict(beam_size=3), "beam search is not built in transcribe"), (dict(patience=1.0), "beam search is not built in transcribe"),
                     (dict(best_of=2), "best_of > 1 is not built in transcribe")):
        with pytest.raises(NotImplementedError, match=word):
            WT.check_transcribe_options(kw)
    WT.check_transcribe_options(dict(beam_size=3, best_of=2), beam=True)
    with pytest.raises(NotImplementedError, match="word_timestamps is not built"):
        WT.check_transcribe_options({}, word_timestamps=True, beam=True)


class FakeBatcher:
    def __init__(self):
        self.calls = []

    def _call(self, name, features, options, **kw):
        self.calls.append((name, options, kw))
        return Future()

    def submit(self, f, o, **kw):
        return self._call("submit", f, o, **kw)

    def submit_sampled(self, f, o, **kw):
        return self._call("submit_sampled", f, o, **kw)

    def submit_beam(self, f, o, **kw):
        return self._call("submit_beam", f, o, **kw)

    def submit_group(self, f, o, **kw):
        return self._call("submit_group", f, o, **kw)


def test_beam_transcribe_routes_the_temperatures_to_the_four_submit_methods():
    cold = WT.WindowRequest(seek=3000, size=3000, prompt=(5, 6), temperature_index=0, temperature=0.0)
    hot = WT.WindowRequest(seek=2 ** 25, size=3000, prompt=(), temperature_index=3, temperature=0.6)
    assert WT.group_stream(cold) == 48000 and WT.group_stream(hot) == (2 ** 29 + 3) % 2 ** 28 == 3
    b = FakeBatcher()
    kw = dict(language=2, prompt=[5, 6], sample_len=9)
    WT.submit_window(b, None, cold, kw, 7, beam_size=5, best_of=5, patience=1.5)
    WT.submit_window(b, None, cold, kw, 7, beam_size=None, best_of=5, patience=None)
    WT.submit_window(b, None, hot, kw, 7, beam_size=5, best_of=5, patience=1.5)
    WT.submit_window(b, None, hot, kw, 7, beam_size=5, best_of=None, patience=None)
    WT.submit_window(b, None, hot, kw, 7, beam_size=5, best_of=1, patience=None)
    names = [c[0] for c in b.calls]
    assert names == ["submit_beam", "submit", "submit_group", "submit_sampled", "submit_sampled"]
    o = b.calls[0][1]
    assert (o.beam_size, o.patience, o.best_of, o.temperature, o.language, o.prompt, o.sample_len) == (5, 1.5, None, 0.0, 2, [5, 6], 9) and b.calls[0][2] == {}
    o = b.calls[1][1]
    assert (o.beam_size, o.patience, o.best_of, o.temperature) == (None, None, None, 0.0)
    o = b.calls[2][1]
    assert (o.beam_size, o.patience, o.best_of, o.temperature) == (None, None, 5, 0.6) and b.calls[2][2] == dict(seed=7, stream=3)
    for c in b.calls[3:]:
        assert (c[1].beam_size, c[1].best_of, c[1].temperature) == (None, None, 0.6) and c[2] == dict(seed=7, stream=3)
    # the argument checks of beam_transcribe run before a model is touched
    from mlx_audio_amd import whisper

    m = whisper.Model(DIMS)
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        m.beam_transcribe(np.zeros(16000, np.float32))
    for kw2, word in ((dict(beam_size=9), "beam_size must be an integer in 1 .. 8"), (dict(beam_size=4, patience=0.5), "at least beam_size"),
                      (dict(beam_size=None, patience=1.0), "patience requires beam_size"), (dict(best_of=9), "best_of must be in 1 .. 8"),
                      (dict(beam_size=5, max_rows=4), "cannot hold a group of 5 rows")):
        with pytest.raises(ValueError, match=word):
            WT.beam_transcribe(m, np.zeros(16000, np.float32), **kw2)


def test_the_group_entries_of_the_library_without_a_gpu():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 26 and (_lib.WHISPER_GROUP_PLAIN, _lib.WHISPER_GROUP_BEAM) == (0, 1)
    cfg = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=1, n_audio_ctx=1500, n_audio_state=384)
    h = C.c_void_p()
    assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**cfg)), C.byref(h)) == 0
    assert lib.kk_whisper_text_rows_groups_state_bytes(h, 0) == 0 and lib.kk_whisper_text_rows_groups_state_bytes(h, _lib.WHISPER_MAX_ROWS + 1) == 0
    n4 = lib.kk_whisper_text_rows_groups_state_bytes(h, 4)
    assert n4 > 4 * (2 * 448 + 16 * 448 + 2 * 9) * 4  # two owner rows, the finished stores and the offers of every row
    assert lib.kk_whisper_text_rows_state_bytes(h, 4) == lib.kk_whisper_text_rows_state_bytes(h, 4)  # (the row state's size is not the groups' business)
    buf = C.create_string_buffer(64)
    z = np.zeros(4, np.int32)
    params = _lib.KKWhisperPickParams(n_vocab=51865, eot=50257)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    calls = [lambda: lib.kk_whisper_text_rows_groups_bind(h, None, C.cast(buf, C.c_void_p), 64),
             lambda: lib.kk_whisper_text_rows_admit_group(h, None, p(z), 2, 1, C.cast(buf, C.c_void_p), p(z), 1, C.byref(params), None, 2, C.cast(buf, C.c_void_p), 64),
             lambda: lib.kk_whisper_text_rows_group_read(h, None, 0, 4, p(z), p(z), p(z), p(z), p(z), p(z), p(z), None),
             lambda: lib.kk_whisper_text_rows_group_offers(h, None, 0, p(z), p(z))]
    for call in calls:
        assert call() != 0 and b"row mode not opened" in lib.kk_last_error(), lib.kk_last_error()
    assert lib.kk_whisper_text_rows_group_release(h, 0) != 0 and b"groups are not bound" in lib.kk_last_error()
    assert lib.kk_whisper_text_rows_group_release(None, 0) != 0 and b"null model" in lib.kk_last_error()
    lib.kk_whisper_text_destroy(h)
