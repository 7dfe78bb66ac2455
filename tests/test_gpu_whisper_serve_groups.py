"""Beam search and best_of groups in the running decoder batch (WhisperBatcher.submit_beam / submit_group, kk_whisper_text_rows_admit_group),
end to end on the device: every request of a mixed batch -- beam groups, a best_of group, a greedy and a sampled row -- gets, field by field, the
DecodingResult of its solo call (`Model.beam_search`, `Model.sample`, `Model.decode`), in either submission order and with so few rows that groups
wait and rows change kinds.  The model, the options (`plain`, and `narrow` so that sequences do finish and groups complete) and the feature seeds are
those of tests/test_gpu_whisper_beam.py: device results are compared with device results by ==, so no margin condition arises here."""
import os
import sys
from dataclasses import replace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_text_ref as T  # noqa: E402
from test_gpu_whisper_beam import FEAT_SEED, K, _model, options  # noqa: E402

from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

FIELDS = ("tokens", "avg_logprob", "no_speech_prob", "language", "language_probs", "temperature")
_cache = {}


def _same(got, want):
    for f in FIELDS:
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))


def _requests():
    """(kind, window, options, seed, stream) and the solo results, once"""
    if "req" not in _cache:
        d, m = _model()
        plain, narrow = T.features(d, 2, FEAT_SEED["plain"]), T.features(d, 2, FEAT_SEED["narrow"])
        hot = WD.DecodingOptions(language=4, sample_len=10, temperature=0.7, best_of=3, prompt=[1000, 1001])
        reqs = [("beam", plain[0], options("plain"), 0, 0),
                ("beam", narrow[1], options("narrow"), 0, 0),
                ("group", plain[1], hot, 7, 41),
                ("greedy", narrow[0], WD.DecodingOptions(language=2, sample_len=12, suppress_tokens=[7, 8]), 0, 0),
                ("sampled", plain[0], WD.DecodingOptions(language=4, sample_len=9, temperature=1.0), 3, 5)]
        solo = []
        for kind, x, o, seed, stream in reqs:
            if kind == "beam":
                solo.append(m.beam_search(x, o))
            elif kind == "greedy":
                solo.append(m.decode(x, o))
            else:
                solo.append(m.sample(x, o, seed=seed, streams=[stream]))
        _cache["req"] = (reqs, solo)
    return _cache["req"]


def _submit(s, req):
    kind, x, o, seed, stream = req
    if kind == "beam":
        return s.submit_beam(x, o)
    if kind == "group":
        return s.submit_group(x, o, seed=seed, stream=stream)
    if kind == "sampled":
        return s.submit_sampled(x, o, seed=seed, stream=stream)
    return s.submit(x, o)


@pytest.mark.parametrize("max_rows", [8, 4])
@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]])
def test_every_request_of_a_mixed_batch_equals_its_solo_call(order, max_rows):
    """Two beam groups of 3, a best_of group of 3, a greedy and a sampled row.  max_rows 8: two groups run side by side and the third waits at the head of
    the queue; max_rows 4: one group at a time beside one single row, and every row is reused across kinds."""
    d, m = _model()
    reqs, solo = _requests()
    assert all(len(r.tokens) > 0 for r in solo)
    with m.serve(max_rows=max_rows, eos_check_interval=4) as s:
        futs = {i: _submit(s, reqs[i]) for i in order}
        s.run_until_idle()
        for i in order:
            _same(futs[i].result(timeout=1), solo[i])
        st = s.stats
        assert (st.admissions, st.retired, st.groups, st.group_rows, st.groups_retired) == (5, 5, 3, 9, 3)
    assert m.decode(reqs[3][1], reqs[3][2]).tokens == solo[3].tokens  # window mode is itself again behind the batcher


def test_language_detection_on_the_leader_and_beam_one():
    d, m = _model()
    feats = T.features(d, 2, FEAT_SEED["plain"])
    auto = replace(options("plain"), language=None)
    one = WD.DecodingOptions(language=4, sample_len=9, prompt=[1000, 1001], suppress_tokens=[7, 8], beam_size=1)
    want_auto, want_one = m.beam_search(feats[1], auto), m.beam_search(feats[0], one)
    greedy = m.decode(feats[0], replace(one, beam_size=None))
    hot = WD.DecodingOptions(sample_len=8, temperature=0.5, best_of=2)
    want_hot = m.sample(feats[0], hot, seed=1, streams=[3])
    with m.serve(max_rows=6, eos_check_interval=4) as s:
        a, b, c = s.submit_beam(feats[1], auto), s.submit_beam(feats[0], one), s.submit_group(feats[0], hot, seed=1, stream=3)
        s.run_until_idle()
        _same(a.result(timeout=1), want_auto)
        _same(b.result(timeout=1), want_one)
        _same(c.result(timeout=1), want_hot)
        assert s.stats.detections == 2
    assert want_auto.language_probs and want_hot.language_probs and b.result().tokens == greedy.tokens and len(greedy.tokens) > 0


def test_a_group_retired_early_frees_its_rows_and_window_mode_works_between_rounds():
    """max_rows 3: the narrow beam (it completes and is retired at a poll, long before its limit) holds every row; the plain beam queued behind it takes
    the same three rows.  Between the rounds window mode runs a beam search and a greedy decode on the same handle."""
    d, m = _model()
    reqs, solo = _requests()
    long_narrow = replace(options("narrow"), sample_len=40)
    x = T.features(d, 2, FEAT_SEED["narrow"])[0]
    want = m.beam_search(x, long_narrow)
    with m.serve(max_rows=3, eos_check_interval=2) as s:
        a, b = s.submit_beam(x, long_narrow), s.submit_beam(reqs[0][1], reqs[0][2])
        rounds, left_at = 0, None
        while s.step():
            rounds += 1
            if left_at is None and a.done():
                left_at = rounds
            if rounds == 3:
                _same(m.beam_search(reqs[0][1], reqs[0][2]), solo[0])
                _same(m.decode(reqs[3][1], reqs[3][2]), solo[3])
        _same(a.result(timeout=1), want)
        _same(b.result(timeout=1), solo[0])
        print(f"the narrow beam left after {left_at} rounds of its 40; {rounds} rounds in all")
        assert s.stats.polls >= 1 and left_at is not None and left_at < 40  # the first group left at a poll, not at its limit of 40 picks
        assert s.stats.groups == 2 and s.stats.group_rows == 2 * K
