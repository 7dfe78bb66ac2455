"""Sampled rows in the running decoder batch (WhisperBatcher.submit_sampled, kk_whisper_text_rows_set_draw, the per-row branch of pick_rows_kernel;
DESIGN 8n): a request decoded at temperature > 0 inside a batch gets, field by field, the DecodingResult of `Model.sample` on its window alone with the
same seed and stream id, the greedy rows beside it keep the result of `Model.decode`, and a row is greedy again after a sampled request has left it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_ref as R  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

FIELDS = ("tokens", "avg_logprob", "no_speech_prob", "language", "temperature")
_cache = {}


def _model():
    if "m" not in _cache:
        d = T.dims(**T.SHAPE_A)
        _cache["m"] = (d, whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **T.decoder_weights(d, 21)}), T.features(d, 6, 61))
    return _cache["m"]


def _same(got, want):
    for f in FIELDS:
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))


# (window, options, seed, stream); temperature None: a greedy request
REQUESTS = [(0, dict(language=4, sample_len=10, temperature=0.2), 7, 41),
            (1, dict(language=2, sample_len=12, suppress_tokens=[7, 8]), 0, 0),
            (2, dict(language=None, sample_len=9, temperature=1.0, prompt=[1000, 1001]), 7, 5),
            (3, dict(language=4, sample_len=6, without_timestamps=True, prompt=[1000, 1001]), 0, 0),
            (4, dict(language=1, sample_len=11, temperature=1.0, without_timestamps=True), 2 ** 40 + 3, 2 ** 32 - 1),
            (5, dict(language=0, sample_len=8, temperature=0.2, best_of=1), 7, 41)]


def _solo(m, feats):
    if "solo" not in _cache:
        out = []
        for i, o, seed, stream in REQUESTS:
            if "temperature" in o:
                out.append(m.sample(feats[i], WD.DecodingOptions(**o), seed=seed, streams=[stream]))
            else:
                out.append(m.decode(feats[i], WD.DecodingOptions(**o)))
        _cache["solo"] = out
    return _cache["solo"]


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]])
def test_sampled_and_greedy_rows_of_one_batch_equal_their_solo_runs(order):
    d, m, feats = _model()
    solo = _solo(m, feats)
    assert any(len(r.tokens) >= 8 for r in solo) and {r.temperature for r in solo} == {0.0, 0.2, 1.0}
    with m.serve(max_rows=3, eos_check_interval=4) as s:
        futs = {}
        for i in order:
            w, o, seed, stream = REQUESTS[i]
            if "temperature" in o:
                futs[i] = s.submit_sampled(feats[w], WD.DecodingOptions(**o), seed=seed, stream=stream)
            else:
                futs[i] = s.submit(feats[w], WD.DecodingOptions(**o))
        s.run_until_idle()
        for i in order:
            _same(futs[i].result(timeout=1), solo[i])
        assert s.stats.admissions == 6 and s.stats.retired == 6  # three rows, each reused: greedy after sampled and sampled after greedy


def test_the_same_stream_draws_the_same_tokens_and_another_stream_others():
    d, m, feats = _model()
    opts = WD.DecodingOptions(language=4, sample_len=12, temperature=1.0)
    with m.serve(max_rows=4) as s:
        a = s.submit_sampled(feats[0], opts, seed=3, stream=9)
        b = s.submit_sampled(feats[0], opts, seed=3, stream=9)
        c = s.submit_sampled(feats[0], opts, seed=3, stream=10)
        e = s.submit_sampled(feats[0], opts, seed=4, stream=9)
        s.run_until_idle()
        a, b, c, e = (f.result(timeout=1) for f in (a, b, c, e))
    _same(a, b)
    assert c.tokens != a.tokens and e.tokens != a.tokens and len(a.tokens) > 1
    _same(c, m.sample(feats[0], opts, seed=3, streams=[10]))


def test_a_row_is_greedy_again_after_a_sampled_request():
    d, m, feats = _model()
    greedy = WD.DecodingOptions(language=4, sample_len=10)
    want = m.decode(feats[1], greedy)
    with m.serve(max_rows=1) as s:  # ONE row: the greedy request takes the row the sampled one leaves
        hot = s.submit_sampled(feats[1], WD.DecodingOptions(language=4, sample_len=10, temperature=1.0), seed=1, stream=2)
        cold = s.submit(feats[1], greedy)
        s.run_until_idle()
        assert hot.result(timeout=1).tokens != want.tokens
        _same(cold.result(timeout=1), want)
        with pytest.raises(NotImplementedError, match="temperature > 0 is not yet implemented"):
            s.submit(feats[1], temperature=0.5)
        with pytest.raises(NotImplementedError, match="best_of groups are not built in the batcher"):
            s.submit_sampled(feats[1], language=4, temperature=0.5, best_of=2)


def test_set_draw_refuses_a_row_that_was_never_admitted():
    from mlx_audio_amd import _lib

    d, m, feats = _model()
    with m.serve(max_rows=2) as s:
        rows = s.engine._rows
        with pytest.raises(_lib.KokoroHipError, match="never admitted"):
            rows.set_draw(1, 0.5, 0, 0)
        with pytest.raises(_lib.KokoroHipError, match="outside"):
            rows.set_draw(2, 0.5, 0, 0)
        with pytest.raises(_lib.KokoroHipError, match="temperature must be finite and > 0"):
            rows.set_draw(0, 0.0, 0, 0)
