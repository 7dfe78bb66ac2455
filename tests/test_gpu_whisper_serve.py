"""Whisper serving on the device (mlx-audio_amd/whisper_serve.py, whisper_decoding.RowRuntime, kk_whisper_text_rows_*): every request of a
running batch gets, field by field, the DecodingResult of `Model.decode` on its window alone -- whatever else the batch runs, in whatever order the
requests arrive, whichever row they land in -- and the window mode of the same model keeps working between the rounds."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_ref as R  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

SHAPES = {"a": T.SHAPE_A, "b": T.SHAPE_B}
FIELDS = ("tokens", "avg_logprob", "no_speech_prob", "language", "language_probs", "temperature")
_cache = {}

OPTS_A = [dict(sample_len=3, language=4),
          dict(sample_len=9, language=4, without_timestamps=True, prompt=[1000, 1001]),
          dict(sample_len=6, language=None, prefix=[50, 51, 52]),
          dict(sample_len=12, language=2, suppress_tokens=[7, 8]),
          dict(sample_len=4, task="lang_id"),
          dict(sample_len=7, language=None, without_timestamps=True, prompt=[1000, 1001])]
OPTS_B = [dict(sample_len=5, language=4), dict(sample_len=4, language=None, without_timestamps=True), dict(sample_len=6, language=1, prompt=[1000, 1001])]


def _model(name, eot_bias=False):
    """(dims, Model with encoder + decoder), once per shape.  eot_bias: the final LayerNorm replaced by a constant that points at eot's embedding, so
    that every position's best token is eot (the construction of test_gpu_whisper_decoder)"""
    key = (name, eot_bias)
    if key not in _cache:
        d = T.dims(**SHAPES[name])
        w = T.decoder_weights(d, 21)
        if eot_bias:
            w = dict(w)
            w["decoder.ln.weight"] = np.zeros_like(w["decoder.ln.weight"])
            w["decoder.ln.bias"] = R.bf16_round(4.0 * w["decoder.token_embedding.weight"][whisper.special_tokens(d).eot])
        _cache[key] = (d, whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **w}))
    return _cache[key]


def _solo(name, m, feats, opts, eot_bias=False):
    """m.decode of every window alone, once per set"""
    key = ("solo", name, eot_bias, len(opts))
    if key not in _cache:
        _cache[key] = [m.decode(feats[i], WD.DecodingOptions(**o)) for i, o in enumerate(opts)]
    return _cache[key]


def _same(got, want):
    """the six fields with ==; a field that is nan on both sides (lang_id leaves the logprob fields unset) counts as equal"""
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a == b or (isinstance(a, float) and a != a and b != b), (f, a, b)


@pytest.mark.parametrize("name,opts,max_tokens", [("a", OPTS_A, 12), ("b", OPTS_B, 6)])
def test_every_request_equals_its_solo_decode_in_any_order(name, opts, max_tokens):
    d, m = _model(name)
    feats = T.features(d, len(opts), 31)
    solo = _solo(name, m, feats, opts)
    assert any(len(r.tokens) == max_tokens for r in solo) and all(r.language_probs is None for r, o in zip(solo, opts) if o.get("task") != "lang_id")
    for order in (list(range(len(opts))), list(range(len(opts)))[::-1]):
        with m.serve(max_rows=2, eos_check_interval=4) as s:
            admitted, admit = [], s.engine.admit

            def spy(rows, x, *more, admit=admit, admitted=admitted):
                assert len(rows) == 1
                admitted.append((rows[0], next(i for i in order if x is feats_in[i])))
                return admit(rows, x, *more)

            s.engine.admit = spy
            feats_in = {i: feats[i] for i in order}
            futs = {i: s.submit(feats_in[i], WD.DecodingOptions(**opts[i])) for i in order}
            s.run_until_idle()
            for i in order:
                _same(futs[i].result(timeout=1), solo[i])
            assert [i for _, i in admitted] == order and {r for r, _ in admitted} == {0, 1}  # FIFO, on two rows that are reused
            assert s.stats.admissions == len(opts) and s.stats.retired == len(opts) and s.stats.detections == sum(1 for o in opts if not o.get("language"))


def test_a_mel_goes_through_the_encoder_as_the_solo_call_does():
    d, m = _model("a")
    mel = np.random.default_rng(0).standard_normal((2 * d.n_audio_ctx, d.n_mels)).astype(np.float32)
    opts = WD.DecodingOptions(language=3, sample_len=5)
    want = m.decode(mel, opts)
    with m.serve(max_rows=2) as s:
        f = s.submit(mel, opts)
        g = s.submit(T.features(d, 1, 2)[0], language=1, sample_len=3)  # beside a row of features
        s.run_until_idle()
        _same(f.result(timeout=1), want)
        assert len(g.result(timeout=1).tokens) == 3


def test_rows_that_end_early_are_retired_at_the_next_poll():
    """Every position prefers eot: a row's first pick is a timestamp (eot is masked there), its second is eot.  Round order (whisper_serve): poll and
    retire, admit, forward, pick.  Six requests on two rows are three generations per row; a generation is the prefill round, the step round whose
    pick ends the row, and at most eos_check_interval further rounds until a poll is due -- the poll, the retirement and the next admission share the
    round that follows.  So fewer than 3 * (2 + eos_check_interval) + 1 rounds; running every row to its limit would take 3 * 224."""
    d, m = _model("a", eot_bias=True)
    tok = whisper.special_tokens(d)
    feats = T.features(d, 6, 13)
    opts = [dict(language=0)] * 6
    solo = _solo("a", m, feats, opts, eot_bias=True)
    interval = 3
    with m.serve(max_rows=2, eos_check_interval=interval) as s:
        futs = [s.submit(feats[i], language=0) for i in range(6)]
        s.run_until_idle()
        for f, want in zip(futs, solo):
            r = f.result(timeout=1)
            assert len(r.tokens) == 1 and r.tokens[0] >= tok.timestamp_begin
            _same(r, want)
        assert s.stats.rounds < 3 * (2 + interval) + 1, s.stats
        assert s.stats.polls == 3 and s.stats.ended_row_rounds > 0


def test_window_mode_keeps_working_beside_live_rows():
    d, m = _model("a")
    feats = T.features(d, 3, 41)
    opts = [dict(language=4, sample_len=10), dict(language=None, sample_len=8)]
    solo = [m.decode(feats[i], WD.DecodingOptions(**o)) for i, o in enumerate(opts)]
    wopts = WD.DecodingOptions(language=2, sample_len=6, prompt=[1000, 1001])
    want_decode, want_lang = m.decode(feats[2], wopts), m.detect_language(feats[2])
    with m.serve(max_rows=2, eos_check_interval=4) as s:
        futs = [s.submit(feats[i], WD.DecodingOptions(**o)) for i, o in enumerate(opts)]
        assert s.step() and s.step() and s.step() and not any(f.done() for f in futs)
        _same(m.decode(feats[2], wopts), want_decode)
        assert m.detect_language(feats[2]) == want_lang
        s.run_until_idle()
        for f, want in zip(futs, solo):
            _same(f.result(timeout=1), want)


def test_submits_from_three_threads_into_a_started_batcher():
    d, m = _model("a")
    feats = T.features(d, 8, 51)
    opts = [dict(language=(i % 3) if i % 4 else None, sample_len=3 + i, without_timestamps=bool(i & 1)) for i in range(8)]
    solo = [m.decode(feats[i], WD.DecodingOptions(**o)) for i, o in enumerate(opts)]
    s = m.serve(max_rows=3, eos_check_interval=4).start()
    futs = {}

    def client(ids):
        for i in ids:
            futs[i] = s.submit(feats[i], WD.DecodingOptions(**opts[i]))

    threads = [threading.Thread(target=client, args=(ids,)) for ids in ([0, 3, 6], [1, 4, 7], [2, 5])]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=30)
    try:
        for i in range(8):
            _same(futs[i].result(timeout=60), solo[i])
    finally:
        s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.submit(feats[0], language=0)
