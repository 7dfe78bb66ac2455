"""The Whisper text decoder end to end on the device (mlx-audio_amd/whisper.py, whisper_decoding.py, csrc/kk_whisper_text.hip): `Model.logits`
against transformers' WhisperDecoder in fp32 on the CPU carrying the same bf16-pre-rounded weights, the step against the prefill and a row against its
batch bit for bit, `detect_language`, and greedy `decode` replayed through the numpy restatement of the filters on the model's own logits."""
import os
import sys

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
_cache = {}


def _model(name, eot_bias=False):
    """(dims, weights, Model with encoder + decoder, HF decoder); built once per shape.  eot_bias: the final LayerNorm replaced by a constant that points
    at eot's embedding, so that every position's best token is eot"""
    key = (name, eot_bias)
    if key not in _cache:
        d = T.dims(**SHAPES[name])
        w = T.decoder_weights(d, 21)
        if eot_bias:
            w = dict(w)
            w["decoder.ln.weight"] = np.zeros_like(w["decoder.ln.weight"])
            w["decoder.ln.bias"] = R.bf16_round(4.0 * w["decoder.token_embedding.weight"][whisper.special_tokens(d).eot])
        m = whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **w})
        assert m.has_text_decoder
        _cache[key] = (d, w, m, None if eot_bias else T.hf_decoder(d, w))
    return _cache[key]


def _tokens(d, B, S, seed):
    return np.random.default_rng(seed).integers(0, d.n_vocab, (B, S)).astype(np.int64)


@pytest.mark.parametrize("S", [1, 5, 37])
@pytest.mark.parametrize("name", ["a", "b"])
def test_logits_against_the_fp32_reference(name, S):
    """B = 2.  The relative rms error against transformers' fp32 decoder is at most 1.5 x that of the reference's own CPU bf16 run on the same input:
    the device keeps the weights and the K/V in bf16 and rounds every Linear's input to bf16, but its residual stream, LayerNorms, softmax and
    accumulations are fp32, where the bf16 run rounds those too."""
    d, w, m, dec = _model(name)
    toks, feats = _tokens(d, 2, S, S), T.features(d, 2, 7)
    ref = T.hf_logits(dec, toks, feats)
    own = R.rel_rms(T.hf_logits(dec, toks, feats, bf16=True), ref)
    got = m.logits(toks, feats).cpu().numpy()
    assert got.shape == (2, S, d.n_vocab) and np.isfinite(got).all()
    err = R.rel_rms(got, ref)
    print(f"shape {name} S {S}: rel rms {err:.5f}, the reference's bf16 run {own:.5f}, ratio {err / own:.3f}, max abs {np.abs(got - ref).max():.4f}")
    assert err <= 1.5 * own


@pytest.mark.parametrize("name", ["a", "b"])
def test_steps_equal_the_prefill_and_a_row_equals_its_batch_bit_for_bit(name):
    """4 tokens of prefill and then 5 single-token steps give, position by position, the bits of one 9-token forward (the same kernels at other M / R,
    the K/V read back from the bf16 cache either way); row 1 alone gives the bits it has in the batch of 2; beyond n_text_ctx is an error, not a fault."""
    import torch

    d, w, m, _ = _model(name)
    toks, feats = _tokens(d, 2, 9, 3), T.features(d, 2, 8)
    full = m.logits(toks, feats).cpu().numpy()
    rt = m._text
    fd = torch.from_numpy(feats).to(m.device)
    td = torch.from_numpy(toks.astype(np.int32)).to(m.device)
    with torch.cuda.device(m.device):
        rt.set_audio(fd)
        pre = rt.forward(td[:, :4].contiguous(), True).cpu().numpy()
        assert np.array_equal(pre, full[:, :4])
        for s in range(4, 9):
            last = rt.forward(td[:, s:s + 1].contiguous(), False).cpu().numpy()
            assert np.array_equal(last, full[:, s]), f"step at position {s}"
        rt.rewind(0)
        assert np.array_equal(rt.forward(td[:, :6].contiguous(), False).cpu().numpy(), full[:, 5])  # last position only, after a rewind
    alone = m.logits(toks[1:], feats[1:]).cpu().numpy()
    assert np.array_equal(alone[0], full[1])
    with pytest.raises(ValueError):
        m.logits(_tokens(d, 1, d.n_text_ctx + 1, 0), feats[:1])
    from mlx_audio_amd._lib import KokoroHipError

    with torch.cuda.device(m.device):
        rt.set_audio(fd)
        rt.forward(torch.zeros((2, d.n_text_ctx - 1), dtype=torch.int32, device=m.device), False)
        with pytest.raises(KokoroHipError, match="exceeds n_text_ctx"):
            rt.forward(td[:, :2].contiguous(), False)


def test_detect_language():
    d, w, m, _ = _model("a")
    tok = whisper.special_tokens(d)
    feats = T.features(d, 2, 9)
    ids, probs = m.detect_language(feats)
    lg = m.logits(np.full((2, 1), tok.sot), feats).cpu().numpy()[:, 0].astype(np.float64)
    lo, hi = tok.language_tokens[0], tok.language_tokens[-1] + 1
    assert [int(i) for i in ids.cpu()] == [lo + int(np.argmax(lg[b, lo:hi])) for b in range(2)]
    for b in range(2):
        p = np.exp(lg[b, lo:hi] - T.logsumexp(lg[b, lo:hi]))
        assert set(probs[b]) == set(tok.language_tokens) and abs(sum(probs[b].values()) - 1.0) < 1e-5
        assert max(abs(probs[b][t] - p[t - lo]) for t in tok.language_tokens) < 1e-6
    one, p1 = m.detect_language(feats[1])  # 2-D input: one id, one dict
    assert one == int(ids[1]) and p1 == probs[1]
    mel = np.random.default_rng(0).standard_normal((2 * d.n_audio_ctx, d.n_mels)).astype(np.float32)  # a mel goes through the encoder first
    assert m.detect_language(mel)[0] in tok.language_tokens
    en = T.dims(128, 2, 1, 51864, 100)
    m_en = whisper.Model(en).load_weights({**R.encoder_weights(en, 5), **T.decoder_weights(en, 2)})
    with pytest.raises(ValueError, match="doesn't have language tokens"):
        m_en.detect_language(feats)
    with pytest.raises(ValueError, match="doesn't have language tokens"):  # (decoding.py:561: language None means detection)
        m_en.decode(feats)


def _replay(m, d, feats, init_rows, results, options):
    """the sampled tokens of `results` re-derived from Model.logits of the whole sequence through the numpy filters: exact, the step's logits being the
    prefill's bit for bit"""
    tok = whisper.special_tokens(d)
    P = T.pick_params(tok, d.n_vocab, without_timestamps=options.without_timestamps, suppress_blank=options.suppress_blank,
                      max_initial_timestamp_index=None if options.without_timestamps or not options.max_initial_timestamp
                      else round(options.max_initial_timestamp / (30 / d.n_audio_ctx)))
    sup = WD.suppress_list(tok, options) if options.suppress_tokens else ()
    n = max(len(r.tokens) for r in results)
    seq = np.array([list(init_rows[b]) + r.tokens + [tok.eot] * (n - len(r.tokens)) for b, r in enumerate(results)], np.int64)
    lg = m.logits(seq, feats).cpu().numpy()
    S0 = len(init_rows[0])
    for b, r in enumerate(results):
        row = T.GreedyRow(tok.eot)
        for i in range(len(r.tokens) + (1 if len(r.tokens) < n else 0)):
            row.update(T.filter_logits(lg[b, S0 - 1 + i], row.sampled, P, suppress=sup))
        want = row.sampled[: row.sampled.index(tok.eot)] if tok.eot in row.sampled else row.sampled
        assert r.tokens == want, (b, r.tokens, want)
        assert abs(r.avg_logprob - row.sum_logprob / (len(want) + 1)) < 1e-4
    return lg


@pytest.mark.parametrize("name,without_timestamps", [("a", False), ("b", True)])
def test_greedy_decode_replays_through_the_numpy_filters(name, without_timestamps):
    d, w, m, _ = _model(name)
    tok = whisper.special_tokens(d)
    feats = T.features(d, 2, 11)
    opts = WD.DecodingOptions(language=4, sample_len=11, without_timestamps=without_timestamps, prompt=[1000, 1001], suppress_tokens=[7, 8])
    res = m.decode(feats, opts, eos_check_interval=4)
    assert len(res) == 2 and all(len(r.tokens) == 11 and r.language == tok.language_tokens[4] and r.text == "" and r.temperature == 0.0 for r in res)
    init = WD.initial_tokens(tok, opts, d.n_text_ctx, 11)
    assert init[0] == tok.sot_prev and init[3] == tok.sot
    lg = _replay(m, d, feats, [init, init], res, opts)
    for b in range(2):  # no_speech_prob: the softmax at the sot position (decoding.py:595-597)
        x = lg[b, 3].astype(np.float64)
        assert abs(res[b].no_speech_prob - np.exp(x[tok.no_speech] - T.logsumexp(x))) < 1e-6
    if not without_timestamps:
        assert all(tok.timestamp_begin <= r.tokens[0] <= tok.timestamp_begin + round(1.0 / (30 / d.n_audio_ctx)) for r in res)  # max_initial_timestamp
    one = m.decode(feats[1], opts)  # 2-D input: one result, the bits of its row in the batch
    assert one.tokens == res[1].tokens and one.avg_logprob == res[1].avg_logprob


def test_decode_detects_the_language_and_lang_id_returns_early():
    d, w, m, _ = _model("a")
    tok = whisper.special_tokens(d)
    feats = T.features(d, 2, 12)
    ids, probs = m.detect_language(feats)
    res = m.decode(feats, sample_len=5)
    assert [r.language for r in res] == [int(i) for i in ids.cpu()]
    opts = WD.DecodingOptions(sample_len=5)
    init = [(tok.sot, r.language, tok.transcribe) for r in res]
    _replay(m, d, feats, init, res, opts)
    lid = m.decode(feats, task="lang_id")
    assert [r.language for r in lid] == [r.language for r in res] and lid[0].language_probs == probs[0] and lid[0].tokens == []
    with pytest.raises(NotImplementedError, match="temperature"):
        m.decode(feats, temperature=0.5)
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        m.generate(feats)


def test_decode_stops_when_every_row_has_ended():
    """a decoder whose every position prefers eot: the first sampled token must be a timestamp (eot is masked there), the second is eot, and the loop
    ends at the next look at the device counter instead of running to sample_len"""
    d, w, m, _ = _model("a", eot_bias=True)
    tok = whisper.special_tokens(d)
    feats = T.features(d, 3, 13)
    res = m.decode(feats, language=0, eos_check_interval=3)
    assert all(len(r.tokens) == 1 and r.tokens[0] >= tok.timestamp_begin for r in res)
    toks, rows = m._text.read()
    assert [r.count for r in rows] == [4, 4, 4] and all(r.ended for r in rows) and m._text.not_ended() == 0  # 1 + 3 steps, not 224
    assert all(list(toks[b, 1:4]) == [tok.eot] * 3 for b in range(3))
    assert all(np.isfinite(r.avg_logprob) and r.avg_logprob == rows[b].sum_logprob / 2 for b, r in enumerate(res))
