"""Whisper sampling end to end on the device (mlx-audio_amd/whisper_sampling.py, csrc/kk_whisper_text.hip): a grouped state's logits against the
plain state with repeated features bit for bit, every sampled candidate replayed through the numpy filters and the sampled restatement on the model's own
logits, the ranker, a window alone against its rows of a batch, the temperature -> 0 limit against greedy `decode`, and the temperature fallback."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_ref as R  # noqa: E402
import _whisper_sample_ref as SR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd import whisper_sampling as WS  # noqa: E402

SHAPES = {"a": T.SHAPE_A, "b": T.SHAPE_B}
_cache = {}


def _model(name):
    if name not in _cache:
        d = T.dims(**SHAPES[name])
        m = whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **T.decoder_weights(d, 21)})
        assert m.has_text_decoder
        _cache[name] = (d, m)
    return _cache[name]


@pytest.mark.parametrize("name", ["a", "b"])
def test_a_grouped_state_gives_the_bits_of_repeated_features(name):
    """n_audio 2, G 3: a 4-token prefill and 3 steps, different tokens in every row, on ONE cross K/V slice per window, against set_audio with every
    window's features repeated 3 times; and the grouped state is smaller by the four slices it does not hold."""
    import torch

    d, m = _model(name)
    rt = m._text
    feats = torch.from_numpy(T.features(d, 2, 31)).to(m.device)
    toks = torch.from_numpy(np.random.default_rng(4).integers(0, d.n_vocab, (6, 7)).astype(np.int32)).to(m.device)

    def run(setup):
        with torch.cuda.device(m.device):
            setup()
            out = [rt.forward(toks[:, :4].contiguous(), True).cpu().numpy()]
            for s in range(4, 7):
                out.append(rt.forward(toks[:, s:s + 1].contiguous(), False).cpu().numpy())
        return out

    plain = run(lambda: rt.set_audio(feats.repeat_interleave(3, dim=0).contiguous()))
    grouped = run(lambda: rt.set_audio_groups(feats, 3))
    assert rt.B == 6
    for s, (a, b) in enumerate(zip(plain, grouped)):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"call {s}"
    assert not np.array_equal(plain[0][0], plain[0][1]) and not np.array_equal(plain[0][0], plain[0][3])  # rows of a window differ, windows differ
    lib = rt._lib
    small, big = lib.kk_whisper_text_state_bytes_groups(rt._h, 2, 3), lib.kk_whisper_text_state_bytes(rt._h, 6)
    assert small < big and big - small == d.n_text_layer * 4 * d.n_audio_ctx * 2 * d.n_text_state * 2
    from mlx_audio_amd._lib import KokoroHipError

    with torch.cuda.device(m.device):
        rt.set_audio_groups(feats, 3)
        with pytest.raises(KokoroHipError, match="n_group = 3"):  # the capturing forward runs on a plain state
            rt.forward_qk(toks[:, :2].contiguous(), [[0, 0]], d.n_audio_ctx)
        with pytest.raises(ValueError, match="n_group"):
            rt.set_audio_groups(feats, 9)
        rt.set_audio(feats)  # and the plain state is back for whoever comes next
        assert rt.B == 2


OPTS = WD.DecodingOptions(language=4, sample_len=11, temperature=1.0, best_of=3, prompt=[1000, 1001], suppress_tokens=[7, 8])
SEED = 7


@pytest.fixture(scope="module")
def sampled_a():
    """the candidates every test of shape a shares: 2 windows, best_of 3, and the model's own logits of every candidate's whole sequence"""
    d, m = _model("a")
    tok = whisper.special_tokens(d)
    feats = T.features(d, 2, 11)
    win = m.sample_candidates(feats, OPTS, seed=SEED, eos_check_interval=4)
    init = WD.initial_tokens(tok, OPTS, d.n_text_ctx, 11)
    flat = [c for group in win.candidates for c in group]
    n = max(len(c[0]) for c in flat)
    seq = np.array([list(init) + c[0] + [tok.eot] * (n - len(c[0])) for c in flat], np.int64)
    lg = m.logits(seq, np.repeat(feats, 3, axis=0)).cpu().numpy()  # the plain state's bits are the grouped state's, the prefill's are the steps'
    return dict(d=d, m=m, tok=tok, feats=feats, win=win, init=init, flat=flat, n=n, lg=lg)


def test_every_candidate_replays_through_the_filters_and_the_restatement(sampled_a):
    """Model.logits of each candidate's whole sequence, then the numpy filters, then the sampled restatement on stream a * 3 + g: each step's token is
    admissible (at most 2 % of the draws with more than one admissible token), sum_logprob within 1e-4, no_speech_prob the softmax at sot."""
    s = sampled_a
    d, tok, win, lg = s["d"], s["tok"], s["win"], s["lg"]
    assert len(win.candidates) == 2 and all(len(g) == 3 for g in win.candidates) and not win.single and win.temperature == 1.0
    assert win.languages == [tok.language_tokens[4]] * 2 and win.language_probs == [None, None]
    P = T.pick_params(tok, d.n_vocab, max_initial_timestamp_index=round(1.0 / (30 / d.n_audio_ctx)))
    sup = WD.suppress_list(tok, OPTS)
    S0 = len(s["init"])
    draws = multi = 0
    for b, (tokens, total) in enumerate(s["flat"]):
        row = SR.SampledRow(tok.eot, 1.0, SEED, b)  # streams default to 0, 1: row (a, g) draws on a * 3 + g = b
        for i in range(len(tokens) + (1 if len(tokens) < 11 else 0)):  # a candidate shorter than sample_len ended on a drawn eot
            want = tokens[i] if i < len(tokens) else tok.eot
            adm = row.update(T.filter_logits(lg[b, S0 - 1 + i], row.sampled, P, suppress=sup), want)
            assert adm is not None and want in adm, (b, i, want, adm)
        assert abs(total - row.sum_logprob) < 1e-4, (b, total, row.sum_logprob)
        draws, multi = draws + row.draws, multi + row.multi
    print(f"{multi} of {draws} draws had more than one admissible token")
    assert multi <= SR.CAP * draws
    assert len({tuple(c[0]) for c in s["flat"]}) > 1  # at temperature 1 the candidates are not one sequence six times
    for a in range(2):
        x = lg[3 * a, s["init"].index(tok.sot)].astype(np.float64)
        assert abs(win.no_speech_probs[a] - np.exp(x[tok.no_speech] - T.logsumexp(x))) < 1e-6


@pytest.mark.parametrize("length_penalty", [None, 0.6])
def test_sample_returns_the_ranked_candidate(sampled_a, length_penalty):
    s = sampled_a
    res = s["m"].sample(s["feats"], OPTS, seed=SEED, length_penalty=length_penalty)
    assert len(res) == 2
    for a, r in enumerate(res):
        group = s["win"].candidates[a]
        tokens, total = group[SR.rank(group, length_penalty)]
        assert WS.rank(group, length_penalty) == SR.rank(group, length_penalty)
        assert r.tokens == tokens and r.avg_logprob == total / (len(tokens) + 1) and r.temperature == 1.0 and r.text == "" and np.isnan(r.compression_ratio)
        assert r.language == s["tok"].language_tokens[4] and r.no_speech_prob == s["win"].no_speech_probs[a]


def test_a_window_alone_equals_its_rows_of_the_batch(sampled_a):
    s = sampled_a
    one = s["m"].sample_candidates(s["feats"][1], OPTS, seed=SEED, streams=[1])  # 2-D input
    assert one.single and one.candidates == [s["win"].candidates[1]] and one.no_speech_probs == [s["win"].no_speech_probs[1]]
    other = s["m"].sample_candidates(s["feats"][1], OPTS, seed=SEED)  # on stream 0 it draws other uniforms
    assert other.candidates != one.candidates
    r = s["m"].sample(s["feats"][1], OPTS, seed=SEED, streams=[1])
    assert isinstance(r, WD.DecodingResult) and r.tokens == s["m"].sample(s["feats"], OPTS, seed=SEED)[1].tokens


def test_the_limit_of_temperature_zero_is_greedy_decoding():
    """at T = 1e-4 the Gumbel noise (at most 16.64) is worth 0.0017 of a logit: the sampled tokens are `decode`'s; and language detection gives its ids"""
    d, m = _model("a")
    feats = T.features(d, 2, 12)
    greedy = m.decode(feats, sample_len=9)
    cold = m.sample(feats, sample_len=9, temperature=1e-4, seed=3)
    assert [r.tokens for r in cold] == [r.tokens for r in greedy] and [r.language for r in cold] == [r.language for r in greedy]
    assert all(abs(c.avg_logprob - g.avg_logprob) < 1e-6 and c.temperature == 1e-4 for c, g in zip(cold, greedy))
    assert all(max(c.language_probs, key=c.language_probs.get) == c.language for c in cold)
    assert all(abs(c.no_speech_prob - g.no_speech_prob) < 1e-7 for c, g in zip(cold, greedy))


def test_fallback_on_the_device():
    d, m = _model("a")
    feats = T.features(d, 2, 13)
    greedy = m.decode(feats, language=2, sample_len=7)
    res = m.decode_with_fallback(feats, logprob_threshold=None, language=2, sample_len=7, best_of=2)  # nothing needs fallback: decode's result, best_of dropped
    assert [r.tokens for r in res] == [r.tokens for r in greedy] and [r.avg_logprob for r in res] == [r.avg_logprob for r in greedy]
    assert all(r.temperature == 0.0 for r in res)
    last = m.decode_with_fallback(feats, temperature=(0.0, 0.5, 1.0), logprob_threshold=1.0, no_speech_threshold=None, seed=5, language=2, sample_len=7,
                                  best_of=2)  # an average log-probability is never above 0: every temperature runs, the last one's result stays
    want = m.sample(feats, language=2, sample_len=7, best_of=2, temperature=1.0, seed=5)
    assert [r.temperature for r in last] == [1.0, 1.0] and [r.tokens for r in last] == [r.tokens for r in want]
    one = m.decode_with_fallback(feats[1], temperature=0.5, logprob_threshold=1.0, no_speech_threshold=None, seed=5, language=2, sample_len=7)
    alone = m.sample(feats[1], language=2, sample_len=7, temperature=0.5, seed=5)  # a scalar temperature, a 2-D input: stream 0
    assert one.temperature == 0.5 and one.tokens == alone.tokens


def test_the_pinned_refusals_still_hold():
    d, m = _model("a")
    feats = T.features(d, 1, 14)
    with pytest.raises(NotImplementedError, match="temperature"):
        m.decode(feats, temperature=0.5)
    with pytest.raises(NotImplementedError, match="best_of"):
        m.decode(feats, temperature=0.5, best_of=3)
    with pytest.raises(ValueError, match="call decode"):
        m.sample(feats, temperature=0.0)
    res = m.decode(feats, language=0, sample_len=3)  # and greedy decoding runs after a sampled state has been used on the handle
    m.sample(feats, language=0, sample_len=3, temperature=0.7, best_of=2)
    again = m.decode(feats, language=0, sample_len=3)
    assert again[0].tokens == res[0].tokens and again[0].avg_logprob == res[0].avg_logprob
