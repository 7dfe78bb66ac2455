"""Whisper beam search end to end on the device (mlx-audio_amd/whisper_beam.py, csrc/kk_whisper_text.hip): every candidate's sum replayed
from the model's own logits of its whole sequence, the numpy restatement driven step by step by the model's logits of ITS OWN live prefixes, beam 1
against greedy `decode`, a window alone against the batch, patience, the ranker and the fallback, and the refusals that stay pinned."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_beam_ref as BR  # noqa: E402
import _whisper_ref as R  # noqa: E402
import _whisper_sample_ref as SR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_beam as WB  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd import whisper_sampling as WS  # noqa: E402

K, SAMPLE_LEN = 3, 11
OPTS = WD.DecodingOptions(language=4, sample_len=SAMPLE_LEN, beam_size=K, prompt=[1000, 1001], suppress_tokens=[7, 8])
WEIGHT_SEED = 21
FEAT_SEED = {"plain": 14, "narrow": 12}  # chosen on the GPU so that the full replay's smallest decision margin clears 1e-3 (see the test)
KEEP_SEED, KEEP = 8, 8  # the narrow set's ids: chosen on the GPU so that eot is among the better of them and sequences do finish
_cache = {}


def options(kind):
    """plain: the sampling tests' options with a beam.  narrow: no timestamps and every id suppressed but 8 text ids and eot -- on random weights eot is
    otherwise never among a row's best four, and no sequence would finish: this set is what exercises the finished stores end to end."""
    if kind == "plain":
        return OPTS
    d = T.dims(**T.SHAPE_A)
    keep = {int(t) for t in np.random.default_rng(KEEP_SEED).choice(np.arange(1000, 50000), size=KEEP, replace=False)} | {whisper.special_tokens(d).eot}
    return WD.DecodingOptions(language=4, sample_len=SAMPLE_LEN, beam_size=K, prompt=[1000, 1001], without_timestamps=True,
                              suppress_tokens=[t for t in range(d.n_vocab) if t not in keep])


def _model():
    if "m" not in _cache:
        d = T.dims(**T.SHAPE_A)
        m = whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **T.decoder_weights(d, WEIGHT_SEED)})
        assert m.has_text_decoder
        _cache["m"] = (d, m)
    return _cache["m"]


def _filters(d, tok, opts):
    P = T.pick_params(tok, d.n_vocab, without_timestamps=opts.without_timestamps, max_initial_timestamp_index=round(1.0 / (30 / d.n_audio_ctx)))
    return P, WD.suppress_list(tok, opts)


def replay(m, d, feats, opts, steps):
    """the restatement driven by Model.logits of its own live prefixes -> the windows"""
    tok = whisper.special_tokens(d)
    P, sup = _filters(d, tok, opts)
    init = list(WD.initial_tokens(tok, opts, d.n_text_ctx, steps))
    k = opts.beam_size
    wins = [BR.BeamWindow(k, WB.max_candidates(k, opts.patience), tok.eot) for _ in range(feats.shape[0])]
    for _ in range(steps):
        seq = np.array([init + w.prefix[j] for w in wins for j in range(k)], np.int64)
        lg = m.logits(seq, np.repeat(feats, k, axis=0))[:, -1].cpu().numpy()
        for a, w in enumerate(wins):
            w.update([T.filter_logits(lg[a * k + j], w.prefix[j], P, suppress=sup) if w.live(j) else None for j in range(k)])
        if all(w.complete for w in wins):
            break
    return wins


def run_beam(kind, feat_seed=None):
    d, m = _model()
    tok = whisper.special_tokens(d)
    opts = options(kind)
    feats = T.features(d, 2, FEAT_SEED[kind] if feat_seed is None else feat_seed)
    win = m.beam_candidates(feats, opts, eos_check_interval=4)
    finished, live = m._text.beam_read()
    return dict(d=d, m=m, tok=tok, feats=feats, opts=opts, win=win, finished=finished, live=live, init=list(WD.initial_tokens(tok, opts, d.n_text_ctx, SAMPLE_LEN)))


@pytest.fixture(scope="module", params=["plain", "narrow"])
def beam_a(request):
    """what every test shares: 2 windows, beam_size 3, the device's candidates and its finished / live stores read right behind them"""
    return run_beam(request.param)


def test_every_candidates_sum_equals_the_replay_of_its_own_sequence(beam_a):
    """Model.logits of each candidate's whole sequence through the numpy filters: the returned sum_logprob within 1e-4 of the replayed one (a finished
    sequence's includes its eot).  Wrong ancestry, a wrong derived pick state or a wrong token store anywhere would show here."""
    s = beam_a
    d, m, tok, win, OPTS = s["d"], s["m"], s["tok"], s["win"], s["opts"]
    assert len(win.candidates) == 2 and not win.single and win.temperature == 0.0 and win.languages == [tok.language_tokens[4]] * 2
    P, sup = _filters(d, tok, OPTS)
    S0 = len(s["init"])
    for a in range(2):
        group = win.candidates[a]
        nf = len(s["finished"][a])
        assert len(group) >= K and group[:nf] == s["finished"][a] and group == WB.finalize(s["finished"][a], s["live"][a], K)
        ended = [True] * nf + [False] * (len(group) - nf)
        n = max(len(c[0]) for c in group) + 1
        seq = np.array([s["init"] + c[0] + [tok.eot] * (n - len(c[0])) for c in group], np.int64)
        lg = m.logits(seq, np.repeat(s["feats"][a:a + 1], len(group), axis=0)).cpu().numpy()
        for b, ((tokens, total), fin) in enumerate(zip(group, ended)):
            want, hist = 0.0, []
            for i, t in enumerate(tokens + ([tok.eot] if fin else [])):
                f = T.filter_logits(lg[b, S0 - 1 + i], hist, P, suppress=sup)
                assert np.isfinite(f[t]), (a, b, i, t)  # an admissible token
                want += f[t] - T.logsumexp(f)
                hist.append(t)
            print(f"window {a} candidate {b}: {len(tokens)} tokens, finished {fin}, sum {total:.5f}, replayed {want:.5f}")
            assert abs(total - want) < 1e-4, (a, b, total, want)
        assert len({tuple(c[0]) for c in group}) == len(group)  # the candidates of a window are different sequences
        x = lg[0, s["init"].index(tok.sot)].astype(np.float64)
        assert abs(win.no_speech_probs[a] - np.exp(x[tok.no_speech] - T.logsumexp(x))) < 1e-6
    if OPTS.without_timestamps:  # the narrow set is there for this
        assert any(s["finished"]), "no sequence finished: the finished stores were not exercised"


def test_the_full_replay_ends_with_the_devices_candidates(beam_a):
    """The restatement, driven step by step by Model.logits of its own live prefixes (prefill logits are the step's bits), ends with the device's candidate
    sequences in the device's order, sums within 1e-4; its smallest decision margin is at least 1e-3, so fp32 and float64 could not have ordered anything
    differently.  Observed on an MI355X with the seeds above: margin 0.0239 with no sequence finished (plain), 0.0222 with 3 + 2 finished (narrow); of the
    feature seeds 11 .. 18 scanned, every one gave the device's candidates, with margins from 0.0022 to 0.031."""
    s = beam_a
    wins = replay(s["m"], s["d"], s["feats"], s["opts"], SAMPLE_LEN)
    margin = min(min(w.margins) for w in wins)
    print(f"smallest decision margin of the replay: {margin:.5f}; steps {[w.steps for w in wins]}; finished {[len(w.finished) for w in wins]}")
    assert margin >= BR.MARGIN, margin
    for a, w in enumerate(wins):
        want, got = w.finalize(), s["win"].candidates[a]
        assert [c[0] for c in got] == [c[0] for c in want], (a, got, want)
        assert all(abs(g[1] - x[1]) < 1e-4 for g, x in zip(got, want))
        assert [f[0] for f in w.finished] == [f[0] for f in s["finished"][a]][: len(w.finished)]  # (the device may have stepped on to its next poll)


def test_beam_one_is_greedy_decoding():
    d, m = _model()
    feats = T.features(d, 2, 12)
    greedy = m.decode(feats, language=4, sample_len=9, prompt=[1000, 1001], suppress_tokens=[7, 8])
    beam = m.beam_search(feats, language=4, sample_len=9, prompt=[1000, 1001], suppress_tokens=[7, 8], beam_size=1)
    assert [r.tokens for r in beam] == [r.tokens for r in greedy] and all(len(r.tokens) > 0 for r in beam)
    assert all(abs(b.avg_logprob - g.avg_logprob) < 1e-6 and b.temperature == 0.0 for b, g in zip(beam, greedy))
    assert all(abs(b.no_speech_prob - g.no_speech_prob) < 1e-7 and b.language == g.language for b, g in zip(beam, greedy))
    det = m.beam_search(feats, sample_len=5, beam_size=2)  # and with language detection: decode's languages
    assert [r.language for r in det] == [r.language for r in m.decode(feats, sample_len=5)] and all(r.language_probs for r in det)


def test_a_window_alone_gives_its_candidates_of_the_batch(beam_a):
    s = beam_a
    one = s["m"].beam_candidates(s["feats"][1], s["opts"])  # 2-D input
    assert one.single and one.candidates == [s["win"].candidates[1]]  # tokens and the bits of the sums
    assert abs(one.no_speech_probs[0] - s["win"].no_speech_probs[1]) < 1e-7  # (torch's softmax over one row or two: not the decoder's bits)
    r = s["m"].beam_search(s["feats"][1], s["opts"])
    assert isinstance(r, WD.DecodingResult) and r.tokens == s["m"].beam_search(s["feats"], s["opts"])[1].tokens


def test_patience_two_returns_at_least_what_patience_one_finished():
    """the narrow options, 24 steps: with patience 2 a window keeps collecting after the K finished sequences that complete it with patience 1"""
    from dataclasses import replace

    d, m = _model()
    feats = T.features(d, 2, FEAT_SEED["narrow"])
    long_ = replace(options("narrow"), sample_len=24)
    m.beam_candidates(feats, long_, eos_check_interval=4)
    fin1, _ = m._text.beam_read()
    two = m.beam_candidates(feats, long_, patience=2.0, eos_check_interval=4)
    fin2, _ = m._text.beam_read()
    assert any(fin1) and sum(len(f) for f in fin2) > sum(len(f) for f in fin1)
    for a in range(2):
        assert len(fin1[a]) <= K and len(fin2[a]) <= 2 * K and fin2[a][: len(fin1[a])] == fin1[a], (a, fin1[a], fin2[a])  # the same walk, stopped later
        assert all(c in two.candidates[a] for c in fin1[a]) and len(two.candidates[a]) >= K
    print(f"finished with patience 1: {[len(f) for f in fin1]}, with patience 2: {[len(f) for f in fin2]}")


@pytest.mark.parametrize("length_penalty", [None, 0.6])
def test_beam_search_returns_the_ranked_candidate(beam_a, length_penalty):
    s = beam_a
    res = s["m"].beam_search(s["feats"], s["opts"], length_penalty=length_penalty)
    assert len(res) == 2
    for a, r in enumerate(res):
        group = s["win"].candidates[a]
        tokens, total = group[SR.rank(group, length_penalty)]
        assert WS.rank(group, length_penalty) == SR.rank(group, length_penalty)
        assert r.tokens == tokens and r.avg_logprob == total / (len(tokens) + 1) and r.temperature == 0.0 and r.text == ""
        assert r.language == s["tok"].language_tokens[4] and r.no_speech_prob == s["win"].no_speech_probs[a]


def test_the_fallback_runs_beam_search_once_and_sample_after_it():
    d, m = _model()
    feats = T.features(d, 2, FEAT_SEED["plain"])
    calls = []
    real = WB.beam_search, WS.sample

    def beam(*a, **kw):
        calls.append("beam")
        return real[0](*a, **kw)

    def sample(*a, **kw):
        calls.append("sample")
        return real[1](*a, **kw)

    WB.beam_search, WS.sample = beam, sample
    try:
        kept = m.beam_decode_with_fallback(feats, logprob_threshold=None, beam_size=K, language=4, sample_len=SAMPLE_LEN, prompt=[1000, 1001], suppress_tokens=[7, 8])
        assert calls == ["beam"] and [r.tokens for r in kept] == [r.tokens for r in real[0](m, feats, OPTS)] and all(r.temperature == 0.0 for r in kept)
        del calls[:]
        last = m.beam_decode_with_fallback(feats, temperature=(0.0, 0.5, 1.0), logprob_threshold=1.0, no_speech_threshold=None, seed=5, beam_size=K, best_of=2,
                                           language=4, sample_len=7)  # an average log-probability is never above 0: every temperature runs
        assert calls == ["beam", "sample", "sample"]
    finally:
        WB.beam_search, WS.sample = real
    want = m.sample(feats, language=4, sample_len=7, best_of=2, temperature=1.0, seed=5)
    assert [r.temperature for r in last] == [1.0, 1.0] and [r.tokens for r in last] == [r.tokens for r in want]


def test_the_pinned_refusals_still_hold_and_greedy_decoding_runs_after_a_beam():
    d, m = _model()
    feats = T.features(d, 1, 14)
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
        m.decode(feats, beam_size=2)
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
        m.sample(feats, temperature=0.5, beam_size=2)
    srv = m.serve(max_rows=2)
    try:
        with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
            srv.submit(feats[0], beam_size=2)
    finally:
        srv.close()
    with pytest.raises(ValueError, match="temperature 0"):
        m.beam_search(feats, beam_size=2, temperature=0.5)
    res = m.decode(feats, language=0, sample_len=3)
    m.beam_search(feats, language=0, sample_len=3, beam_size=2)
    again = m.decode(feats, language=0, sample_len=3)  # the handle is back on the greedy pick and on the direct attention
    assert again[0].tokens == res[0].tokens and again[0].avg_logprob == res[0].avg_logprob
