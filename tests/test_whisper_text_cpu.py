"""Whisper text side, host half (mlx-audio_amd/whisper_decoding.py) and the CPU references of its GPU tests (tests/_whisper_text_ref.py), pinned against
an independent implementation: transformers' WhisperDecoder, WhisperConfig and logits processors.  No GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

DA = T.dims(**T.SHAPE_A)


# ---- shapes and tokens ------------------------------------------------------------------------------------------------------------------------
def test_decoder_shapes_cover_exactly_the_hf_decoder_minus_the_key_biases():
    from transformers.models.whisper.modeling_whisper import WhisperDecoder

    d = T.dims(128, 2, 2, 1000, 50, 64)  # a small vocabulary: only names and shapes matter here
    dec = WhisperDecoder(T.hf_config(d))
    theirs = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    ours = whisper.decoder_shapes(d)
    w = {k: np.zeros(s, np.float32) for k, s in ours.items()}
    mapped = {k: tuple(v.shape) for k, v in T.hf_state_dict(d, w).items()}
    assert len(mapped) == len(ours)
    assert set(theirs) == set(mapped)  # (its k_proj Linears are built without a bias, like the reference's keys)
    assert not any(k.endswith("k_proj.bias") for k in theirs)
    assert all(theirs[k] == s for k, s in mapped.items())
    assert not any(k.endswith("key.bias") for k in ours)


def test_special_tokens_of_the_three_vocabularies():
    from transformers import WhisperConfig

    t = whisper.special_tokens(T.dims(128, 2, 1, 51865, 100))
    assert (t.eot, t.sot, t.translate, t.transcribe, t.sot_lm, t.sot_prev, t.no_speech, t.no_timestamps, t.timestamp_begin) == \
        (50257, 50258, 50358, 50359, 50360, 50361, 50362, 50363, 50364)
    assert t.language_tokens[0] == 50259 and len(t.language_tokens) == 99 and t.multilingual
    t3 = whisper.special_tokens(T.dims(128, 2, 1, 51866, 100))  # large-v3: one more language
    assert (t3.eot, t3.sot, len(t3.language_tokens), t3.translate, t3.transcribe, t3.sot_lm, t3.sot_prev, t3.no_speech, t3.no_timestamps, t3.timestamp_begin) == \
        (50257, 50258, 100, 50359, 50360, 50361, 50362, 50363, 50364, 50365)
    te = whisper.special_tokens(T.dims(128, 2, 1, 51864, 100))  # English-only (GPT-2 vocabulary)
    assert (te.eot, te.sot, te.translate, te.transcribe, te.sot_lm, te.sot_prev, te.no_speech, te.no_timestamps, te.timestamp_begin) == \
        (50256, 50257, 50357, 50358, 50359, 50360, 50361, 50362, 50363)
    assert not te.multilingual
    cfg = WhisperConfig()  # its defaults state the English-only numbering: eos, the start token, and the blank suppression (" " and eot)
    assert cfg.eos_token_id == te.eot and cfg.decoder_start_token_id == te.sot and set(cfg.begin_suppress_tokens) == {220, te.eot}
    assert cfg.vocab_size == 51865 and cfg.max_target_positions == 448
    for tok, n in ((t, 51865), (t3, 51866), (te, 51864)):
        assert n - tok.timestamp_begin == 1501  # <|0.00|> .. <|30.00|>


def test_initial_tokens_and_suppress_list():
    t = whisper.special_tokens(DA)
    o = WD.DecodingOptions(language=3)
    assert WD.initial_tokens(t, o, 448, 224) == (t.sot, t.language_tokens[3], t.transcribe)
    o = WD.DecodingOptions(language=t.language_tokens[7], task="translate", without_timestamps=True)
    assert WD.initial_tokens(t, o, 448, 224) == (t.sot, t.language_tokens[7], t.translate, t.no_timestamps)
    o = WD.DecodingOptions(language=0, prompt=list(range(1000, 1300)), prefix=list(range(2000, 2100)), sample_len=200)
    got = WD.initial_tokens(t, o, 448, 200)
    assert got[0] == t.sot_prev and got[1:224] == tuple(range(1077, 1300))  # the last n_ctx // 2 - 1 prompt tokens
    assert got[224:227] == (t.sot, t.language_tokens[0], t.transcribe) and got[227:] == tuple(range(2076, 2100))  # the last n_ctx // 2 - sample_len
    assert WD.suppress_list(t, WD.DecodingOptions()) == tuple(sorted({t.transcribe, t.translate, t.sot, t.sot_prev, t.sot_lm, t.no_speech}))
    assert set(WD.suppress_list(t, WD.DecodingOptions(suppress_tokens=[5, 7]))) >= {5, 7, t.sot}
    assert set(WD.suppress_list(t, WD.DecodingOptions(suppress_tokens="-1,11"))) >= {11, t.no_speech}
    bits = WD.suppress_bitmask(100, [0, 31, 32, 99])
    assert bits.tolist() == [0x80000001, 1, 0, 8]
    with pytest.raises(ValueError):
        WD.language_token(t, 50000)
    te = whisper.special_tokens(T.dims(128, 2, 1, 51864, 100))
    assert WD.initial_tokens(te, WD.DecodingOptions(), 448, 224) == (te.sot,)


# ---- the filters --------------------------------------------------------------------------------------------------------------------------------
def _histories(tok):
    """sampled-token histories that reach every branch of the timestamp rules"""
    tb, txt = tok.timestamp_begin, 1000
    return [[], [tb + 5], [txt], [tb + 5, txt], [tb + 5, txt, tb + 9], [tb + 5, txt, tb + 9, tb + 9], [tb, txt, txt + 1], [tb], [tb + 3, tb + 3],
            [tb + 2, txt, tb + 4, tb + 4, txt], [txt, txt + 1], [tb + 1499, txt]]


@pytest.mark.parametrize("n_vocab", [51865, 51866])
def test_timestamp_rules_equal_transformers(n_vocab):
    """The numpy restatement against WhisperTimeStampLogitsProcessor on random logits, every history of _histories, with and without
    max_initial_timestamp_index, and with the timestamps' share of the probability on both sides of the best text token.  No case is left out: the
    restatement follows OpenAI's original where the reference's text departs from it (filter_logits' docstring), and transformers follows the original
    too.  The reference's own reading of the probability-mass rule (mass_on="handed") is run beside it: it may differ in that rule's decision only."""
    import torch
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor

    tok = whisper.special_tokens(T.dims(128, 2, 1, n_vocab, 100))
    g = np.random.default_rng(n_vocab)
    begin = 3
    checked = differ = 0
    for mi in (None, 50):
        gc = SimpleNamespace(eos_token_id=tok.eot, bos_token_id=tok.eot, no_timestamps_token_id=tok.no_timestamps, max_initial_timestamp_index=mi)
        proc = WhisperTimeStampLogitsProcessor(gc, begin_index=begin)
        P = T.pick_params(tok, n_vocab, suppress_blank=False, max_initial_timestamp_index=mi)
        for hist in _histories(tok):
            for boost in (0.0, 12.0):  # 1501 timestamps at +12 outweigh any single text token; at +0 the best text token wins
                logits = g.standard_normal(n_vocab).astype(np.float32) * 2.0
                logits[tok.timestamp_begin:] += np.float32(boost) - 6.0
                ids = torch.tensor([[tok.sot, tok.language_tokens[0], tok.transcribe] + hist])
                want = proc(ids, torch.from_numpy(logits)[None].clone())[0].numpy()
                got = T.filter_logits(logits, hist, P, mass_on="masked")
                assert np.array_equal(np.isneginf(got), np.isneginf(want)), (mi, hist, boost)
                assert np.array_equal(got[~np.isneginf(got)], logits[~np.isneginf(want)].astype(np.float64))
                ref = T.filter_logits(logits, hist, P, mass_on="handed")
                assert np.isfinite(got).any()
                if not np.array_equal(np.isneginf(ref), np.isneginf(got)):  # only ever: text masked by one and not by the other
                    differ += 1
                    d = np.isneginf(ref) != np.isneginf(got)
                    assert not d[tok.timestamp_begin:].any()
                checked += 1
    print(f"n_vocab {n_vocab}: {checked} cases equal transformers, {differ} where the probability-mass rule on the handed logits decides otherwise")
    assert checked == 48


def test_suppress_rules_equal_transformers():
    import torch
    from transformers.generation.logits_process import SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor

    tok = whisper.special_tokens(DA)
    V = DA.n_vocab
    g = np.random.default_rng(3)
    sup = WD.suppress_list(tok, WD.DecodingOptions(suppress_tokens=[1, 2, 7, 50000]))
    P = T.pick_params(tok, V, without_timestamps=True)
    procs = [SuppressTokensAtBeginLogitsProcessor([220, tok.eot], begin_index=4), SuppressTokensLogitsProcessor(sup)]
    for hist in ([], [1000], [1000, tok.eot]):
        logits = g.standard_normal(V).astype(np.float32)
        ids = torch.tensor([[tok.sot, tok.language_tokens[0], tok.transcribe, tok.no_timestamps] + hist])
        want = torch.from_numpy(logits)[None].clone()
        for p in procs:
            want = p(ids, want)
        got = T.filter_logits(logits, hist, P, suppress=sup)
        assert np.array_equal(got, want[0].numpy().astype(np.float64))
        assert np.isneginf(got[220]) == (len(hist) == 0) and np.isneginf(got[tok.sot])
    got = T.filter_logits(logits, [], dict(P, suppress_blank=0))
    assert np.array_equal(got, logits.astype(np.float64))


def test_greedy_row_freezes_after_eot():
    r = T.GreedyRow(eot=5)
    x = np.array([0.0, 1.0, 3.0, 0.5, 0.2, 2.0, -np.inf])
    assert r.update(x) == 2 and r.sum_logprob == pytest.approx(3.0 - T.logsumexp(x))
    y = x.copy()
    y[2] = -np.inf
    assert r.update(y) == 5 and r.ended
    s = r.sum_logprob
    assert r.update(x) == 5 and r.sum_logprob == s and r.sampled == [2, 5, 5]
    assert int(np.argmax(np.array([1.0, 7.0, 7.0]))) == 1  # ties: the lowest index


# ---- options ------------------------------------------------------------------------------------------------------------------------------------
def test_option_validation():
    v = WD.verify_options
    O = WD.DecodingOptions
    with pytest.raises(ValueError, match="beam_size and best_of can't be given together"):
        v(O(beam_size=2, best_of=2))
    with pytest.raises(ValueError, match=r"best_of with greedy sampling \(T=0\) is not compatible"):
        v(O(best_of=2))
    with pytest.raises(ValueError, match="patience requires beam_size to be given"):
        v(O(patience=1.0))
    with pytest.raises(ValueError, match=r"length_penalty \(alpha\) should be a value between 0 and 1"):
        v(O(length_penalty=1.5))
    msgs = []
    for o in (O(temperature=0.5), O(temperature=0.5, best_of=3), O(beam_size=4), O(beam_size=4, patience=2.0)):
        with pytest.raises(NotImplementedError) as ei:
            v(o)
        assert "text decoder: not built" not in str(ei.value)
        msgs.append(str(ei.value))
    assert len(set(msgs)) == 4 and "temperature" in msgs[0] and "best_of" in msgs[1] and "Beam search" in msgs[2] and "patience" in msgs[3]
    with pytest.raises(ValueError, match="tokenizer is not built"):
        v(O(language="en"))
    with pytest.raises(ValueError, match="tokenizer is not built"):
        v(O(language=0, prompt="hello"))
    assert v(O(language=0)) == O(language=0)
    names = [f.name for f in O.__dataclass_fields__.values()]
    assert names == ["task", "language", "temperature", "sample_len", "best_of", "beam_size", "patience", "length_penalty", "prompt", "prefix",
                     "suppress_tokens", "suppress_blank", "without_timestamps", "max_initial_timestamp", "fp16"]
    r = WD.DecodingResult(audio_features=None, language=50259)
    assert r.text == "" and np.isnan(r.compression_ratio) and r.tokens == [] and np.isnan(r.avg_logprob)
    assert whisper.DecodingOptions is O and whisper.DecodingResult is WD.DecodingResult


# ---- weights --------------------------------------------------------------------------------------------------------------------------------------
SMALL = T.dims(128, 2, 2, 300, 50, 32)


@pytest.mark.parametrize("name", ["decoder.token_embedding.weight", "decoder.blocks.1.cross_attn.key.weight", "decoder.blocks.0.mlp_ln.bias",
                                  "decoder.positional_embedding"])
def test_a_complete_set_with_a_misshapen_or_missing_tensor_names_it(name):
    w = {k: np.zeros(s, np.float32) for k, s in whisper.decoder_shapes(SMALL).items()}
    assert set(whisper.decoder_tensors(SMALL, dict(w, alignment_heads=b"x"))) == set(w)
    good = w[name]
    w[name] = np.zeros(tuple(s + 1 for s in good.shape), np.float32)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        whisper.decoder_tensors(SMALL, w)
    del w[name]
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        WD.check_decoder_tensors(SMALL, w)


def test_a_partial_set_leaves_the_text_side_unbuilt():
    w = {k: np.zeros(s, np.float32) for k, s in whisper.decoder_shapes(SMALL).items()}
    del w["decoder.blocks.1.mlp2.bias"]
    assert whisper.decoder_tensors(SMALL, w) is None
    assert whisper.decoder_tensors(SMALL, {"decoder.token_embedding.weight": np.ones((4, 4), np.float16)}) is None  # misshapen, but not a complete set
    assert whisper.decoder_tensors(SMALL, {}) is None
    m = whisper.Model(SMALL)
    assert m.has_text_decoder is False
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        m.decode(np.zeros((100, 80), np.float32), temperature=0.7)  # the first check, before any option is looked at


def test_the_library_refuses_bad_text_configs_without_a_gpu():
    import ctypes as C

    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 15
    ok = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=1, n_audio_ctx=1500, n_audio_state=384)
    for bad, word in ((dict(n_text_head=4), b"head dimension"), (dict(n_text_state=192, n_text_head=3, n_audio_state=192), b"multiple of 128"),
                      (dict(n_text_state=2176, n_text_head=34, n_audio_state=2176), b"at most 2048"), (dict(n_audio_state=512), b"n_audio_state")):
        h = C.c_void_p()
        assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**dict(ok, **bad))), C.byref(h)) != 0
        assert word in lib.kk_last_error(), lib.kk_last_error()
    h = C.c_void_p()
    assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**ok)), C.byref(h)) == 0
    assert lib.kk_whisper_text_state_bytes(h, 2) > 2 * 1500 * 2 * 384 * 2 and lib.kk_whisper_text_position(h) == -1
    lib.kk_whisper_text_destroy(h)
    # M = 17 rows is an error return of the skinny Linear, before anything is launched
    assert lib.kk_op_whisper_linear_rows(None, 17, 16, 32, 16, 32, 16, None, 0, None, 0, 16, 16, None, 0, None, 0) != 0
    assert b"M <= 16" in lib.kk_last_error()


def test_the_hf_yardstick_runs_and_its_bf16_run_is_close():
    """the reference of the GPU tests at shape a: fp32 against its own bf16 CPU run (the 1.5x criterion's denominator is not degenerate)"""
    w = T.decoder_weights(DA, 1)
    dec = T.hf_decoder(DA, w)
    g = np.random.default_rng(0)
    toks = g.integers(0, DA.n_vocab, (2, 5))
    feats = T.features(DA, 2, 2)
    a, b = T.hf_logits(dec, toks, feats), T.hf_logits(dec, toks, feats, bf16=True)
    from _whisper_ref import rel_rms

    e = rel_rms(b, a)
    print(f"shape a: logits rms {np.sqrt((a ** 2).mean()):.3f}, bf16 CPU run rel rms {e:.4f}")
    assert a.shape == (2, 5, DA.n_vocab) and 1e-4 < e < 0.05
