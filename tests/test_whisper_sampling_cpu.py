"""Whisper sampling, host half (mlx-audio_amd/whisper_sampling.py) and the restatement its GPU tests compare against
(tests/_whisper_sample_ref.py): the uniform mapping, the ranker, option validation, the fallback loop on scripted callables, and the cap on draws with
more than one admissible token evaluated on the GPU kernel tests' own inputs.  No GPU."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sampler_ref as S  # noqa: E402
import _whisper_sample_ref as SR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd import whisper_sampling as WS  # noqa: E402

O = whisper.DecodingOptions


def test_philox_open_is_exact_and_strictly_inside_the_unit_interval():
    r = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], np.uint64)
    u = SR.philox_open(r)
    assert u.dtype == np.float32
    want = [((int(x) >> 9) + 0.5) / 2.0 ** 23 for x in r]  # exact rationals: a 23-bit integer plus a half has 24 significant bits
    assert [float(x) for x in u] == want
    assert float(u[0]) == 2.0 ** -24 and float(u[-1]) == 1.0 - 2.0 ** -24 and (u > 0).all() and (u < 1).all()
    assert float(SR.philox_unit_f32(0xFFFFFFFF)) == 1.0 and float(SR.philox_unit_f32(0)) > 0.0  # what philox_open is there to avoid
    g = -np.log(-np.log(u.astype(np.float64)))
    assert np.isfinite(g).all() and -2.82 < g.min() and g.max() < 16.64


def test_the_vectorised_philox_equals_the_scalar_one():
    subs = np.array([0, 1, 2, 12966, 0xFFFFFFFF], np.uint64)
    for seed, ctr in ((0, 0), (7, (5 << 32) | 3), (0xDEADBEEFCAFEF00D, (0xFFFFFFFF << 32) | 0xFFFFFFFF)):
        got = SR.philox4_vec(seed, ctr, subs)
        for j, sub in enumerate(subs):
            assert [int(x) for x in got[:, j]] == S.philox4(seed, ctr, int(sub))
    ids = np.array([0, 1, 2, 3, 4, 51865])  # token i: word i & 3 of the counter's sub-word i >> 2
    u = SR.uniforms(9, 2, 5, ids)
    for i, x in zip(ids, u):
        assert float(x) == ((S.philox4(9, (2 << 32) | 5, int(i) >> 2)[int(i) & 3] >> 9) + 0.5) / 2.0 ** 23


def test_rank():
    long_, short = ([1] * 10, -10.0), ([1, 2], -3.0)
    for rank in (WS.rank, SR.rank):
        assert rank([long_, short], None) == 0  # -1.0 against -1.5 per token
        assert rank([long_, short], 0) == 1  # no penalty: the plain sums, -10 against -3
        assert rank([long_, short], 0.6) == 1  # -10 / 2.5^0.6 = -5.77 against -3 / (7 / 6)^0.6 = -2.73
        assert rank([([1] * 30, -9.0), ([1, 2], -3.0)], 0.6) == 1 and rank([([1] * 30, -9.0), ([1, 2], -3.0)], 1.0) == 0  # -2.63 / -2.73, then -1.54 / -2.57
        assert rank([([1, 2], -3.0), ([3, 4], -3.0), ([5], -1.5)], None) == 0  # ties: the lowest index
        assert rank([([1], -2.0), ([3, 4], -3.0), ([5, 6], -3.0)], 0.0) == 0
        assert rank([([], -0.5), ([1, 2], -30.0)], None) == 1  # a zero-length candidate scores -inf where the reference divides by zero
        assert rank([([], -0.5), ([], -0.1)], None) == 0
        assert rank([([], -0.5), ([1, 2], -30.0)], 0.6) == 0  # with a penalty its length is (5 + 0) / 6: an ordinary score
        assert rank([([7], -1.0)], None) == 0


def test_verify_sampling_options_every_message():
    v = WS.verify_sampling_options
    for o, word in ((O(temperature=0.5, beam_size=2, best_of=2), "beam_size and best_of can't be given together"),
                    (O(temperature=0, best_of=2), r"best_of with greedy sampling \(T=0\) is not compatible"),
                    (O(temperature=0.5, patience=1.0), "patience requires beam_size to be given"),
                    (O(temperature=0.5, length_penalty=1.5), r"length_penalty \(alpha\) should be a value between 0 and 1"),
                    (O(temperature=0.0), "temperature 0 is greedy decoding: call decode"), (O(temperature=-0.5), "finite temperature > 0"),
                    (O(temperature=float("nan")), "finite temperature > 0"), (O(temperature=float("inf")), "finite temperature > 0"),
                    (O(temperature=0.5, best_of=9), "best_of must be in 1 .. 8"), (O(temperature=0.5, best_of=0), "best_of must be in 1 .. 8"),
                    (O(temperature=0.5, language="en"), "tokenizer is not built"), (O(temperature=0.5, language=0, prompt="hi"), "prompt must be a list of token ids"),
                    (O(temperature=0.5, language=0, prefix="hi"), "prefix must be a list of token ids"), (O(temperature=0.5, task="lang_id"), "call decode"),
                    (O(temperature=0.5, task="sing"), "unknown task")):
        with pytest.raises(ValueError, match=word):
            v(o)
    for o, word in ((O(temperature=0.5, beam_size=2), "Beam search decoder is not yet implemented"),
                    (O(temperature=0.5, beam_size=2, patience=1.0), "patience belongs to beam search, which is not yet implemented")):
        with pytest.raises(NotImplementedError, match=word) as ei:
            v(o)
        with pytest.raises(NotImplementedError) as theirs:  # the messages verify_options already uses
            WD.verify_options(O(beam_size=o.beam_size, patience=o.patience))
        assert str(ei.value) == str(theirs.value)
    ok = O(temperature=0.5, best_of=8, language=3, length_penalty=0.6)
    assert v(ok) is ok and v(O(temperature=1)) == O(temperature=1)
    assert WS.MAX_GROUP == 8
    with pytest.raises(NotImplementedError, match="sampling at temperature > 0 is not yet implemented"):  # the pinned refusals are not this module's to lift
        WD.verify_options(O(temperature=0.5))
    m = whisper.Model(T.dims(128, 2, 2, 300, 50, 32))  # encoder-only
    for call in (m.sample, m.sample_candidates, m.decode_with_fallback):
        with pytest.raises(NotImplementedError, match="text decoder: not built"):
            call(np.zeros((100, 80), np.float32))


def _scripted(table):
    """greedy / sampled callables that answer from table[(window, temperature)] = (avg_logprob, no_speech_prob) and log their calls"""
    calls = []

    def res(i, t):
        lp, ns = table[(i, t)]
        return SimpleNamespace(avg_logprob=lp, no_speech_prob=ns, temperature=t, window=i)

    def greedy(idx):
        calls.append((0.0, list(idx)))
        return [res(i, 0.0) for i in idx]

    def sampled(idx, t):
        calls.append((t, list(idx)))
        return [res(i, t) for i in idx]

    return greedy, sampled, calls


def test_the_fallback_loop_on_scripted_results():
    temps = (0.0, 0.2, 0.4)
    table = {(0, 0.0): (-0.5, 0.1),                                              # passes at once
             (1, 0.0): (-2.0, 0.1), (1, 0.2): (-0.9, 0.1),                       # passes at the second temperature
             (2, 0.0): (-3.0, 0.9),                                              # silence: its low log-probability does not count
             (3, 0.0): (-2.0, 0.2), (3, 0.2): (-1.5, 0.2), (3, 0.4): (-1.2, 0.2)}  # never passes: the last temperature's result
    greedy, sampled, calls = _scripted(table)
    out = WS.fallback_loop(4, temps, greedy, sampled, -1.0, 0.6)
    assert [(r.window, r.temperature) for r in out] == [(0, 0.0), (1, 0.2), (2, 0.0), (3, 0.4)]
    assert calls == [(0.0, [0, 1, 2, 3]), (0.2, [1, 3]), (0.4, [3])]  # only the failing windows, together, under their original indices
    greedy, sampled, calls = _scripted(table)
    out = WS.fallback_loop(4, temps, greedy, sampled, None, 0.6)  # no threshold: nothing needs fallback
    assert [r.temperature for r in out] == [0.0] * 4 and calls == [(0.0, [0, 1, 2, 3])]
    greedy, sampled, calls = _scripted({**table, (2, 0.2): (-0.1, 0.9)})
    out = WS.fallback_loop(4, temps, greedy, sampled, -1.0, None)  # no silence rule: window 2 falls back too
    assert calls[1] == (0.2, [1, 2, 3]) and out[2].temperature == 0.2
    greedy, sampled, calls = _scripted({(0, 0.7): (-5.0, 0.0)})
    out = WS.fallback_loop(1, [0.7], greedy, sampled, -1.0, 0.6)  # a first temperature above 0 goes to the sampler
    assert calls == [(0.7, [0])] and out[0].temperature == 0.7


def test_decode_with_fallback_routes_options_and_accepts_a_scalar_temperature():
    """on a fake model: temperature 0 goes to model.decode with best_of dropped, above 0 to sample with beam_size / patience dropped and the original
    indices as streams; a scalar temperature is one pass"""
    import torch

    d = T.dims(128, 2, 2, 300, 50, 32)
    seen = []

    class Fake:
        dims, device = d, torch.device("cpu")

        def decode(self, feats, options):
            seen.append(("decode", tuple(feats.shape), options))
            return [SimpleNamespace(avg_logprob=-9.0, no_speech_prob=0.0, temperature=0.0) for _ in range(feats.shape[0])]

    def fake_sample(model, feats, options, seed, streams):
        seen.append(("sample", tuple(feats.shape), options, seed, list(streams)))
        return [SimpleNamespace(avg_logprob=-9.0 if s == 2 else -0.1, no_speech_prob=0.0, temperature=options.temperature) for s in streams]

    feats = np.zeros((3, d.n_audio_ctx, d.n_audio_state), np.float32)
    real = WS.sample
    WS.sample = fake_sample
    try:
        out = WS.decode_with_fallback(Fake(), feats, temperature=(0.0, 0.5, 1.0), seed=4, best_of=3, language=2)
        assert [r.temperature for r in out] == [0.5, 0.5, 1.0]
        assert seen[0][:2] == ("decode", (3, 50, 128)) and seen[0][2] == O(language=2)  # best_of dropped, temperature 0
        assert seen[1] == ("sample", (3, 50, 128), O(language=2, best_of=3, temperature=0.5), 4, [0, 1, 2])
        assert seen[2] == ("sample", (1, 50, 128), O(language=2, best_of=3, temperature=1.0), 4, [2])
        del seen[:]
        one = WS.decode_with_fallback(Fake(), feats[0], temperature=0.0, beam_size=5, patience=2.0, language=2)  # scalar temperature, 2-D input: one result
        assert one.temperature == 0.0 and len(seen) == 1 and seen[0][2] == O(language=2, beam_size=5, patience=2.0)  # (decode itself refuses beam search)
        del seen[:]
        WS.decode_with_fallback(Fake(), feats[:1], temperature=0.3, beam_size=5, patience=2.0, language=2)
        assert seen == [("sample", (1, 50, 128), O(language=2, temperature=0.3), 0, [0])]  # beam_size / patience dropped above 0
        with pytest.raises(ValueError, match="at least one temperature"):
            WS.decode_with_fallback(Fake(), feats, temperature=())
    finally:
        WS.sample = real
    assert "compression_ratio" in WS.decode_with_fallback.__doc__ and "nan" in WS.decode_with_fallback.__doc__


def test_sampled_row_follows_given_tokens_and_freezes_after_eot():
    x = np.full(50, -np.inf)
    x[[3, 7, 9]] = [0.0, 1.0, 2.0]
    row = SR.SampledRow(eot=7, temperature=1.0, seed=1, stream=0)
    adm = row.update(x, 9)
    lse = T.logsumexp(x)
    assert adm is not None and set(adm) <= {3, 7, 9} and abs(row.sum_logprob - (2.0 - lse)) < 1e-12 and not row.ended
    row.update(x, 7)
    assert row.ended and abs(row.sum_logprob - (3.0 - 2 * lse)) < 1e-12
    assert row.update(x, 3) is None and row.sampled == [9, 7, 7] and row.draws == 2  # an ended row emits eot, its sum stays
    assert abs(row.sum_logprob - (3.0 - 2 * lse)) < 1e-12
    empty = SR.SampledRow(eot=7, temperature=1.0, seed=1, stream=0)
    assert empty.update(np.full(50, -np.inf)) == [7] and empty.ended and empty.sum_logprob == 0.0  # every token masked: eot, logprob 0
    # the draws of a row do not depend on anything but (seed, stream, count): two rows with the same key agree, another stream differs somewhere
    a, b, c = (SR.SampledRow(7, 1.0, 5, s) for s in (2, 2, 3))
    y = np.random.default_rng(0).standard_normal(2000)
    ta, tb, tc = ([r.update(y) and r.sampled[-1] for _ in range(6)] for r in (a, b, c))
    assert ta == tb and ta != tc


def test_the_cap_on_ambiguous_draws_holds_on_the_gpu_tests_own_inputs():
    """The restatement alone, following its own choices, over the inputs of tests/test_gpu_whisper_sample_kernels.py: at most 2 % of the draws of each test
    have more than one admissible token (a numpy simulation at V = 51 866, T in {0.2, 1.0}, 400 draws each gave 0 - 0.25 %)."""
    for n_vocab, mi in SR.PICK_CASES:
        tok = whisper.special_tokens(T.dims(128, 2, 1, n_vocab, 100))
        P = T.pick_params(tok, n_vocab, max_initial_timestamp_index=mi)
        steps, sup = SR.pick_script(tok, n_vocab, mi)
        for temp in SR.PICK_TEMPERATURES:
            rows = [SR.SampledRow(tok.eot, temp, SR.PICK_SEED, s) for s in SR.PICK_STREAMS]
            for x in steps:
                for b, row in enumerate(rows):
                    row.update(T.filter_logits(x[b], row.sampled, P, suppress=sup))
            draws, multi = sum(r.draws for r in rows), sum(r.multi for r in rows)
            print(f"pick script V {n_vocab} T {temp}: {multi} of {draws} draws ambiguous")
            assert draws >= 8 and multi <= SR.CAP * draws
    x = SR.dist_logits().astype(np.float64)
    f = np.full(SR.DIST_V, -np.inf)
    f[list(SR.DIST_IDS)] = x[list(SR.DIST_IDS)]
    for temp in SR.PICK_TEMPERATURES:
        multi = sum(len(SR.draw(f, temp, SR.DIST_SEED, b, s)[0]) > 1 for b in range(SR.DIST_ROWS) for s in range(SR.DIST_STEPS))
        print(f"distribution T {temp}: {multi} of {SR.DIST_ROWS * SR.DIST_STEPS} draws ambiguous")
        assert multi <= SR.CAP * SR.DIST_ROWS * SR.DIST_STEPS


def test_the_library_declares_the_sampling_entries_and_refuses_without_a_gpu():
    import ctypes as C

    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 21 and _lib.WHISPER_MAX_GROUP == WS.MAX_GROUP
    cfg = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=1, n_audio_ctx=1500, n_audio_state=384)
    h = C.c_void_p()
    assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**cfg)), C.byref(h)) == 0
    plain, grouped = lib.kk_whisper_text_state_bytes(h, 6), lib.kk_whisper_text_state_bytes_groups(h, 2, 3)
    assert lib.kk_whisper_text_state_bytes_groups(h, 6, 1) == plain
    assert plain - grouped == 4 * 1500 * 2 * 384 * 2  # four cross K/V slices fewer: 6 rows on 2 windows
    assert lib.kk_whisper_text_state_bytes_groups(h, 2, 0) == 0 and lib.kk_whisper_text_state_bytes_groups(h, 2, 9) == 0
    assert lib.kk_whisper_text_sample_setup(h, None, 0.5, 0, (C.c_uint32 * 1)(0)) != 0 and b"set_audio first" in lib.kk_last_error()
    lib.kk_whisper_text_destroy(h)
    # the raw entry refuses a temperature that is not finite or not > 0 before anything is launched (the pointers are never looked at)
    one = C.c_void_p(16)
    for t in (0.0, -1.0, math.nan, math.inf):
        assert lib.kk_op_whisper_pick_sampled(None, 1, one, 8, one, None, t, 0, one, one, one, 1, one, one) != 0
        assert b"temperature" in lib.kk_last_error()
