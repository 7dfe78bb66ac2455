"""Whisper beam search, host half (mlx-audio_amd/whisper_beam.py) and the restatement its GPU tests compare against
(tests/_whisper_beam_ref.py): the update on hand-written tables, finalize, option validation, the fallback routing on a fake model, the library's new
entries, and the margin condition on the GPU kernel tests' own inputs.  No GPU."""
import ctypes as C
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_beam_ref as BR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_beam as WB  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd import whisper_sampling as WS  # noqa: E402

O = whisper.DecodingOptions
EOT = 9


def _row(pairs, V=12):
    """filtered logits of a row whose log-probabilities are the given {token: logprob} (they sum to one with a filler token 0) and -inf elsewhere"""
    x = np.full(V, -np.inf)
    rest = 1.0 - sum(math.exp(v) for v in pairs.values())
    assert rest > 0
    x[0] = math.log(rest)
    for t, v in pairs.items():
        x[t] = v
    return x


def test_an_eot_behind_the_kth_saved_prefix_is_dropped_and_the_first_step_is_one_row():
    w = BR.BeamWindow(2, 2, EOT)
    a = _row({1: math.log(0.5), 2: math.log(0.3), EOT: math.log(0.1)})
    other = _row({5: math.log(0.9)})  # rows 1.. of the first step are copies of row 0 in a real run; a different row shows that they are not read
    w.update([a, other])
    assert w.prefix == [[1], [2]] and w.parents == [[0, 0]] and w.finished == [] and not w.complete  # eot ranked third: behind the second saved prefix
    assert abs(w.sums[0] - math.log(0.5)) < 1e-12 and abs(w.sums[1] - math.log(0.3)) < 1e-12
    # second step: (0, eot) -0.69 - 0.22; (0, 3) ...: eot first in the walk finishes, the walk goes on until two are saved
    r0 = _row({EOT: math.log(0.8), 3: math.log(0.15), 4: math.log(0.04)})
    r1 = _row({6: math.log(0.9), EOT: math.log(0.05), 7: math.log(0.04)})
    w.update([r0, r1])
    assert w.finished == [([1], pytest.approx(math.log(0.5) + math.log(0.8)))]
    assert w.prefix == [[2, 6], [1, 3]] and w.parents[-1] == [1, 0]  # 0.3 * 0.9 above 0.5 * 0.15; (1, eot) = 0.015 lies behind them: dropped
    assert len(w.finished) == 1 and not w.complete


def test_finished_stops_at_max_candidates_and_a_complete_window_keeps_stepping():
    w = BR.BeamWindow(3, 2, EOT)
    w.update([_row({1: math.log(0.4), 2: math.log(0.3), 3: math.log(0.2), 4: math.log(0.05)})] * 3)
    assert w.prefix == [[1], [2], [3]]
    rows = [_row({EOT: math.log(0.6), 5: math.log(0.2), 6: math.log(0.1), 7: math.log(0.05)}) for _ in range(3)]
    w.update(rows)  # three eot candidates, 0.24, 0.18 and 0.12, all ahead of the third saved prefix: only two fit
    assert [f[0] for f in w.finished] == [[1], [2]] and w.complete
    before = list(w.finished)
    w.update(rows)
    assert w.finished == before and w.complete and w.steps == 3 and all(len(p) == 3 for p in w.prefix)


def test_patience_two_keeps_a_window_running():
    rows1 = [_row({1: math.log(0.5), 2: math.log(0.4), 3: math.log(0.05)})] * 2
    rows2 = [_row({EOT: math.log(0.7), 5: math.log(0.2), 6: math.log(0.05)})] * 2
    one, two = BR.BeamWindow(2, WB.max_candidates(2, None), EOT), BR.BeamWindow(2, WB.max_candidates(2, 2.0), EOT)
    assert (one.max_candidates, two.max_candidates) == (2, 4)
    for w in (one, two):
        w.update(rows1)
        w.update(rows2)
    assert one.complete and not two.complete and one.finished == two.finished and len(two.finished) == 2
    two.update(rows2)
    assert two.complete and len(two.finished) == 4 and [f[0] for f in two.finished[:2]] == [f[0] for f in one.finished]


def test_finalize_tops_up_from_the_live_prefixes_and_skips_dead_slots():
    w = BR.BeamWindow(3, 3, EOT)
    w.update([_row({1: math.log(0.4), 2: math.log(0.3), 3: math.log(0.2), 4: math.log(0.05)})] * 3)
    w.update([_row({EOT: math.log(0.5), 5: math.log(0.3), 6: math.log(0.1), 7: math.log(0.05)})] + [_row({8: math.log(0.9), 5: math.log(0.04), 6: math.log(0.03), 7: math.log(0.01)})] * 2)
    assert [f[0] for f in w.finished] == [[1]] and w.prefix == [[2, 8], [3, 8], [1, 5]]
    got = w.finalize()
    assert [c[0] for c in got] == [[1], [2, 8], [3, 8]] and got[1][1] == w.sums[0]  # one finished, two live prefixes in descending sum, their sums unchanged
    assert WB.finalize(w.finished, list(zip(w.prefix, w.sums)), 3) == got  # the module's finalize is the restatement's
    # a row with a single unmasked token offers only it; a row with none offers (eot, 0): slots without a prefix die and are no candidates
    d = BR.BeamWindow(2, 2, EOT)
    only = np.full(12, -np.inf)
    only[4] = 1.5
    d.update([only, only])
    assert d.prefix == [[4], [EOT]] and d.sums[0] == 0.0 and d.sums[1] == -np.inf and d.parents == [[0, -1]]
    d.update([np.full(12, -np.inf), only])  # row 0 has nothing left: (eot, 0.0); row 1 is dead and is not read
    assert d.finished == [([4], 0.0)] and d.sums == [-np.inf, -np.inf] and not d.complete
    assert d.finalize() == [([4], 0.0)] and WB.finalize(d.finished, list(zip(d.prefix, d.sums)), 2) == [([4], 0.0)]


def test_exact_ties_follow_the_stated_order():
    offers, gap = BR.top_offers(np.array([1.0, 3.0, 3.0, -np.inf, 3.0, 2.0]), 3, EOT)
    assert [t for t, _ in offers] == [1, 2, 4] and gap == 1.0  # equal logits by the lower id; the gap to the next best
    w = BR.BeamWindow(2, 2, EOT)
    w.update_offers([[(1, -1.0), (2, -1.0), (3, -2.0)], []])
    assert w.prefix == [[1], [2]] and w.margins == [0.0]  # equal scores within a row: by rank
    w.update_offers([[(5, -1.0), (6, -3.0), (7, -4.0)], [(8, -1.0), (6, -3.0), (7, -4.0)]])
    assert w.prefix == [[1, 5], [2, 8]] and w.parents[-1] == [0, 1]  # equal scores across rows: the lower parent row first
    w.update_offers([[(EOT, -1.0), (6, -1.5), (7, -4.0)], [(EOT, -1.0), (6, -1.5), (7, -4.0)]])
    assert [f[0] for f in w.finished] == [[1, 5], [2, 8]] and w.prefix == [[1, 5, 6], [2, 8, 6]]


def test_verify_beam_options_every_message():
    v = WB.verify_beam_options
    for o, word in ((O(beam_size=2, best_of=2), "beam_size and best_of can't be given together"),
                    (O(temperature=0, best_of=2), r"best_of with greedy sampling \(T=0\) is not compatible"),
                    (O(patience=1.0), "patience requires beam_size to be given"),
                    (O(beam_size=2, length_penalty=1.5), r"length_penalty \(alpha\) should be a value between 0 and 1"),
                    (O(), "beam search needs beam_size"), (O(beam_size=0), "beam_size must be an integer in 1 .. 8"), (O(beam_size=9), "beam_size must be an integer in 1 .. 8"),
                    (O(beam_size=2.0), "beam_size must be an integer in 1 .. 8"),
                    (O(beam_size=2, patience=0.0), "patience must be finite and > 0"), (O(beam_size=2, patience=-1.0), "patience must be finite and > 0"),
                    (O(beam_size=2, patience=float("nan")), "patience must be finite and > 0"), (O(beam_size=2, patience=float("inf")), "patience must be finite and > 0"),
                    (O(beam_size=8, patience=2.1), r"round\(beam_size \* patience\) must be in 1 .. 16"), (O(beam_size=1, patience=0.2), r"round\(beam_size \* patience\) must be in 1 .. 16"),
                    (O(beam_size=2, temperature=0.5), "beam search runs at temperature 0"),
                    (O(beam_size=2, language="en"), "tokenizer is not built"), (O(beam_size=2, language=0, prompt="hi"), "prompt must be a list of token ids"),
                    (O(beam_size=2, language=0, prefix="hi"), "prefix must be a list of token ids"), (O(beam_size=2, task="lang_id"), "call decode"),
                    (O(beam_size=2, task="sing"), "unknown task")):
        with pytest.raises(ValueError, match=word):
            v(o)
    ok = O(beam_size=8, patience=2.0, language=3, length_penalty=0.6)
    assert v(ok) is ok and v(O(beam_size=1)) == O(beam_size=1)
    assert WB.max_candidates(5, None) == 5 and WB.max_candidates(5, 1.5) == 8 and WB.max_candidates(3, 0.5) == 2 and WB.max_candidates(8, 2.0) == 16
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):  # the pinned refusals are not this module's to lift
        WD.verify_options(O(beam_size=2))
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
        WS.verify_sampling_options(O(temperature=0.5, beam_size=2))
    m = whisper.Model(T.dims(128, 2, 2, 300, 50, 32))  # encoder-only
    for call in (m.beam_search, m.beam_candidates, m.beam_decode_with_fallback):
        with pytest.raises(NotImplementedError, match="text decoder: not built"):
            call(np.zeros((100, 80), np.float32))


def test_the_fallback_routes_temperature_zero_to_beam_search_and_the_rest_to_sample():
    import torch

    d = T.dims(128, 2, 2, 300, 50, 32)
    seen = []

    class Fake:
        dims, device = d, torch.device("cpu")

        def decode(self, feats, options):
            seen.append(("decode", tuple(feats.shape), options))
            return [SimpleNamespace(avg_logprob=-9.0, no_speech_prob=0.0, temperature=0.0) for _ in range(feats.shape[0])]

    def fake_beam(model, feats, options):
        seen.append(("beam", tuple(feats.shape), options))
        return [SimpleNamespace(avg_logprob=-9.0 if i != 1 else -0.1, no_speech_prob=0.0, temperature=0.0) for i in range(feats.shape[0])]

    def fake_sample(model, feats, options, seed, streams):
        seen.append(("sample", tuple(feats.shape), options, seed, list(streams)))
        return [SimpleNamespace(avg_logprob=-9.0 if s == 2 else -0.1, no_speech_prob=0.0, temperature=options.temperature) for s in streams]

    feats = np.zeros((3, d.n_audio_ctx, d.n_audio_state), np.float32)
    real = WB.beam_search, WS.sample
    WB.beam_search, WS.sample = fake_beam, fake_sample
    try:
        out = WB.decode_with_fallback(Fake(), feats, temperature=(0.0, 0.5, 1.0), seed=4, beam_size=3, best_of=2, patience=2.0, language=2)
        assert [r.temperature for r in out] == [0.5, 0.0, 1.0]
        assert seen[0] == ("beam", (3, 50, 128), O(language=2, beam_size=3, patience=2.0))  # beam search ONCE, best_of dropped
        assert seen[1] == ("sample", (2, 50, 128), O(language=2, best_of=2, temperature=0.5), 4, [0, 2])  # beam_size and patience dropped, original indices
        assert seen[2] == ("sample", (1, 50, 128), O(language=2, best_of=2, temperature=1.0), 4, [2]) and len(seen) == 3
        del seen[:]
        one = WB.decode_with_fallback(Fake(), feats[0], temperature=0.0, language=2)  # the defaults are OpenAI's pairing: beam_size 5 (and best_of 5)
        assert one.temperature == 0.0 and seen == [("beam", (1, 50, 128), O(language=2, beam_size=5))]
        del seen[:]
        WB.decode_with_fallback(Fake(), feats[:1], temperature=0.3, language=2)
        assert seen == [("sample", (1, 50, 128), O(language=2, best_of=5, temperature=0.3), 0, [0])]
        del seen[:]
        WB.decode_with_fallback(Fake(), feats[:1], temperature=0.0, beam_size=None, patience=None, language=2)  # no beam: greedy decode
        assert seen == [("decode", (1, 50, 128), O(language=2))]
        with pytest.raises(ValueError, match="at least one temperature"):
            WB.decode_with_fallback(Fake(), feats, temperature=())
    finally:
        WB.beam_search, WS.sample = real


def test_the_library_declares_the_beam_entries_and_refuses_without_a_gpu():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 23 and _lib.WHISPER_MAX_GROUP == WB.MAX_GROUP  # (minor 22 went to the fused conv kernels' epilogue switch)
    cfg = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=1, n_audio_ctx=1500, n_audio_state=384)
    h = C.c_void_p()
    assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**cfg)), C.byref(h)) == 0
    grouped = lib.kk_whisper_text_state_bytes_groups(h, 2, 3)
    need = lib.kk_whisper_text_beam_state_bytes(h, 2, 3, 3)
    assert 2 * 6 * 448 * 4 + 6 * 448 * 4 < need < 2 * 6 * 448 * 4 + 6 * 448 * 4 + 64 * 256  # two owner tables and the finished tokens, little else
    assert lib.kk_whisper_text_state_bytes_groups(h, 2, 3) == grouped  # the window state keeps its size
    for bad in ((0, 3, 3), (2, 0, 3), (2, 9, 3), (2, 3, 0), (2, 3, 17)):
        assert lib.kk_whisper_text_beam_state_bytes(h, *bad) == 0
    buf = (C.c_char * 64)()
    n = C.c_int32()
    assert lib.kk_whisper_text_beam_setup(h, None, 3, 3, C.cast(buf, C.c_void_p), 64) != 0 and b"set_audio_groups first" in lib.kk_last_error()
    assert lib.kk_whisper_text_beam_not_complete(h, None, C.byref(n)) != 0 and b"beam_setup first" in lib.kk_last_error()
    one = C.c_void_p(16)
    assert lib.kk_whisper_text_beam_read(h, None, 4, one, one, one, one, one, one, one) != 0 and b"beam_setup first" in lib.kk_last_error()
    lib.kk_whisper_text_destroy(h)
    # the raw entries refuse their arguments before anything is launched (the pointers are never looked at)
    for k in (0, 9):
        assert lib.kk_op_whisper_beam_topk(None, 1, k, one, 8, one, None, one, one, one) != 0 and b"beam_size" in lib.kk_last_error()
    assert lib.kk_op_whisper_beam_topk(None, 1, 2, None, 8, one, None, one, one, one) != 0 and b"null argument" in lib.kk_last_error()

    def bufs(**kw):
        b = _lib.KKWhisperBeamBufs(n_audio=1, beam_size=2, max_candidates=2, n_ctx=8, cap=8)
        for name in ("cand_token", "cand_logprob", "parent", "fin_score", "fin_length", "fin_tokens", "fin_count", "complete", "not_complete"):
            setattr(b, name, 16)
        b.owner[0] = b.owner[1] = 16
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    for kw, word in ((dict(beam_size=9), b"beam_size"), (dict(max_candidates=17), b"max_candidates"), (dict(max_candidates=0), b"max_candidates"),
                     (dict(n_audio=0), b"n_audio"), (dict(parent=None), b"null buffer")):
        assert lib.kk_op_whisper_beam_select(None, C.byref(bufs(**kw)), 0, 4, one, one, one, one) != 0 and word in lib.kk_last_error()
        assert lib.kk_op_whisper_beam_reset(None, C.byref(bufs(**kw))) != 0 and word in lib.kk_last_error()
    assert lib.kk_op_whisper_beam_select(None, C.byref(bufs()), 2, 4, one, one, one, one) != 0 and b"flip" in lib.kk_last_error()
    assert lib.kk_op_whisper_beam_select(None, C.byref(bufs()), 0, 9, one, one, one, one) != 0 and b"pos = 9" in lib.kk_last_error()
    assert lib.kk_op_whisper_beam_select(None, C.byref(bufs()), 0, 4, one, None, one, one) != 0 and b"null argument" in lib.kk_last_error()
    assert lib.kk_op_whisper_attn_rows_owned(None, 1, 2, one, one, 0, 128, 1, 8, 250, one, one, one, one, 1 << 20) != 0 and b"multiples of 8" in lib.kk_last_error()


def test_the_margin_condition_holds_on_the_gpu_kernel_tests_own_inputs():
    """Every decision the GPU kernel tests compare -- the order of a row's K + 2 best filtered logits (the planted equal ones aside), and every adjacent pair
    of the select walk that has a visited member -- is decided by at least 1e-3, ten times the 1e-4 the project allows on a sum of log-probabilities:
    fp32 on the device and float64 here cannot order them differently."""
    for V in BR.TOPK_VOCABS:
        P, rows = BR.topk_case(V)
        for name, ts, sampled, sup, x in rows:
            f = T.filter_logits(x, sampled, P[ts], suppress=sup)
            m = BR.topk_margin(f, BR.TOPK_K, planted="planted" in name)
            print(f"top-k V {V} {name}: margin {m:.4g}")
            assert m >= BR.MARGIN, (V, name, m)
    for K in BR.SELECT_KS:
        wins = BR.select_replay(K)
        m = min(min(w.margins) for w in wins)
        print(f"select K {K}: margin {m:.4g}, finished {[len(w.finished) for w in wins]}, complete {[w.complete for w in wins]}, "
              f"dead {[sum(not w.live(j) for j in range(K)) for w in wins]}")
        assert m >= BR.MARGIN, (K, m)
        # what the scripts are there to exercise: finished sequences in both windows, dead slots, and (K 1 and 3) a complete window that keeps stepping
        assert all(w.finished for w in wins) and any(-1 in p for p in wins[1].parents) and (K == 8 or any(w.completes[2] for w in wins))
