"""Whisper token timestamps, host half (mlx-audio_amd/whisper_timing.py, whisper.Model's alignment heads) and the CPU references of the GPU tests
(tests/_whisper_align_ref.py), pinned against transformers' `_dynamic_time_warping` and `_median_filter`.  No GPU."""
import base64
import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_align_ref as A  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_timing as WT  # noqa: E402


# ---- the restatements -------------------------------------------------------------------------------------------------------------------------
def _dtw_inputs():
    g = np.random.default_rng(0)
    for n, m in ((1, 1), (1, 9), (7, 1), (5, 13), (23, 40), (40, 23)):
        yield g.standard_normal((n, m)).astype(np.float32)
        yield np.zeros((n, m), np.float32)  # every comparison a tie
        yield g.integers(-2, 3, (n, m)).astype(np.float32)  # many ties, every branch


def test_the_restated_dtw_equals_transformers():
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping

    seen = set()
    for x in _dtw_inputs():
        ti, tj = A.dtw(x)
        hi, hj = _dynamic_time_warping(x)
        assert np.array_equal(ti, hi) and np.array_equal(tj, hj), x.shape
        assert ti[0] == 0 and tj[0] == 0 and ti[-1] == x.shape[0] - 1 and tj[-1] == x.shape[1] - 1
        assert np.array_equal(A.first_cols(ti, tj, x.shape[0]), A.jumps(ti, tj))
        assert np.array_equal(WT.jump_frames(ti, tj), A.jumps(ti, tj))
        seen |= set(zip(np.diff(ti).tolist(), np.diff(tj).tolist()))
    assert seen == {(1, 1), (1, 0), (0, 1)}  # diagonal, up and left all occur


def test_the_restated_dtw_finishes_on_nan_and_inf():
    """NaN: every comparison is false, the rule says "left" everywhere, and the path leaves through column 0 (time index -1) as the reference's does"""
    x = np.full((3, 4), np.nan, np.float32)
    ti, tj = A.dtw(x)
    assert ti.tolist() == [0, 1, 2, 2, 2, 2, 2] and tj.tolist() == [-1, -1, -1, 0, 1, 2, 3]
    assert A.first_cols(ti, tj, 3).tolist() == [-1, -1, -1]
    x = np.random.default_rng(1).standard_normal((6, 9)).astype(np.float32)
    x[2, 3:] = np.inf
    ti, tj = A.dtw(x)
    assert len(ti) <= 6 + 9 and ti[-1] == 5 and tj[-1] == 8


@pytest.mark.parametrize("width", [1, 3, 7, 9])
@pytest.mark.parametrize("n", [3, 4, 5, 40])
def test_the_restated_median_filter_equals_transformers(n, width):
    import torch
    from transformers.models.whisper.generation_whisper import _median_filter

    g = np.random.default_rng(n * 100 + width)
    for x in (g.standard_normal((2, 5, n)).astype(np.float32), g.integers(0, 3, (2, 5, n)).astype(np.float32)):
        want = _median_filter(torch.from_numpy(x)[None], width)[0].numpy()
        assert np.array_equal(A.median_filter(x, width), want)
    if n <= width // 2:
        assert A.median_filter(x, width) is x  # timing.py:22-24


def test_the_alignment_matrix_restatement_is_the_reference_pipeline():
    g = np.random.default_rng(3)
    qk = g.standard_normal((3, 6, 11))
    m = A.align_matrix(qk, 0.5, 3)
    w = np.exp(0.5 * qk)
    w /= w.sum(-1, keepdims=True)
    z = (w - w.mean(-2, keepdims=True)) / w.std(-2, keepdims=True)
    pad = np.pad(z, ((0, 0), (0, 0), (1, 1)), mode="reflect")
    want = np.median(np.stack([pad[..., i:i + 11] for i in range(3)]), axis=0).mean(0)
    assert np.allclose(m, want, rtol=0, atol=1e-12)


# ---- the alignment heads ----------------------------------------------------------------------------------------------------------------------
def _host_model(**shape):
    """a Model whose text side counts as built: the heads are host state, nothing here reaches the device"""
    m = whisper.Model(T.dims(**shape))
    m._text = object()
    return m


def test_default_alignment_heads_are_the_upper_half_of_the_layers():
    m = _host_model(width=256, heads=4, layers=5, n_vocab=51865, audio_ctx=100)
    h = m.alignment_heads
    assert h.shape == (12, 2) and h.tolist() == [[l, k] for l in (2, 3, 4) for k in range(4)]
    assert _host_model(**T.SHAPE_B).alignment_heads.tolist() == [[0, k] for k in range(6)]  # one layer: 1 // 2 = 0
    m._text = None


def test_set_alignment_heads():
    m = _host_model(width=256, heads=4, layers=3, n_vocab=51865, audio_ctx=100)
    m.set_alignment_heads(np.array([[2, 1], [0, 3]]))
    assert m.alignment_heads.tolist() == [[2, 1], [0, 3]]  # the order is kept
    mask = np.zeros((3, 4), bool)
    mask[1, 2] = mask[2, 0] = mask[0, 3] = True
    m.set_alignment_heads(base64.b85encode(gzip.compress(mask.tobytes())))
    assert m.alignment_heads.tolist() == [[0, 3], [1, 2], [2, 0]]
    with pytest.raises(ValueError, match="Invalid type for `dump`"):
        m.set_alignment_heads([[0, 1]])
    with pytest.raises(ValueError, match="Invalid type for `dump`"):
        m.set_alignment_heads("ABzY8")
    for bad in (np.array([[3, 0]]), np.array([[0, 4]]), np.array([[-1, 0]]), np.array([0, 1]), np.zeros((0, 2), int), np.array([[0.0, 1.0]])):
        with pytest.raises(ValueError):
            m.set_alignment_heads(bad)
    with pytest.raises(ValueError, match="mask holds"):
        m.set_alignment_heads(base64.b85encode(gzip.compress(np.zeros((2, 4), bool).tobytes())))
    assert m.alignment_heads.tolist() == [[0, 3], [1, 2], [2, 0]]  # a refused dump leaves the heads as they were
    m._text = None


def test_an_encoder_only_model_refuses_the_alignment_surface():
    m = whisper.Model(T.dims(**T.SHAPE_A))
    assert not m.has_text_decoder
    x = np.zeros((100, 128), np.float32)
    for call in (lambda: m.alignment_heads, lambda: m.set_alignment_heads(np.array([[0, 0]])), lambda: m.forward_with_cross_qk(x[None], np.zeros((1, 3), int)),
                 lambda: whisper.find_alignment(m, [1, 2], x, 200), lambda: WT.find_alignment(m, [[1, 2]], x[None], [200])):
        with pytest.raises(NotImplementedError, match="text decoder: not built"):
            call()
    assert whisper.find_alignment(m, [], x, 200) == []  # timing.py:122-123, before anything else
    for name in ("find_alignment", "dtw", "median_filter", "TokenTiming", "WordTiming"):
        assert getattr(whisper, name) is getattr(WT, name)


def test_load_weights_keeps_ignoring_a_checkpoints_alignment_heads():
    d = T.dims(128, 2, 2, 300, 50, 32)
    w = {k: np.zeros(s, np.float32) for k, s in whisper.decoder_shapes(d).items()}
    assert set(whisper.decoder_tensors(d, dict(w, alignment_heads=b"not a dump"))) == set(w)


# ---- what find_alignment builds -----------------------------------------------------------------------------------------------------------------
def test_the_token_sequence_and_the_warped_rows():
    tok = whisper.special_tokens(T.dims(**T.SHAPE_A))  # multilingual, 51865
    seq, r0, r1 = WT.alignment_tokens(T.dims(**T.SHAPE_A), [11, 12, 13])
    assert seq == [tok.sot, tok.language_tokens[0], tok.transcribe, tok.no_timestamps, 11, 12, 13, tok.eot] and (r0, r1) == (3, 7)
    seq, r0, r1 = WT.alignment_tokens(T.dims(**T.SHAPE_A), [5], language=4, task="translate")
    assert seq == [tok.sot, tok.language_tokens[4], tok.translate, tok.no_timestamps, 5, tok.eot] and (r0, r1) == (3, 5)
    assert WT.alignment_tokens(T.dims(**T.SHAPE_A), [5], language=tok.language_tokens[7])[0][1] == tok.language_tokens[7]
    en = T.dims(128, 2, 1, 51864, 100)
    ten = whisper.special_tokens(en)
    seq, r0, r1 = WT.alignment_tokens(en, [9, 8])
    assert seq == [ten.sot, ten.no_timestamps, 9, 8, ten.eot] and (r0, r1) == (1, 4)  # rows: no_timestamps, 9, 8
    with pytest.raises(ValueError, match="tokenizer is not built"):
        WT.alignment_tokens(en, [9], language="en")


def test_word_boundaries_on_a_hand_made_path():
    """4 text tokens -> 5 warped rows (no_timestamps first); the path enters them at frames 0, 0, 3, 4, 9"""
    ti = np.array([0, 1, 1, 1, 2, 3, 3, 3, 3, 3, 4, 4])
    tj = np.array([0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
    first = WT.jump_frames(ti, tj)
    assert first.tolist() == [0, 0, 3, 4, 9]
    probs = np.array([0.5, 0.25, 0.75, 1.0])
    words = WT.word_timings([[101], [102, 103], [104]], first, probs)
    assert [(w.word, w.tokens, w.start, w.end, w.probability) for w in words] == [("", [101], 0.0, 0.0, 0.5), ("", [102, 103], 0.0, 0.08, 0.5),
                                                                                  ("", [104], 0.08, 0.18, 1.0)]
    # the reference's own arithmetic on the same path (timing.py:167-176), the eot word appended as split_to_word_tokens does
    word_tokens = [[101], [102, 103], [104], [50257]]
    wb = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jt = first / whisper.TOKENS_PER_SECOND
    assert [w.start for w in words] == jt[wb[:-1]].tolist() and [w.end for w in words] == jt[wb[1:]].tolist()
    assert WT.word_timings([], first, probs) == []
    with pytest.raises(ValueError, match="concatenate"):
        WT.word_timings([[101], [102]], first, probs)


# ---- the library's argument checks ----------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_bad_alignment_arguments_without_a_gpu():
    import ctypes as C

    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 16
    p = C.c_void_p(256)  # never dereferenced: every call below is refused before a launch

    def dtw(rows_max=4, cols_max=8, ld=8, stride=32, ws=1 << 20):
        return lib.kk_op_whisper_dtw(None, 1, p, stride, ld, p, rows_max, p, cols_max, 0, p, p, p, p, p, ws)

    for kw, word in ((dict(rows_max=0), b"n_rows >= 1"), (dict(cols_max=0), b"n_cols >= 1"), (dict(cols_max=9), b"exceeds the leading dimension"),
                     (dict(rows_max=5), b"do not fit the item stride"), (dict(ws=8), b"workspace too small"),
                     (dict(cols_max=20000, ld=20000, stride=80000), b"at most 15360 columns")):
        assert dtw(**kw) != 0
        assert word in lib.kk_last_error(), (kw, lib.kk_last_error())
    assert lib.kk_op_whisper_dtw(None, 1, None, 32, 8, p, 4, p, 8, 0, p, p, p, p, p, 1 << 20) != 0 and b"null" in lib.kk_last_error()
    assert lib.kk_op_whisper_dtw_workspace_bytes(2, 444, 1500) == 2 * 444 * 94 * 4 and lib.kk_op_whisper_dtw_workspace_bytes(0, 4, 8) == 0

    def align(width=7, rows_max=4, cols_max=8, ld_in=8, ld_out=8, group=0, ws=1 << 20):
        return lib.kk_op_whisper_align_matrix(None, 1, 3, p, 96, 32, ld_in, p, rows_max, p, cols_max, 1.0, width, group, p, ld_out, p, ws)

    for kw, word in ((dict(width=4), b"must be odd"), (dict(width=0), b"must be odd"), (dict(width=33), b"within 1 .. 31"), (dict(rows_max=0), b"n_rows >= 1"),
                     (dict(cols_max=0), b"n_cols >= 1"), (dict(cols_max=9), b"exceeds a leading dimension"), (dict(ld_out=7), b"exceeds a leading dimension"),
                     (dict(rows_max=5), b"do not fit the head stride"), (dict(ws=16), b"workspace too small"), (dict(group=-1), b"group >= 0")):
        assert align(**kw) != 0
        assert word in lib.kk_last_error(), (kw, lib.kk_last_error())
    # the workspace holds one group of heads, however many heads there are
    assert lib.kk_op_whisper_align_matrix_workspace_bytes(1, 320, 448, 750, 0) == lib.kk_op_whisper_align_matrix_workspace_bytes(1, 8, 448, 750, 0)
    assert lib.kk_op_whisper_align_matrix_workspace_bytes(1, 320, 448, 750, 4) == 4 * 448 * 750 * 4
    sel = (C.c_int32 * 2)(0, 5)
    assert lib.kk_op_whisper_qk_rows(None, 1, 4, 2, p, p, 100, 256, sel, 2, 50, p, 50) != 0 and b"sel[1] = 5" in lib.kk_last_error()
    assert lib.kk_op_whisper_qk_rows(None, 1, 4, 2, p, p, 100, 256, sel, 1, 101, p, 101) != 0 and b"n_keys" in lib.kk_last_error()
    assert lib.kk_op_whisper_median_filter(None, 2, 8, p, 8, 4, p, 8) != 0 and b"must be odd" in lib.kk_last_error()
    assert lib.kk_op_whisper_median_filter(None, 2, 3, p, 8, 7, p, 8) != 0 and b"no longer than the padding" in lib.kk_last_error()
