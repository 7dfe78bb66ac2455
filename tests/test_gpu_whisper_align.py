"""Whisper's token timestamps end to end on the device (mlx-audio_amd/whisper_timing.py, whisper.Model.forward_with_cross_qk) on the synthetic
decoders of tests/_whisper_text_ref.py: the captured scores and the alignment matrix against transformers' fp32 WhisperDecoder (its cross-attentions through
the float64 restatement of timing.py:147-155), the path exactly the restated DTW of the device's own matrix, and the structure of what `find_alignment` returns."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_align_ref as A  # noqa: E402
import _whisper_ref as R  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_timing as WT  # noqa: E402

SHAPES = {"a": T.SHAPE_A, "b": T.SHAPE_B}
_models, _hf = {}, {}


def _model(name):
    if name not in _models:
        d = T.dims(**SHAPES[name])
        w = T.decoder_weights(d, 21)
        m = whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **w})
        _models[name] = (d, m, T.hf_decoder(d, w))
    return _models[name]


def _text(d, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, whisper.special_tokens(d).eot, n)]


def _hf_cross(name, seq, feats, bf16):
    """transformers' cross-attention probabilities of one sequence, [layer] of float64 (H, S, ctx); computed once per input and kept"""
    import torch

    key = (name, tuple(seq), feats.tobytes()[:64], bf16)
    if key not in _hf:
        dec = _model(name)[2]
        ids = torch.tensor([seq], dtype=torch.long)
        xa = torch.from_numpy(feats[None])
        with torch.no_grad():
            if bf16:
                out = copy.deepcopy(dec).bfloat16()(input_ids=ids, encoder_hidden_states=xa.bfloat16(), use_cache=False, output_attentions=True)
            else:
                out = dec(input_ids=ids, encoder_hidden_states=xa, use_cache=False, output_attentions=True)
        _hf[key] = [a[0].double().numpy() for a in out.cross_attentions]
    return _hf[key]


def _pipeline(cross, heads, n_frames, r0, r1, width=7, qk_scale=1.0):
    """the module's cross-attention of the alignment heads, cropped to n_frames and renormalised (= the softmax of the cropped scores), through
    timing.py:149-156 in float64; qk_scale != 1 re-scales the logarithms first"""
    w = np.stack([cross[l][h][:, :n_frames] for l, h in heads])
    if qk_scale != 1.0:
        w = np.exp(qk_scale * np.log(w))
    w = w / w.sum(-1, keepdims=True)
    return A.standardise_filter_mean(w, width)[r0:r1]


@pytest.mark.parametrize("name,n_tokens", [("a", 9), ("b", 20)])
def test_forward_with_cross_qk(name, n_tokens):
    """the logits are Model.logits bit for bit; softmax(qk) of every layer and head against the fp32 module's cross-attention, at most 1.5 x the relative
    rms error of the same module in bf16 on the CPU (the bar of DESIGN 8g)"""
    import torch

    d, m, _ = _model(name)
    toks = np.random.default_rng(n_tokens).integers(0, d.n_vocab, (2, n_tokens)).astype(np.int64)
    feats = T.features(d, 2, 31)
    logits, qk = m.forward_with_cross_qk(feats, toks)
    assert len(qk) == d.n_text_layer and all(tuple(q.shape) == (2, d.n_text_head, n_tokens, d.n_audio_ctx) and q.dtype == torch.float32 for q in qk)
    assert torch.equal(logits, m.logits(toks, feats))
    for b in range(2):
        ref = _hf_cross(name, toks[b].tolist(), feats[b], False)
        own = _hf_cross(name, toks[b].tolist(), feats[b], True)
        for l in range(d.n_text_layer):
            got = torch.softmax(qk[l][b].double(), dim=-1).cpu().numpy()
            err, bar = R.rel_rms(got, ref[l]), R.rel_rms(own[l], ref[l])
            print(f"shape {name} item {b} layer {l}: softmax(qk) rel rms {err:.5f}, the module in bf16 {bar:.5f}, ratio {err / bar:.3f}")
            assert err <= 1.5 * bar
    alone = m.forward_with_cross_qk(feats[1:], toks[1:])  # a row alone: the bits it has in the batch
    assert torch.equal(alone[0][0], logits[1]) and all(torch.equal(alone[1][l][0], qk[l][1]) for l in range(d.n_text_layer))
    mel = np.random.default_rng(0).standard_normal((1, 2 * d.n_audio_ctx, d.n_mels)).astype(np.float32)  # a mel goes through the encoder first
    assert tuple(m.forward_with_cross_qk(mel, toks[:1])[1][0].shape) == (1, d.n_text_head, n_tokens, d.n_audio_ctx)


CASES = [("a", 12, 146), ("b", 37, 3000), ("b", 37, 1222)]


@pytest.mark.parametrize("name,n_tokens,num_frames", CASES)
def test_find_alignment_matrix_path_and_structure(name, n_tokens, num_frames):
    d, m, _ = _model(name)
    tok = whisper.special_tokens(d)
    text, feats = _text(d, n_tokens, 3), T.features(d, 1, 41)[0]
    seq, r0, r1 = WT.alignment_tokens(d, text)
    F = num_frames // 2
    al = WT.alignment_details(m, [text], feats[None], num_frames)[0]
    mat = al.matrix.cpu().numpy()
    assert mat.shape == (n_tokens + 1, F)
    # (1) the matrix: against the fp32 module through the float64 pipeline, at most 1.5 x what the module in bf16 shows through the same pipeline
    heads = m.alignment_heads.tolist()
    ref = _pipeline(_hf_cross(name, seq, feats, False), heads, F, r0, r1)
    own = _pipeline(_hf_cross(name, seq, feats, True), heads, F, r0, r1)
    err, bar = A.rms(mat - ref) / A.rms(ref), A.rms(own - ref) / A.rms(ref)
    print(f"shape {name} tokens {n_tokens} frames {F}: matrix rms {A.rms(ref):.3f}, rel rms {err:.5f} (rms diff {A.rms(mat - ref):.5f}), the module in bf16 "
          f"{bar:.5f} (rms diff {A.rms(own - ref):.5f}), ratio {err / bar:.3f}")
    assert err <= 1.5 * bar
    # (2) the path: exactly the restated DTW of the device's own matrix
    ri, rj = A.dtw(-mat)
    assert np.array_equal(al.text_indices, ri) and np.array_equal(al.time_indices, rj)
    first = A.first_cols(ri, rj, n_tokens + 1)
    assert np.array_equal(al.first_frames, first) and np.array_equal(first, A.jumps(ri, rj))
    # (3) what find_alignment returns
    res = whisper.find_alignment(m, text, feats, num_frames)
    assert [t.token for t in res] == text and all(isinstance(t, whisper.TokenTiming) for t in res)
    assert [t.start for t in res] == (first[:-1] / whisper.TOKENS_PER_SECOND).tolist() and [t.end for t in res] == (first[1:] / whisper.TOKENS_PER_SECOND).tolist()
    assert all(a.start <= b.start and a.end == b.start for a, b in zip(res, res[1:])) and res[-1].end <= (F - 1) / whisper.TOKENS_PER_SECOND
    lg = m.logits(np.asarray([seq]), feats[None]).cpu().numpy()[0, r0:r0 + n_tokens, : tok.eot].astype(np.float64)
    p = np.exp(lg - lg.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    assert max(abs(t.probability - p[i, text[i]]) for i, t in enumerate(res)) < 1e-6
    cut = [text[:1], text[1:5], text[5:]]
    ws = whisper.find_alignment(m, text, feats, num_frames, words=cut)
    assert all(isinstance(w, whisper.WordTiming) and w.word == "" for w in ws) and [w.tokens for w in ws] == cut
    assert [w.start for w in ws] == [res[0].start, res[1].start, res[5].start] and [w.end for w in ws] == [res[0].end, res[4].end, res[-1].end]
    assert abs(ws[1].probability - np.mean([t.probability for t in res[1:5]])) < 1e-6
    with pytest.raises(ValueError, match="concatenate"):
        whisper.find_alignment(m, text, feats, num_frames, words=cut[:2])


def test_find_alignment_batch_is_bit_equal_to_the_single_calls():
    d, m, _ = _model("a")
    feats = T.features(d, 3, 43)
    texts, frames = [_text(d, 12, 1), _text(d, 3, 2), _text(d, 30, 3)], [146, 200, 51]
    batch = whisper.find_alignment(m, texts, feats, frames)
    details = WT.alignment_details(m, texts, feats, frames)
    assert len(batch) == 3
    for b in range(3):
        one = whisper.find_alignment(m, texts[b], feats[b], frames[b])
        assert one == batch[b] and len(one) == len(texts[b])
        alone = WT.alignment_details(m, [texts[b]], feats[b:b + 1], frames[b])[0]
        assert np.array_equal(alone.matrix.cpu().numpy(), details[b].matrix.cpu().numpy())
        assert np.array_equal(alone.text_indices, details[b].text_indices) and np.array_equal(alone.time_indices, details[b].time_indices)
        assert np.array_equal(alone.probabilities, details[b].probabilities)
    mixed = whisper.find_alignment(m, [texts[0], [], texts[2]], feats, frames)  # an item without text: [], the others as before
    assert mixed[1] == [] and mixed[0] == batch[0] and mixed[2] == batch[2]
    assert whisper.find_alignment(m, [], feats[0], 146) == []
    same = whisper.find_alignment(m, texts, feats, 146)  # one num_frames for all
    assert same[0] == batch[0] and len(same[2]) == 30
    with pytest.raises(ValueError, match="n_text_ctx"):
        whisper.find_alignment(m, _text(d, d.n_text_ctx, 0), feats[0], 146)
    with pytest.raises(ValueError, match="num_frames"):
        whisper.find_alignment(m, texts[0], feats[0], 1)


def test_find_alignment_honours_width_scale_language_and_the_heads():
    d, m, _ = _model("a")
    tok = whisper.special_tokens(d)
    text, feats = _text(d, 12, 3), T.features(d, 1, 41)[0]
    F = 73
    base = WT.alignment_details(m, [text], feats[None], 146)[0].matrix.cpu().numpy()
    try:
        for kw in (dict(medfilt_width=1), dict(qk_scale=0.5), dict(medfilt_width=9, qk_scale=0.5)):
            al = WT.alignment_details(m, [text], feats[None], 146, **kw)[0]
            mat = al.matrix.cpu().numpy()
            assert not np.array_equal(mat, base)
            seq, r0, r1 = WT.alignment_tokens(d, text)
            heads = m.alignment_heads.tolist()
            args = (kw.get("medfilt_width", 7), kw.get("qk_scale", 1.0))
            ref = _pipeline(_hf_cross("a", seq, feats, False), heads, F, r0, r1, *args)
            own = _pipeline(_hf_cross("a", seq, feats, True), heads, F, r0, r1, *args)
            err, bar = A.rms(mat - ref) / A.rms(ref), A.rms(own - ref) / A.rms(ref)
            print(f"{kw}: rel rms {err:.5f}, the module in bf16 {bar:.5f}, ratio {err / bar:.3f}")
            assert err <= 1.5 * bar
            ri, rj = A.dtw(-mat)
            assert np.array_equal(al.text_indices, ri) and np.array_equal(al.time_indices, rj)
        # another language and task change the prompt, hence the scores
        seq, r0, r1 = WT.alignment_tokens(d, text, language=4, task="translate")
        al = WT.alignment_details(m, [text], feats[None], 146, language=4, task="translate")[0]
        ref = _pipeline(_hf_cross("a", seq, feats, False), m.alignment_heads.tolist(), F, r0, r1)
        own = _pipeline(_hf_cross("a", seq, feats, True), m.alignment_heads.tolist(), F, r0, r1)
        assert seq[1] == tok.language_tokens[4] and A.rms(al.matrix.cpu().numpy() - ref) <= 1.5 * A.rms(own - ref)
        # chosen heads, in the caller's order, from both layers
        m.set_alignment_heads(np.array([[1, 0], [0, 1], [1, 1]]))
        al = WT.alignment_details(m, [text], feats[None], 146)[0]
        seq, r0, r1 = WT.alignment_tokens(d, text)
        ref = _pipeline(_hf_cross("a", seq, feats, False), [[1, 0], [0, 1], [1, 1]], F, r0, r1)
        own = _pipeline(_hf_cross("a", seq, feats, True), [[1, 0], [0, 1], [1, 1]], F, r0, r1)
        assert A.rms(al.matrix.cpu().numpy() - ref) <= 1.5 * A.rms(own - ref)
    finally:
        m._alignment_heads = None  # the model is shared with the other tests: back to the default heads
