"""MLX 4- / 8-bit Whisper checkpoints on the device (mlx-audio_amd/whisper.py, quant.py, csrc/kk_whisper_text.hip): a quantised SHAPE_A
checkpoint on disk loads with a weight_storage, and with "packed" -- the decoder's matrices and the token embedding kept as the checkpoint's integers --
every logit and every decoding path gives what "dequantized" gives on the same file, with `==`."""
import json
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

from mlx_audio_amd import quant, whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

GROUP = 64
MIXED = {"decoder.blocks.0.mlp1": {"group_size": 32, "bits": 8}, "decoder.blocks.1.attn.out": False}
_weights = {}


def _float_weights():
    if "w" not in _weights:
        d = T.dims(**T.SHAPE_A)
        _weights["w"] = (d, {**R.encoder_weights(d, 5), **T.decoder_weights(d, 21)})
    return _weights["w"]


def _write(path, kind):
    """SHAPE_A as `convert(..., quantize=True)` leaves it: config.json with "quantization", weights.npz with the triplets.  kind 4 / 8: every Linear and
    the embedding at that width; "mixed": a 4-bit file with one matrix at 8 bits in groups of 32 and one left unquantised, by per-layer entries."""
    d, w = _float_weights()
    names = quant.whisper_quantised_layer_names(w, GROUP)
    cfg = {"group_size": GROUP, "bits": 4 if kind == "mixed" else kind}
    if kind == "mixed":
        cfg.update(MIXED)
        eight, plain = (k + ".weight" for k in MIXED)
        q = quant.quantize_checkpoint(w, GROUP, 4, names=[k for k in names if k not in (eight, plain)])
        q.update(quant.quantize_checkpoint({eight: w[eight]}, 32, 8, names=[eight]))
    else:
        q = quant.quantize_checkpoint(w, GROUP, kind, names=names)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(dict({k: int(getattr(d, k)) for k in whisper.DIMENSION_KEYS}, quantization=cfg), f)
    np.savez(os.path.join(path, "weights.npz"), **q)
    return d


@pytest.fixture(scope="module", params=[4, 8, "mixed"])
def pair(request, tmp_path_factory):
    """(dims, directory, the packed model, its dequantised twin) of one checkpoint on disk"""
    path = str(tmp_path_factory.mktemp(f"whisper_q{request.param}"))
    d = _write(path, request.param)
    packed = whisper.Model.from_pretrained(path, weight_storage="packed")
    deq = whisper.load_model(path, weight_storage="dequantized")
    assert packed.has_text_decoder and deq.has_text_decoder
    return dict(kind=request.param, d=d, path=path, packed=packed, deq=deq)


def test_a_quantised_directory_needs_a_weight_storage(pair):
    with pytest.raises(ValueError, match="quantised Whisper checkpoints are not supported yet"):
        whisper.Model.from_pretrained(pair["path"])
    from mlx_audio_amd.utils import load_model

    m = load_model(pair["path"], weight_storage="packed")
    assert m.has_text_decoder and m.weight_report()["packed"] > 0


def test_weight_report(pair):
    d, kind = pair["d"], pair["kind"]
    rp, rd = pair["packed"].weight_report(), pair["deq"].weight_report()
    n = 9 * d.n_text_layer + 1  # per layer: four self, three cross (key | value stacked) and two MLP matrices; the embedding
    assert rd["packed"] == 0 and rd["bf16"] == n and rd["fallbacks"] == {}
    stacked = {f"decoder.blocks.{i}.cross_attn.{p}.weight" for i in range(d.n_text_layer) for p in ("key", "value")}
    assert set(rp["fallbacks"]) == stacked and all("cross key | value" in why for why in rp["fallbacks"].values())  # named, as bf16
    unquantised = 1 if kind == "mixed" else 0
    assert rp["bf16"] == d.n_text_layer + unquantised and rp["packed"] == n - rp["bf16"]
    assert rp["matrix_bytes"] < rd["matrix_bytes"] and rp["resident_bytes"] < rd["resident_bytes"]
    # the embedding dominates this shape: bits / 16 of its bf16 bytes plus a float pair per group of 64 (8 / 128)
    bits = 8 if kind == 8 else 4
    assert rp["matrix_bytes"] < (bits / 16 + 8 / 128 + 0.03) * rd["matrix_bytes"]
    print(f"kind {kind}: packed {rp['matrix_bytes']} bytes of matrices, dequantised {rd['matrix_bytes']}")


def test_logits_are_bit_equal(pair):
    d = pair["d"]
    toks = np.random.default_rng(3).integers(0, d.n_vocab, (2, 9)).astype(np.int64)
    toks[1, 4] = d.n_vocab - 1  # the embedding's last row
    feats = T.features(d, 2, 8)
    want = pair["deq"].logits(toks, feats).cpu().numpy()
    got = pair["packed"].logits(toks, feats).cpu().numpy()
    assert np.isfinite(want).all() and np.array_equal(got, want)
    one = pair["packed"].logits(toks[:, :1], feats).cpu().numpy()  # S = 1, the step's shape
    assert np.array_equal(one, pair["deq"].logits(toks[:, :1], feats).cpu().numpy())
    # and the self K/V the prefill wrote is the same: a step on top of it reads it back
    import torch

    for m in (pair["packed"], pair["deq"]):
        with torch.cuda.device(m.device):
            m._text.set_audio(torch.from_numpy(feats).to(m.device))
            m._text.forward(torch.from_numpy(toks[:, :8].astype(np.int32)).to(m.device), False)
    states = [m._text._state.cpu().numpy() for m in (pair["packed"], pair["deq"])]
    n_kv = 2 * (d.n_text_layer * 2 * d.n_audio_ctx * 2 * d.n_text_state + d.n_text_layer * 2 * d.n_text_ctx * 2 * d.n_text_state)  # cross then self, bf16
    a, b = (s[:n_kv].view(np.uint16).reshape(-1, 2 * d.n_text_state) for s in states)
    cross_rows = d.n_text_layer * 2 * d.n_audio_ctx
    assert np.array_equal(a[:cross_rows], b[:cross_rows])
    self_a, self_b = (x[cross_rows:].reshape(d.n_text_layer, 2, d.n_text_ctx, -1)[:, :, :8] for x in (a, b))
    assert np.array_equal(self_a, self_b) and self_a.any()


def _same(a, b):
    assert a.tokens == b.tokens and a.avg_logprob == b.avg_logprob and a.language == b.language and a.no_speech_prob == b.no_speech_prob, (a, b)


def test_decode_sample_and_beam_search_are_equal(pair):
    d, mp, md = pair["d"], pair["packed"], pair["deq"]
    feats = T.features(d, 2, 31)
    for got, want in zip(mp.decode(feats, sample_len=10), md.decode(feats, sample_len=10)):  # with language detection
        assert len(want.tokens) > 0
        _same(got, want)
    for got, want in zip(mp.beam_search(feats, language=4, sample_len=8, beam_size=2), md.beam_search(feats, language=4, sample_len=8, beam_size=2)):
        _same(got, want)
    kw = dict(language=4, sample_len=8, temperature=0.7, best_of=2, seed=0)
    for got, want in zip(mp.sample(feats, **kw), md.sample(feats, **kw)):
        _same(got, want)


def test_a_serve_round_and_find_alignment_are_equal(pair):
    d, mp, md = pair["d"], pair["packed"], pair["deq"]
    feats = T.features(d, 2, 13)
    opts = [dict(language=4, sample_len=6), dict(language=None, sample_len=9, without_timestamps=True, prompt=[1000, 1001])]
    results = []
    for m in (mp, md):
        with m.serve(max_rows=2, eos_check_interval=4) as s:  # the row-mode path: two windows in one running batch
            futs = [s.submit(feats[i], WD.DecodingOptions(**o)) for i, o in enumerate(opts)]
            s.run_until_idle()
            results.append([f.result(timeout=1) for f in futs])
    for got, want, o in zip(results[0], results[1], opts):
        assert 0 < len(want.tokens) <= o["sample_len"]
        _same(got, want)
    for got, solo in zip(results[0], (mp.decode(feats[i], WD.DecodingOptions(**o)) for i, o in enumerate(opts))):
        _same(got, solo)
    text = [int(t) for t in np.random.default_rng(2).integers(0, 50000, 12)]
    assert whisper.find_alignment(mp, text, feats[0], 146) == whisper.find_alignment(md, text, feats[0], 146)


def test_unpackable_formats_fall_back_matrix_by_matrix():
    """load_weights on tensors held by the caller: a 2-bit matrix, a matrix in groups of 16 and one in groups of 256 beside 4-bit ones.  Each is dequantised by
    the checkpoint's rule and named with its reason; the model still equals its dequantised twin bit for bit."""
    d, w = _float_weights()
    names = quant.whisper_quantised_layer_names(w, GROUP)
    odd = {"decoder.blocks.0.attn.query": {"group_size": 64, "bits": 2}, "decoder.blocks.0.mlp1": {"group_size": 16, "bits": 4},
           "decoder.blocks.1.mlp2": {"group_size": 256, "bits": 8}}
    q = quant.quantize_checkpoint(w, GROUP, 4, names=[k for k in names if k[: -len(".weight")] not in odd])
    for p, o in odd.items():
        q.update(quant.quantize_checkpoint({p + ".weight": w[p + ".weight"]}, o["group_size"], o["bits"], names=[p + ".weight"]))
    cfg = dict({"group_size": GROUP, "bits": 4}, **odd)
    mp = whisper.Model(d).load_weights(q, cfg)  # "packed" is load_weights' default
    md = whisper.Model(d).load_weights(q, cfg, "dequantized")
    fb = mp.weight_report()["fallbacks"]
    assert "bits" in fb["decoder.blocks.0.attn.query.weight"] and "group size" in fb["decoder.blocks.0.mlp1.weight"] and "group size" in fb["decoder.blocks.1.mlp2.weight"]
    for p, o in odd.items():
        assert quant.whisper_weight_route(p + ".weight", w[p + ".weight"].shape[1], o["group_size"], o["bits"]) == ("bf16", fb[p + ".weight"])  # one rule, stated twice
    assert len(fb) == 3 + 2 * d.n_text_layer and mp.weight_report()["bf16"] == 3 + d.n_text_layer
    toks = np.random.default_rng(4).integers(0, d.n_vocab, (1, 6)).astype(np.int64)
    feats = T.features(d, 1, 5)
    assert np.array_equal(mp.logits(toks, feats).cpu().numpy(), md.logits(toks, feats).cpu().numpy())
    plain = whisper.Model(d).load_weights(w, None, "packed")  # a checkpoint that is not quantised ignores the argument
    assert plain.weight_report()["packed"] == 0 and plain.weight_report()["fallbacks"] == {}
