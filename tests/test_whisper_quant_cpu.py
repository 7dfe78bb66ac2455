"""Quantised Whisper checkpoints without a device (mlx-audio_amd/whisper.py, quant.py): the refusal that stays the default, the set of layers a
checkpoint quantises, the round trip of the triplets with per-layer entries, the bit widths that are refused and the routing of a matrix to packed or
bf16 storage."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_ref as R  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import quant, whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402


def _config(d, **extra):
    return dict({k: int(getattr(d, k)) for k in whisper.DIMENSION_KEYS}, **extra)


def _small():
    """a decoder small enough to quantise in a blink: SHAPE_A's blocks behind a 512-token vocabulary"""
    d = T.dims(128, 2, 2, 512, 100)
    return d, {**R.encoder_weights(d, 5), **T.decoder_weights(d, 3)}


def test_the_default_refuses_and_names_weight_storage(tmp_path):
    d = T.dims(**T.SHAPE_A)
    (tmp_path / "config.json").write_text(json.dumps(_config(d, quantization={"group_size": 64, "bits": 4})))
    with pytest.raises(ValueError, match="quantised Whisper checkpoints are not supported yet.*weight_storage"):
        whisper.Model.from_pretrained(str(tmp_path))
    with pytest.raises(ValueError, match="quantised Whisper checkpoints are not supported yet"):
        whisper.load_model(tmp_path)
    from mlx_audio_amd.utils import load_model

    with pytest.raises(ValueError, match="quantised Whisper checkpoints are not supported yet"):
        load_model(tmp_path)
    for call in (lambda: whisper.Model.from_pretrained(str(tmp_path), weight_storage="bogus"), lambda: whisper.load_model(tmp_path, weight_storage="bogus"),
                 lambda: load_model(tmp_path, weight_storage="bogus"), lambda: whisper.Model(d).load_weights({}, {"group_size": 64, "bits": 4}, "bogus")):
        with pytest.raises(ValueError, match="weight_storage must be 'packed' or 'dequantized'"):
            call()
    assert whisper.dimensions_from_config(_config(d, quantization={"group_size": 64, "bits": 4}), "packed") == d  # with a storage the dimensions are read


def test_quantised_layer_names_are_the_linears_and_the_embedding():
    d = T.dims(**T.SHAPE_A)
    shapes = {**whisper.encoder_shapes(d), **WD.decoder_shapes(d), "encoder._positional_embedding": (d.n_audio_ctx, d.n_audio_state)}
    w = {k: np.zeros(s, np.float32) for k, s in shapes.items()}
    want = {"decoder.token_embedding.weight"}
    for i in range(d.n_audio_layer):
        want |= {f"encoder.blocks.{i}.{n}.weight" for n in ("attn.query", "attn.key", "attn.value", "attn.out", "mlp1", "mlp2")}
    for i in range(d.n_text_layer):
        want |= {f"decoder.blocks.{i}.{a}.{n}.weight" for a in ("attn", "cross_attn") for n in ("query", "key", "value", "out")}
        want |= {f"decoder.blocks.{i}.{n}.weight" for n in ("mlp1", "mlp2")}
    got = quant.whisper_quantised_layer_names(w, 64)
    assert len(got) == len(set(got)) and set(got) == want
    assert not any("conv" in k or "ln" in k or "positional" in k for k in got)
    assert "decoder.blocks.0.mlp2.weight" in quant.whisper_quantised_layer_names(w, 128)
    assert quant.whisper_quantised_layer_names({"decoder.blocks.0.mlp1.weight": np.zeros((8, 96), np.float32)}, 64) == []  # 96 is no multiple of the group


def test_split_triplets_round_trips_a_fixture_with_per_layer_entries():
    d, w = _small()
    names = quant.whisper_quantised_layer_names(w, 64)
    eight, plain_name = "decoder.blocks.0.mlp1", "decoder.blocks.1.attn.out"
    names4 = [k for k in names if k not in (eight + ".weight", plain_name + ".weight")]
    q = quant.quantize_checkpoint(w, 64, 4, names=names4)
    q.update({k: v for k, v in quant.quantize_checkpoint({eight + ".weight": w[eight + ".weight"]}, 64, 8, names=[eight + ".weight"]).items()})
    per_layer = {eight: {"group_size": 64, "bits": 8}, plain_name: False}
    plain, trip = quant.split_triplets(q, 64, 4, per_layer)
    assert set(trip) == set(names4) | {eight + ".weight"} and plain_name + ".weight" in plain
    assert not any(k.endswith(".scales") or k.endswith(".biases") for k in plain)
    assert trip[eight + ".weight"][3:] == (64, 8) and trip["decoder.token_embedding.weight"][3:] == (64, 4)
    for k, (words, scales, biases, g, bits) in trip.items():
        assert words.dtype == np.uint32 and words.shape == (w[k].shape[0], w[k].shape[1] * bits // 32) and scales.shape == (w[k].shape[0], w[k].shape[1] // g)
        back = quant.dequantize_affine(words, scales, biases, g, bits)
        step = np.repeat(scales, g, axis=1)
        assert (np.abs(back - w[k]) <= 0.5 * step * (1 + 1e-5) + 1e-7).all()  # a value moves by at most half a quantisation step
    assert np.array_equal(plain[plain_name + ".weight"], w[plain_name + ".weight"])
    # whisper.split_quantised: "dequantized" leaves nothing packed; "packed" hands on the decoder's triplets and dequantises the encoder's
    cfg = dict({"group_size": 64, "bits": 4}, **per_layer)
    flat, none = whisper.split_quantised(q, cfg, "dequantized")
    assert none == {} and set(flat) == set(w)
    rest, packed = whisper.split_quantised(q, cfg, "packed")
    assert set(packed) == {k for k in trip if k.startswith("decoder.")} and all(k in rest for k in trip if k.startswith("encoder."))
    for k in trip:
        if k.startswith("encoder."):
            assert np.array_equal(rest[k], flat[k]) and rest[k].dtype == np.float32
    assert WD.decoder_tensors(d, rest, packed) is not None and WD.decoder_tensors(d, rest) is None
    bad = dict(packed)
    k = "decoder.blocks.0.attn.query.weight"
    bad[k] = (packed[k][0][:, :-1],) + packed[k][1:]
    with pytest.raises(ValueError, match=k):
        WD.decoder_tensors(d, rest, bad)


def test_three_bits_are_refused_with_check_bits_message():
    d, w = _small()
    q = quant.quantize_checkpoint(w, 64, 4, names=["decoder.blocks.0.mlp1.weight"])
    for cfg in ({"group_size": 64, "bits": 3}, {"group_size": 64, "bits": 4, "decoder.blocks.0.mlp1": {"bits": 6}}):
        with pytest.raises(ValueError, match="only 2, 4 and 8 bits fit the word layout"):
            whisper.split_quantised(q, cfg, "packed")
    with pytest.raises(ValueError, match="only 2, 4 and 8 bits fit the word layout"):
        quant.whisper_weight_route("decoder.blocks.0.mlp1.weight", 128, 64, 3)


def test_routing_to_packed_or_bf16():
    route = quant.whisper_weight_route
    name = "decoder.blocks.1.mlp2.weight"
    for bits in (4, 8):
        for group in (32, 64, 128):
            assert route(name, 512, group, bits) == ("packed", None)
            assert route("decoder.token_embedding.weight", 128, group, bits) == ("packed", None)
    kind, why = route(name, 512, 64, 2)
    assert kind == "bf16" and "bits" in why
    kind, why = route(name, 512, 16, 4)
    assert kind == "bf16" and "group size" in why
    kind, why = route(name, 512, 256, 8)
    assert kind == "bf16" and "group size" in why
    kind, why = route(name, 96, 64, 4)  # K is not a multiple of the group
    assert kind == "bf16" and "multiple of the group" in why
    assert route(name, 32, 64, 4)[0] == "bf16"
    for part in ("key", "value"):
        kind, why = route(f"decoder.blocks.0.cross_attn.{part}.weight", 128, 64, 4)
        assert kind == "bf16" and "cross key | value" in why
    assert route("decoder.blocks.0.cross_attn.query.weight", 128, 64, 4) == ("packed", None)
    kind, why = route("encoder.blocks.0.mlp1.weight", 128, 64, 4)
    assert kind == "bf16" and "encoder" in why
