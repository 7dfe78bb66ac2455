"""The Whisper audio encoder on the device (whisper.Model.embed_audio -> kk_whisper_encode, csrc/kk_whisper.hip) against
transformers' WhisperEncoder in fp32 on the CPU with the same (bf16-exact) weights.

The bar (3c): the relative rms error of embed_audio against that fp32 run may be 1.5 x the relative rms error of the same torch module
converted with .bfloat16() and run on the CPU -- an independent bf16 execution of the reference, which rounds at other places, hence the 1.5.
Both figures are computed and printed every run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _whisper_ref as R  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"a": (80, 100, 128, 2, 2), "b": (128, 1500, 384, 6, 1)}
SEEDS = {"a": 31, "b": 32}
_cache = {}


def _case(key, ctx=None):
    """-> (dims, device model, fp32 CPU reference module), built once per shape"""
    if (key, ctx) not in _cache:
        n_mels, c, width, heads, layers = SHAPES[key]
        d = R.dims(n_mels, ctx or c, width, heads, layers)
        w = R.encoder_weights(d, SEEDS[key])
        _cache[(key, ctx)] = (d, whisper.Model(d).load_weights(w), R.hf_encoder(d, w))
    return _cache[(key, ctx)]


def _mel(d, B, seed):
    return (0.5 * np.random.default_rng(seed).standard_normal((B, 2 * d.n_audio_ctx, d.n_mels))).astype(np.float32)


@pytest.mark.parametrize("key", ["a", "b"])
def test_embed_audio_against_the_fp32_reference(key):
    d, model, enc = _case(key)
    mel = _mel(d, 2, 7)
    ref = R.hf_encode(enc, mel)
    got = model.embed_audio(mel)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, d.n_audio_ctx, d.n_audio_state)
    got = got.cpu().numpy()
    assert not np.isnan(got).any()
    ours, theirs = R.rel_rms(got, ref), R.rel_rms(R.hf_encode(enc, mel, bf16=True), ref)
    print(f"shape ({key}): relative rms error {ours:.5f}; the CPU bf16 run of the reference {theirs:.5f}; bar {1.5 * theirs:.5f}; output rms "
          f"{float(np.sqrt((ref ** 2).mean())):.3f}")
    assert ours <= 1.5 * theirs
    one = model.embed_audio(mel[0])  # the 2-D form
    assert tuple(one.shape) == (d.n_audio_ctx, d.n_audio_state)


def test_an_items_bits_do_not_depend_on_the_batch():
    d, model, _ = _case("a")
    mel = _mel(d, 3, 9)
    all3 = model.embed_audio(mel).clone()
    one = model.embed_audio(mel[1:2])
    assert torch.equal(all3[1], one[0])


def test_end_to_end_from_samples():
    d, model, enc = _case("a", ctx=1500)
    x = (0.1 * np.random.default_rng(3).standard_normal(16000)).astype(np.float32)
    mel = whisper.pad_or_trim(whisper.log_mel_spectrogram(x, 80, padding=whisper.N_SAMPLES), whisper.N_FRAMES, axis=-2)
    assert tuple(mel.shape) == (3000, 80)
    got = model.embed_audio(mel).cpu().numpy()
    mel_ref = R.log_mel(x, 80, whisper.N_SAMPLES)[: whisper.N_FRAMES].astype(np.float32)[None]
    ref = R.hf_encode(enc, mel_ref)
    ours, theirs = R.rel_rms(got, ref[0]), R.rel_rms(R.hf_encode(enc, mel_ref, bf16=True), ref)
    print(f"end to end: relative rms error {ours:.5f}; the CPU bf16 run of the reference {theirs:.5f}; bar {1.5 * theirs:.5f}")
    assert not np.isnan(got).any() and ours <= 1.5 * theirs


def test_the_wrong_mel_length_raises_the_references_assertion():
    d, model, _ = _case("a")
    with pytest.raises(AssertionError, match="incorrect audio shape"):
        model.embed_audio(np.zeros((2, 2 * d.n_audio_ctx - 2, d.n_mels), np.float32))
    with pytest.raises(AssertionError, match="incorrect audio shape"):
        model.embed_audio(np.zeros((2 * d.n_audio_ctx, d.n_mels + 1), np.float32))


@pytest.mark.parametrize("kind", ["safetensors", "npz"])
def test_a_checkpoint_directory_loads_through_load_model(tmp_path, kind):
    import dataclasses
    import json

    from mlx_audio_amd.utils import load_model

    d, model, _ = _case("a")
    w = R.encoder_weights(d, SEEDS["a"], torch_conv_layout=(kind == "safetensors"))  # the weights of _case("a")
    w["decoder.token_embedding.weight"] = np.ones((4, 128), np.float32)
    (tmp_path / "config.json").write_text(json.dumps(dict(dataclasses.asdict(d), model_type="whisper")))
    if kind == "safetensors":
        from safetensors.torch import save_file

        save_file({k: torch.from_numpy(v).bfloat16() for k, v in w.items()}, str(tmp_path / "weights.safetensors"))
    else:
        np.savez(str(tmp_path / "weights.npz"), **{k: v.astype(np.float16) for k, v in w.items()})
    loaded = load_model(tmp_path)
    assert isinstance(loaded, whisper.Model) and loaded.dims == d and set(loaded.decoder_weights) == {"decoder.token_embedding.weight"}
    mel = _mel(d, 1, 13)
    if kind == "safetensors":  # bf16-exact weights in another container and conv layout: the same bits
        assert torch.equal(loaded.embed_audio(mel), model.embed_audio(mel))
    else:  # fp16 storage rounds the weights: close, not equal
        assert R.rel_rms(loaded.embed_audio(mel).cpu().numpy(), model.embed_audio(mel).cpu().numpy()) < 0.01
