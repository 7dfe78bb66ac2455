"""Whisper audio side, host half (mlx-audio_amd/whisper.py) and the CPU references of its GPU tests (tests/_whisper_ref.py), pinned against an
independent implementation: transformers' audio_utils and WhisperEncoder.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_ref as R  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402


# ---- the yardsticks themselves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_filter_bank_equals_transformers(n_mels):
    from transformers.audio_utils import mel_filter_bank

    want = mel_filter_bank(201, n_mels, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T
    got = whisper.mel_filters(n_mels)
    assert got.dtype == np.float64 and got.shape == (n_mels, 201)
    err = float(np.abs(got - want).max())
    print(f"n_mels {n_mels}: max |bank - transformers| = {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("n_mels,padding", [(80, 0), (128, 1600)])
def test_log_mel_restatement_equals_transformers(n_mels, padding):
    from transformers.audio_utils import spectrogram

    x = R.signal(32000, 11)
    xp = np.concatenate([x.astype(np.float64), np.zeros(padding)])
    spec = spectrogram(xp, R.hann_symmetric(), 400, 160, power=2.0, center=True, pad_mode="reflect", mel_filters=whisper.mel_filters(n_mels).T,
                       mel_floor=1e-10, log_mel="log10")
    lg = spec[:, :-1]  # drop the last frame
    lg = np.maximum(lg, lg.max() - 8.0)
    want = ((lg + 4.0) / 4.0).T
    got = R.log_mel(x, n_mels, padding)
    assert got.shape == ((32000 + padding) // 160, n_mels) == want.shape
    err = float(np.abs(got - want).max())
    print(f"n_mels {n_mels} padding {padding}: max |restatement - transformers| = {err:.2e}")
    assert err <= 1e-6


def test_positions_equal_transformers():
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder

    for ctx, D in ((100, 128), (1500, 384)):
        enc = WhisperEncoder(WhisperConfig(d_model=D, max_source_positions=ctx, encoder_layers=1, encoder_attention_heads=D // 64, decoder_layers=1,
                                           decoder_attention_heads=1, encoder_ffn_dim=8, decoder_ffn_dim=8))
        want = enc.embed_positions.weight.detach().numpy()
        err = float(np.abs(R.sinusoids(ctx, D) - want).max())
        print(f"sinusoids({ctx}, {D}): max error {err:.2e}")
        assert err <= 1e-6


def test_constants():
    assert (whisper.SAMPLE_RATE, whisper.N_FFT, whisper.HOP_LENGTH, whisper.CHUNK_LENGTH) == (16000, 400, 160, 30)
    assert (whisper.N_SAMPLES, whisper.N_FRAMES, whisper.N_SAMPLES_PER_TOKEN, whisper.FRAMES_PER_SECOND, whisper.TOKENS_PER_SECOND) == (480000, 3000, 320, 100, 50)


# ---- pad_or_trim --------------------------------------------------------------------------------------------------------------------------
def test_pad_or_trim_both_axes():
    import torch

    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(whisper.pad_or_trim(a, 2), a[:, :2])
    assert np.array_equal(whisper.pad_or_trim(a, 6), np.pad(a, ((0, 0), (0, 2))))
    assert np.array_equal(whisper.pad_or_trim(a, 2, axis=-2), a[:2])
    assert np.array_equal(whisper.pad_or_trim(a, 5, axis=0), np.pad(a, ((0, 2), (0, 0))))
    assert whisper.pad_or_trim(a, 4) is a
    t = torch.from_numpy(a)
    assert torch.equal(whisper.pad_or_trim(t, 5, axis=-2), torch.from_numpy(np.pad(a, ((0, 2), (0, 0)))))
    assert torch.equal(whisper.pad_or_trim(t, 3), t[:, :3])
    assert whisper.pad_or_trim(np.zeros(7, np.float32)).shape == (whisper.N_SAMPLES,)


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
D = R.dims(80, 100, 128, 2, 2)


def test_name_map_covers_the_encoder_and_passes_the_decoder_through():
    w = R.encoder_weights(D, 5)
    dec = {"decoder.token_embedding.weight": np.ones((4, 4), np.float16), "decoder.blocks.0.attn.key.weight": object(), "alignment_heads": b"x"}
    enc, rest = whisper.split_weights(D, {**w, **dec})
    assert set(enc) == set(whisper.encoder_shapes(D)) == set(w)
    assert all(v.dtype == np.float32 and v.shape == whisper.encoder_shapes(D)[k] for k, v in enc.items())
    assert all(np.array_equal(enc[k], w[k]) for k in w)
    assert set(rest) == set(dec) and all(rest[k] is dec[k] for k in dec)  # untouched: the very objects
    assert "encoder.blocks.0.attn.key.bias" not in enc and enc["encoder.blocks.1.mlp1.weight"].shape == (512, 128)


def test_both_conv_layouts_are_accepted():
    import torch

    a, _ = whisper.split_weights(D, R.encoder_weights(D, 5))
    b, _ = whisper.split_weights(D, R.encoder_weights(D, 5, torch_conv_layout=True))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c, _ = whisper.split_weights(D, {k: torch.from_numpy(v).half() for k, v in R.encoder_weights(D, 5).items()})  # fp16 tensors widen exactly
    assert all(np.array_equal(c[k], a[k].astype(np.float16).astype(np.float32)) for k in a)


@pytest.mark.parametrize("name", ["encoder.conv2.weight", "encoder.blocks.1.attn.key.weight", "encoder.ln_post.bias"])
def test_a_missing_or_misshapen_encoder_tensor_is_named(name):
    w = R.encoder_weights(D, 5)
    good = w.pop(name)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        whisper.split_weights(D, w)
    w[name] = np.zeros(tuple(s + 1 for s in good.shape), np.float32)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        whisper.split_weights(D, w)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
CONFIG = dict(n_mels=80, n_audio_ctx=100, n_audio_state=128, n_audio_head=2, n_audio_layer=2, n_vocab=51865, n_text_ctx=448, n_text_state=128,
              n_text_head=2, n_text_layer=1)


def test_quantised_checkpoint_is_refused(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(dict(CONFIG, quantization={"group_size": 64, "bits": 4})))
    with pytest.raises(ValueError, match="quantised Whisper checkpoints are not supported yet"):
        whisper.Model.from_pretrained(str(tmp_path))
    from mlx_audio_amd.utils import load_model

    with pytest.raises(ValueError, match="quantised Whisper checkpoints are not supported yet"):  # the ten dimensions route here
        load_model(tmp_path)
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "whisper"}))
    with pytest.raises(ValueError, match="lacks the Whisper dimensions"):  # model_type routes here too
        load_model(tmp_path)


def test_from_pretrained_never_leaves_the_disk(tmp_path):
    with pytest.raises(FileNotFoundError):
        whisper.Model.from_pretrained("mlx-community/whisper-tiny")
    (tmp_path / "config.json").write_text(json.dumps(CONFIG))
    with pytest.raises(FileNotFoundError, match="weights"):
        whisper.Model.from_pretrained(str(tmp_path))


def test_too_short_audio_is_a_value_error():
    with pytest.raises(ValueError, match="201"):
        whisper.log_mel_spectrogram(np.zeros(200, np.float32))
    with pytest.raises(ValueError, match="201"):
        whisper.log_mel_spectrogram([np.zeros(400, np.float32), np.zeros(100, np.float32)], padding=100)
    with pytest.raises(ValueError):
        whisper.log_mel_spectrogram(np.zeros(400, np.float32), n_mels=64)


def test_text_side_is_not_built():
    m = whisper.Model(whisper.dimensions_from_config(CONFIG))
    for call in (m.generate, m.decode, m.logits, m.detect_language):
        with pytest.raises(NotImplementedError, match="text decoder: not built"):
            call(np.zeros(16000, np.float32))
    assert m.is_multilingual and m.num_languages == 99
    assert not whisper.Model(R.dims(80, 100, 128, 2, 1).__class__(**dict(CONFIG, n_vocab=51864))).is_multilingual
    with pytest.raises(AssertionError, match="incorrect audio shape"):
        m.embed_audio(np.zeros((199, 80), np.float32))
    with pytest.raises(ValueError, match="bfloat16"):
        whisper.Model(whisper.dimensions_from_config(CONFIG), dtype="float16")
