"""The FastConformer encoder on the device (parakeet.Model.encode, kk_parakeet_*, csrc/kk_parakeet.hip) against the restatement module of
tests/_parakeet_ref.py on the CPU.  Bar, as in test_gpu_whisper_encoder.py: the relative rms error against the module in fp32 is at most 1.5 x that of
the module's own .bfloat16() run; both are printed.  Config a: 80 features, factor 8 (three stages), heads of 64, k = 9, biases; config b: 128 features,
factor 4, heads of 128, k = 31, no biases, xscaling.  BatchNorm statistics are non-trivial.  One case starts from samples."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _parakeet_ref as R  # noqa: E402

from mlx_audio_amd import parakeet, utils  # noqa: E402

pytestmark = pytest.mark.gpu
BASE = dict(self_attention_model="rel_pos", subsampling="dw_striding", pos_emb_max_len=5000, ff_expansion_factor=4)
CONFIGS = {
    "a": (dict(BASE, feat_in=80, d_model=128, n_heads=2, n_layers=2, subsampling_factor=8, subsampling_conv_channels=128, conv_kernel_size=9, use_bias=True,
               xscaling=False), 203, 26),
    "b": (dict(BASE, feat_in=128, d_model=256, n_heads=2, n_layers=1, subsampling_factor=4, subsampling_conv_channels=256, conv_kernel_size=31, use_bias=False,
               xscaling=True), 530, 133),
}
_made = {}


def _case(name):
    """(config, module, mel, fp32 reference, the module's bf16 error), made once"""
    if name not in _made:
        enc, T_mel, T = CONFIGS[name]
        ref = R.Encoder(enc, seed=len(name) + T)
        mel = torch.randn((2, T_mel, enc["feat_in"]), generator=torch.Generator().manual_seed(T_mel))
        want = ref(mel)
        assert want.shape == (2, T, enc["d_model"])
        import copy

        e16 = rel_rms(copy.deepcopy(ref).bfloat16()(mel), want)
        pre = dict(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=enc["feat_in"], n_fft=512, dither=1e-5)
        _made[name] = (dict(encoder=enc, preprocessor=pre), ref, mel, want, e16)
    return _made[name]


def rel_rms(got, ref):
    return float(torch.sqrt(((got.double() - ref.double()) ** 2).mean() / (ref.double() ** 2).mean()))


@pytest.mark.parametrize("name", ["a", "b"])
def test_against_the_module(name):
    cfg, ref, mel, want, e16 = _case(name)
    model = parakeet.Model(cfg).load_weights(ref.weights())
    got, lengths = model.encode(mel)
    err = rel_rms(got.cpu(), want)
    print(f"config {name}: device {err:.3e}, the module in bf16 {e16:.3e}")
    assert list(lengths) == [want.shape[1]] * 2
    assert err <= 1.5 * e16
    alone, _ = model.encode(mel[1])  # an item's bits do not depend on the batch
    assert torch.equal(alone[0], got[1])


def test_from_samples():
    """encode_audio = the module on the float64 restatement of the features: the same bar, the features' own error being far below it"""
    import copy

    cfg, ref, _, _, _ = _case("a")
    x = R.signal(16007, 5)
    mel = torch.from_numpy(R.log_mel(x, 16000, 512, 400, 160, 80, True)).float()[None]
    want = ref(mel)
    e16 = rel_rms(copy.deepcopy(ref).bfloat16()(mel), want)
    got, lengths = parakeet.Model(cfg).load_weights(ref.weights()).encode_audio(x)
    err = rel_rms(got.cpu(), want)
    print(f"from samples: device {err:.3e}, the module in bf16 {e16:.3e}")
    assert list(lengths) == [want.shape[1]] and err <= 1.5 * e16


def test_from_pretrained_round_trip(tmp_path):
    from safetensors.numpy import save_file

    cfg, ref, mel, want, e16 = _case("a")
    w = dict(ref.weights(), **{"decoder.prediction.embed.weight": np.zeros((4, 8), np.float32)})
    save_file(w, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    model = utils.load_model(str(tmp_path))
    assert isinstance(model, parakeet.Model) and list(model.text_side_weights) == ["decoder.prediction.embed.weight"]
    assert torch.equal(model.encode(mel)[0], parakeet.Model(cfg).load_weights(ref.weights()).encode(mel)[0])
    with pytest.raises(NotImplementedError, match="text side"):
        model.generate(mel)
    with pytest.raises(NotImplementedError, match="cache"):
        model.encode(mel, cache=[None])
