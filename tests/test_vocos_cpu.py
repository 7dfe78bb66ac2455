"""Host surface of the Vocos vocoder (mlx-audio_amd/vocos.py, kk_vocos_* of include/kokoro_hip.h), no GPU: the parameter names `load_weights` consumes and
how a PyTorch checkpoint reaches them, the config round trip, what is refused, and the reference restatement's iSTFT against a direct inverse DFT."""
import dataclasses

import numpy as np
import pytest
import torch
import yaml

import _vocos_ref as R
from mlx_audio_amd import vocos


@pytest.mark.parametrize("preset", [vocos.vocos_mel_24khz, vocos.vocos_encodec_24khz])
@pytest.mark.parametrize("embedding_layout", [False, True])
def test_sanitize_of_a_pytorch_state_dict_gives_param_shapes(preset, embedding_layout):
    cfg = preset()
    want = vocos.param_shapes(cfg)
    w = {k: np.random.default_rng(0).standard_normal(s).astype(np.float32) for k, s in want.items()}
    pt = {k: np.moveaxis(v, 1, 2) if v.ndim == 3 else v for k, v in w.items()}  # Conv1d weights [O][I / groups][K]
    if embedding_layout:  # AdaLayerNorm as two nn.Embedding: [num_embeddings][dim], no bias
        pt = {k: v.T if k.endswith((".scale.weight", ".shift.weight")) else v for k, v in pt.items() if not k.endswith((".scale.bias", ".shift.bias"))}
    pt.update({"head.istft.window": np.zeros(cfg.n_fft), "feature_extractor.mel_spec.spectrogram.window": np.zeros(cfg.n_fft), "feature_extractor.encodec.x": np.zeros(3)})
    back = vocos.sanitize(cfg, pt)
    assert {k: v.shape for k, v in back.items()} == {k: tuple(s) for k, s in want.items()}
    assert all(np.array_equal(back[k], w[k]) or (embedding_layout and k.endswith(".bias") and not back[k].any()) for k in w)
    assert ("backbone.norm.scale.weight" in want) == bool(cfg.adanorm_num_embeddings) and want["backbone.convnext.7.dwconv.weight"] == (cfg.dim, 7, 1)


@pytest.mark.parametrize("preset", [vocos.vocos_mel_24khz, vocos.vocos_encodec_24khz])
def test_from_yaml_reproduces_the_preset(preset, tmp_path):
    d = dict(preset().to_dict(), feature_extractor={"class_path": "vocos.feature_extractors.MelSpectrogramFeatures", "init_args": {"n_fft": 1024}})
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(d))
    assert dataclasses.asdict(vocos.VocosConfig.from_yaml(tmp_path / "config.yaml")) == dataclasses.asdict(preset())


def _model(**kw):
    m = vocos.Vocos(vocos.VocosConfig(**dict(R.TINY_ADA, **kw)))  # no weights, no GPU needed
    m._final = True
    return m


REFUSALS = {
    "n_fft 768": (NotImplementedError, "n_fft=768", lambda: vocos.Vocos(vocos.VocosConfig(**dict(R.TINY, n_fft=768, hop_length=192)))),
    "hop": (NotImplementedError, "hop_length=100", lambda: vocos.istft_head(torch.zeros(1, 4, 258), 256, 100)),
    "T 1": (ValueError, "T=1", lambda: vocos.istft_head(torch.zeros(1, 1, 258), 256, 64)),
    "T 1 decode": (ValueError, "T=1", lambda: _model().decode(np.zeros((1, 1, 24), np.float32), bandwidth_id=[[3.0, 3, 3, 3]])),
    "padding": (NotImplementedError, "padding", lambda: vocos.param_shapes(vocos.VocosConfig(**dict(R.TINY, padding="same")))),
    "C kernel": (NotImplementedError, "C=1025", lambda: vocos.dwconv_layernorm(torch.zeros(1, 2, 1025), np.zeros((1025, 7, 1)), np.zeros(1025), None, None)),
    "C model": (NotImplementedError, "dim=0", lambda: vocos.Vocos(vocos.VocosConfig(**dict(R.TINY, dim=0)))),
    "bandwidth_id": (ValueError, "bandwidth_id", lambda: _model().decode(np.zeros((1, 5, 24), np.float32))),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_are_made_on_the_host(case):
    exc, match, call = REFUSALS[case]
    with pytest.raises(exc, match=match):
        call()


def test_reference_istft_is_the_direct_inverse_dft():
    N, H, T = 256, 64, 5
    h = np.random.default_rng(3).standard_normal((2, T, N + 2)) * np.r_[np.full(N // 2 + 1, 2.5), np.full(N // 2 + 1, 4.0)]
    got, clipped = R.istft_head(h, N, H)
    k, n = np.arange(N // 2 + 1)[:, None], np.arange(N)[None]
    wk = np.where((k == 0) | (k == N // 2), 1.0, 2.0)  # the Hermitian half counted twice, bins 0 and N / 2 once and real
    mag, p = np.minimum(np.exp(h[..., : N // 2 + 1]), 100.0), h[..., N // 2 + 1 :]
    ph = p[..., None] + 2 * np.pi * k * n / N
    frames = (mag[..., None] * wk * np.where((k == 0) | (k == N // 2), np.cos(p)[..., None] * np.cos(2 * np.pi * k * n / N), np.cos(ph))).sum(-2) / N
    w = 0.5 * (1 - np.cos(2 * np.pi * np.arange(N) / (N - 1)))
    y, ws = np.zeros((2, (T - 1) * H + N)), np.zeros((T - 1) * H + N)
    for f in range(T):
        y[:, f * H : f * H + N] += frames[:, f] * w
        ws[f * H : f * H + N] += w
    want = (y / np.where(ws != 0, ws, 1.0))[:, N // 2 : -(N // 2)]
    assert got.shape == (2, (T - 1) * H) and np.abs(got - want).max() <= 1e-12 and 0.01 <= clipped <= 0.10
