"""Host surface of the BigVGAN vocoder (mlx-audio_amd/bigvgan.py, kk_bigvgan_* of include/kokoro_hip.h), no GPU: the filter taps, the index
formula the kernel implements, what is refused, and the parameter names `load_weights` consumes."""
import dataclasses

import numpy as np
import pytest

import _bigvgan_ref as R
from mlx_audio_amd import bigvgan

cfg_of = lambda **kw: bigvgan.BigVGANConfig(**dict(R.TINY, **kw))


def test_host_made_taps_equal_the_reference_formula():
    taps = bigvgan.filter_taps()
    assert taps.shape == (12,) and np.abs(taps - R.kaiser_sinc()).max() <= 6e-8 and np.array_equal(taps, taps[::-1])  # (float32 rounding of taps < 0.5)


def clamped_formula(x, alpha, beta, logscale):
    """what kk_op_bigvgan_amp_act computes (include/kokoro_hip.h), x [B][L][C]"""
    f, L = R.kaiser_sinc(), x.shape[1]
    a, b = (np.exp(v) if logscale else v for v in (alpha, beta))
    xc = lambda i: x[:, np.clip(i, 0, L - 1)]
    u = np.empty((x.shape[0], 2 * L, x.shape[2]))
    t = np.arange(L)
    u[:, 0::2] = 2 * sum(f[5 - 2 * d] * xc(t + d) for d in range(-3, 3))
    u[:, 1::2] = 2 * sum(f[6 - 2 * d] * xc(t + d) for d in range(-2, 4))
    s = u + np.sin(a * u) ** 2 / (b + 1e-9)
    return sum(f[k] * s[:, np.clip(2 * t - 5 + k, 0, 2 * L - 1)] for k in range(12))


@pytest.mark.parametrize("L", [1, 2, 5, 13])
def test_clamped_index_formula_is_the_padded_formulation(L):
    rng = np.random.default_rng(L)
    x, alpha, beta = rng.standard_normal((2, L, 3)), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    assert np.abs(clamped_formula(x, alpha, beta, True) - R.activation1d(x, alpha, beta, True)).max() <= 1e-12


def test_refusals_name_the_field():
    with pytest.raises(NotImplementedError, match="snake.*TIME axis"):
        bigvgan.BigVGAN(cfg_of(activation="snake"))
    with pytest.raises(NotImplementedError, match="resblock"):
        bigvgan.param_shapes(cfg_of(resblock="3"))
    with pytest.raises(ValueError, match="compute_dtype"):
        bigvgan.BigVGAN(cfg_of(), compute_dtype="float16")
    m = bigvgan.BigVGAN(cfg_of())  # no weights, no GPU needed
    m._final = True
    with pytest.raises(NotImplementedError, match="lengths"):
        m(np.zeros((2, 8, 4), np.float32), lengths=[4, 2])
    with pytest.raises(NotImplementedError, match="lengths"):
        m([np.zeros((8, 4), np.float32), np.zeros((8, 3), np.float32)])
    bad = dict(R.synth_weights(bigvgan.param_shapes(cfg_of())))
    bad["activation_post.upsample.filter"] = np.full((1, 12, 1), 1 / 12, np.float32)  # some other Activation1d
    with pytest.raises(ValueError, match="activation_post.upsample.filter"):
        bigvgan.BigVGAN(cfg_of()).load_weights(bad)
    with pytest.raises(bigvgan.KokoroHipError, match="length"):  # an even kernel: the residual add of amp.py would not broadcast
        bigvgan.BigVGAN(cfg_of(resblock_kernel_sizes=[4, 7, 11]))


@pytest.mark.parametrize("resblock", ["1", "2"])
def test_param_shapes_are_the_reference_parameter_names(resblock):
    cfg = cfg_of(resblock=resblock, use_bias_at_final=False)
    names = bigvgan.param_shapes(cfg)
    per_act = 4  # alpha, beta, upsample.filter, downsample.lowpass.filter
    convs = 2 if resblock == "1" else 1
    assert len(names) == 3 + 2 * (3 + 3 * 3 * convs * (3 + per_act)) + per_act + 2
    assert names["ups.1.0.weight_v"] == (16, 4, 32) and names["ups.1.0.weight_g"] == (1, 1, 32) and names["conv_pre.weight_v"] == (64, 7, 8)
    assert names["resblocks.5.activations.2.act.beta"] == (16,) and names["resblocks.0.activations.0.downsample.lowpass.filter"] == (1, 12, 1)
    assert ("resblocks.3.convs2.2.bias" in names) == (resblock == "1") and ("resblocks.3.convs.2.bias" in names) == (resblock == "2")
    assert names["conv_post.weight_v"] == (1, 7, 16) and "conv_post.bias" not in names and "conv_post.bias" in bigvgan.param_shapes(cfg_of())
    # PyTorch layouts come back to these shapes through sanitize (bigvgan.py:124-149)
    w = R.synth_weights(names)
    pt = {k: (v.transpose(2, 0, 1) if k.startswith("ups.") and v.ndim == 3 else v.transpose(0, 2, 1) if v.ndim == 3 else v) for k, v in w.items()}
    back = bigvgan.sanitize(cfg, dict(pt, **{"bn.num_batches_tracked": np.zeros(1)}))
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    assert dataclasses.asdict(bigvgan.BigVGANConfig.from_dict(dict(dataclasses.asdict(cfg), extra=1))) == dataclasses.asdict(cfg)
