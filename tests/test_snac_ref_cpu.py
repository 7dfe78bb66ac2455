"""Pins tests/_snac_ref.py (the float64 numpy restatement of the reference's SNAC port) independently of the device code: its convolutions
against torch.nn.functional in float64, from_codes against the quantiser, preprocess lengths, the Orpheus helpers, and the encode inputs of
tests/test_gpu_snac.py (a float32 restatement stays under the cap of excused coarse frames).  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import _snac_ref as R
from mlx_audio_amd import snac

T64 = lambda a: torch.tensor(np.asarray(a, np.float64))


def cfg_of(name):
    return snac.SNACConfig(**R.CONFIGS[name])


@pytest.mark.parametrize("stride,pad,dil,K", [(1, 0, 1, 1), (1, 3, 1, 7), (2, 1, 1, 4), (3, 2, 1, 6), (4, 2, 1, 8), (1, 6, 2, 7)])
def test_conv_matches_torch(stride, pad, dil, K):
    rng = np.random.default_rng(K * 10 + stride)
    x, w, b = rng.standard_normal((2, 23, 5)), rng.standard_normal((6, K, 5)), rng.standard_normal(6)
    got, s = R.conv(x, w, b, stride=stride, pad=pad, dil=dil, absum=True)
    ref = TF.conv1d(T64(x).permute(0, 2, 1), T64(w).permute(0, 2, 1), T64(b), stride=stride, padding=pad, dilation=dil).permute(0, 2, 1).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12
    assert np.all(s >= np.abs(got) - 1e-12)


@pytest.mark.parametrize("stride", [2, 3, 4, 7, 8])
def test_transposed_conv_matches_torch_and_has_the_ports_length(stride):
    rng = np.random.default_rng(stride)
    T, pad, K = 9, math.ceil(stride / 2), 2 * stride
    x, w, b = rng.standard_normal((2, T, 6)), rng.standard_normal((6, K, 4)), rng.standard_normal(4)
    got = R.conv_transposed(x, w, b, stride=stride, pad=pad)
    ref = TF.conv_transpose1d(T64(x).permute(0, 2, 1), T64(w).permute(0, 2, 1), T64(b), stride=stride, padding=pad).permute(0, 2, 1).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12
    # layers.py:105-121 never passes output_padding: T s rows for an even stride, T s - 1 for an odd one
    assert got.shape[1] == (T * stride if stride % 2 == 0 else T * stride - 1)


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("L", [1, 5, 30, 70])
def test_depthwise_conv_matches_torch(L, dil):
    rng = np.random.default_rng(L * 10 + dil)
    C = 6
    x, w, b = rng.standard_normal((2, L, C)), rng.standard_normal((C, 7, 1)), rng.standard_normal(C)
    a1, a2 = rng.uniform(0.5, 2, C), rng.uniform(0.5, 2, C)
    ref = TF.conv1d(T64(x).permute(0, 2, 1), T64(w).permute(0, 2, 1), T64(b), padding=3 * dil, dilation=dil, groups=C).permute(0, 2, 1).numpy()
    assert np.abs(R.dw_conv(x, w, b, dil=dil) - ref).max() <= 1e-12
    sn = lambda v, a: v + np.sin(a * v) ** 2 / (a + 1e-9)
    ref2 = TF.conv1d(T64(sn(x, a1)).permute(0, 2, 1), T64(w).permute(0, 2, 1), T64(b), padding=3 * dil, dilation=dil, groups=C).permute(0, 2, 1).numpy()
    assert np.abs(R.dw_conv(x, w, b, dil=dil, alpha_in=a1, alpha_out=a2) - sn(ref2, a2)).max() <= 1e-12


def test_last_conv_and_snake():
    rng = np.random.default_rng(3)
    x, w, b, a = rng.standard_normal((2, 11, 5)), rng.standard_normal((1, 7, 5)), rng.standard_normal(1), rng.uniform(0.5, 2, 5)
    sx = x + np.sin(a * x) ** 2 * (1.0 / (a + 1e-9))
    ref = torch.tanh(TF.conv1d(T64(sx).permute(0, 2, 1), T64(w).permute(0, 2, 1), T64(b), padding=3))[:, 0].numpy()
    assert np.abs(R.conv_cout1(x, w, b, pad=3, alpha=a, tanh=True) - ref).max() <= 1e-12
    assert np.abs(R.snake(x, a.reshape(1, 5, 1)) - sx).max() == 0.0


@pytest.mark.parametrize("name", ["even", "odd", "wide"])
def test_from_codes_equals_the_quantisers_z_q(name):
    cfg = cfg_of(name)
    W = R.Weights(R.synth_weights(snac.param_shapes(cfg), R.WEIGHT_SEED))
    T = 8
    z = np.random.default_rng(5).standard_normal((2, T, cfg.latent_dim))
    zq, codes, trace = R.quantizer(W, cfg, z)
    assert [c.shape for c in codes] == [(2, T // s) for s in cfg.vq_strides]
    # equal up to the rounding of z_e + (z_q - z_e) (vq.py:37): a few ulp of |z_e| + |z_q| through out_proj
    assert np.abs(R.from_codes(W, cfg, codes) - zq).max() <= 1e-12 * max(1.0, np.abs(zq).max())
    # the residual trace is what is left after each quantiser
    assert np.abs(trace[-1][1] - (z - zq)).max() <= 1e-12 * max(1.0, np.abs(z).max())


def test_vq_search_first_index_on_ties_and_the_eps_of_normalize():
    rng = np.random.default_rng(9)
    cb = rng.standard_normal((12, 8))
    cb[7] = cb[2]  # a duplicate row: index 2 wins
    ze = np.stack([cb[7] * 3.0, np.zeros(8), cb[5]])
    idx, dist = R.vq_search(ze, cb)
    assert idx[0] == 2 and idx[2] == 5 and np.isfinite(dist).all()
    assert 0 <= idx[1] < 12 and np.abs(dist[1] - 1.0).max() < 1e-12  # a zero row: e = 0 / eps = 0, every distance is |c|^2 = 1


def test_preprocess_lengths():
    for name, cases in (("even", [(1, 32), (32, 32), (33, 64), (601, 608)]), ("odd", [(1, 12), (12, 12), (13, 24)])):
        cfg = cfg_of(name)
        m = snac.SNAC(cfg)  # (no weights: host only)
        assert m.hop_length == int(np.prod(cfg.encoder_rates)) and m.n_codebooks == len(cfg.vq_strides) and m.vq_strides == cfg.vq_strides
        assert m.sampling_rate == 24000
        for n, want in cases:
            x = torch.ones(2, 1, n)
            y = m.preprocess(x)
            assert tuple(y.shape) == (2, 1, want) == (2, 1, R.preprocess_length(cfg, n))
            assert torch.equal(y[..., :n], x) and float(y[..., n:].abs().sum()) == 0.0
    m24 = snac.SNAC(snac.snac_24khz())
    assert m24.hop_length == 512 and m24.pad_to() == 2048 and m24.noise_channels == [512, 256, 128, 64]
    assert R.decode_length(snac.snac_24khz(), 32) == 32 * 512 and R.decode_length(cfg_of("odd"), 4) == (4 * 2) * 3 - 1


def test_orpheus_helpers_invert_each_other_and_match_the_slot_pattern():
    rng = np.random.default_rng(1)
    n = 5
    l1, l2, l3 = (rng.integers(0, 4096, (1, k * n)) for k in (1, 2, 4))
    flat = snac.codes_to_orpheus([l1, l2, l3])
    assert len(flat) == 7 * n
    for i in range(n):  # llama.py:61-70, literally
        assert flat[7 * i : 7 * i + 7] == [l1[0, i], l2[0, 2 * i] + 4096, l3[0, 4 * i] + 2 * 4096, l3[0, 4 * i + 1] + 3 * 4096,
                                          l2[0, 2 * i + 1] + 4 * 4096, l3[0, 4 * i + 2] + 5 * 4096, l3[0, 4 * i + 3] + 6 * 4096]
    back = snac.codes_from_orpheus(flat)
    assert [tuple(c.shape) for c in back] == [(1, n), (1, 2 * n), (1, 4 * n)] and all(c.dtype == torch.int32 for c in back)
    for got, want in zip(back, (l1, l2, l3)):
        assert np.array_equal(got.numpy(), want)
    assert snac.codes_to_orpheus(back) == flat
    with pytest.raises(ValueError):
        snac.codes_to_orpheus([l1, l2])
    with pytest.raises(ValueError):
        snac.codes_to_orpheus([l1, l2, l3[:, :-1]])


@pytest.mark.parametrize("case", sorted(R.ENCODE_CASES))
def test_encode_inputs_keep_a_float32_restatement_under_the_cap(case):
    """The inputs tests/test_gpu_snac.py encodes: torch float64 reproduces the numpy reference's codes exactly, and torch float32 differs
    from it on at most EXCUSED_CAP of the coarse frames, each time at a near-tie of the reference's own distances."""
    name, B, N, seed = R.ENCODE_CASES[case]
    cfg = cfg_of(name)
    w = R.synth_weights(snac.param_shapes(cfg), R.WEIGHT_SEED)
    x = R.audio(B, N, seed)
    codes, trace, z = R.encode(R.Weights(w), cfg, x)
    T = R.preprocess_length(cfg, N) // int(np.prod(cfg.encoder_rates))
    assert z.shape == (B, T, cfg.latent_dim) and [c.shape for c in codes] == [(B, T // s) for s in cfg.vq_strides]
    c64 = R.encode_torch(w, cfg, x, torch.float64)
    assert all(np.array_equal(a, b) for a, b in zip(c64, codes))
    excused, frames = R.excused_frames(R.encode_torch(w, cfg, x, torch.float32), codes, trace, cfg.vq_strides)
    assert excused <= R.EXCUSED_CAP * frames, (excused, frames)
    assert len({int(v) for c in codes for v in c.reshape(-1)}) > 8  # the search is not degenerate
