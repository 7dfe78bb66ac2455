"""The host surface of the Parakeet kernels (mlx-audio_amd/parakeet.py, csrc/kk_parakeet.hip) without a GPU: the ABI, the entry points' refusals
(all made before anything is launched) and the float64 host tables against the restatements of tests/_parakeet_ref.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _parakeet_ref as R  # noqa: E402

from mlx_audio_amd import _lib, parakeet  # noqa: E402

P = C.c_void_p(4096)  # an aligned pointer that is never followed: every call below is refused first


def test_abi_minor_and_signatures():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kokoro_hip.h")).read()
    assert lib.kk_abi_minor() >= 31 and int(re.search(r"#define KK_ABI_MINOR (\d+)", hdr).group(1)) == lib.kk_abi_minor()
    for name in ("kk_op_rel_pos_attention", "kk_op_conformer_dwconv", "kk_op_conv2d_s2", "kk_op_parakeet_log_mel", "kk_parakeet_create", "kk_parakeet_destroy",
                 "kk_parakeet_load_tensor", "kk_parakeet_finalize", "kk_parakeet_encode_frames", "kk_parakeet_encode_workspace_bytes", "kk_parakeet_encode"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, hdr)


@pytest.mark.parametrize("call,message", [
    (lambda lib: lib.kk_op_rel_pos_attention(None, 1, P, 288, 4, 4, 1, 96, P, 96, P, P, P, 96), "head_dim = 96"),
    (lambda lib: lib.kk_op_rel_pos_attention(None, 1, P, 192, 4, 5, 1, 64, P, 64, P, P, P, 64), "T <= T_rows"),
    (lambda lib: lib.kk_op_rel_pos_attention(None, 1, P, 184, 4, 4, 1, 64, P, 64, P, P, P, 64), "ld is smaller"),
    (lambda lib: lib.kk_op_rel_pos_attention(None, 1, P, 192, 4, 4, 1, 64, None, 64, P, P, P, 64), "null argument"),
    (lambda lib: lib.kk_op_conformer_dwconv(None, 1, P, 16, 4, 8, 8, P, P, P, 8), "k = 8 must be odd"),
    (lambda lib: lib.kk_op_conformer_dwconv(None, 1, P, 16, 4, 8, 33, P, P, P, 8), "k = 33 must be odd and <= 31"),
    (lambda lib: lib.kk_op_conformer_dwconv(None, 1, P, 14, 4, 8, 9, P, P, P, 8), "ld >= 2 D"),
    (lambda lib: lib.kk_op_conv2d_s2(None, 1, P, 0, 4, 4, 7, P, P, P), "even C"),
    (lambda lib: lib.kk_op_parakeet_log_mel(None, 1, P, 200, 200, 0, 0.0, 512, 160, 400, 80, 1, P, P, P, P), "too few for the reflect padding"),
    (lambda lib: lib.kk_op_parakeet_log_mel(None, 1, P, 4000, 4000, 0, 0.0, 1024, 160, 400, 80, 1, P, P, P, P), "n_fft = 1024"),
])
def test_refusals(call, message):
    lib = _lib.load()
    assert call(lib) != 0
    assert message in lib.kk_last_error().decode()


def test_host_tables():
    for n in (1, 2, 7, 8, 203, 530, 3001):
        for factor in (2, 4, 8):
            assert parakeet.subsampled_lengths([n], factor)[0] == R.subsampled_lengths([n], factor)[0]
    assert parakeet.subsampled_lengths([203], 8)[0] == 26 and parakeet.subsampled_lengths([530], 4)[0] == 133
    for T in (1, 26, 133):
        assert np.array_equal(parakeet.rel_positions(T, 128), R.rel_positions(T, 128))
    g = np.random.default_rng(3)
    dw_w, dw_b, bn = g.standard_normal((6, 9, 1)), g.standard_normal(6), [g.standard_normal(6), g.standard_normal(6), g.standard_normal(6), g.uniform(0.5, 2, 6)]
    w, b = parakeet.fold_batch_norm(dw_w, dw_b, *bn)
    y = g.standard_normal((9, 6))  # one window per channel: conv, then BatchNorm
    want = ((y * dw_w[:, :, 0].T).sum(0) + dw_b - bn[2]) / np.sqrt(bn[3] + 1e-5) * bn[0] + bn[1]
    assert w.shape == (9, 6) and np.allclose((y * w).sum(0) + b, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("field,value", [("subsampling", "striding"), ("causal_downsampling", True), ("self_attention_model", "abs_pos")])
def test_config_refusals_name_the_field(field, value):
    enc = dict(feat_in=80, n_layers=1, d_model=128, n_heads=2, ff_expansion_factor=4, subsampling_factor=8, conv_kernel_size=9, subsampling_conv_channels=128,
               self_attention_model="rel_pos", subsampling="dw_striding")
    assert parakeet.is_parakeet_config(dict(encoder=enc, preprocessor={}))
    parakeet.Model(dict(encoder=enc, preprocessor={}))
    with pytest.raises(NotImplementedError, match=field):
        parakeet.Model(dict(encoder=dict(enc, **{field: value}), preprocessor={}))
    lib, h = _lib.load(), C.c_void_p()
    assert lib.kk_parakeet_create(C.byref(_lib.KKParakeetConfig(80, 1, 192, 2, 4, 8, 9, 128)), C.byref(h)) != 0
    assert b"d_model" in lib.kk_last_error()


def test_load_model_routes_a_parakeet_config(tmp_path, monkeypatch):
    import json

    from mlx_audio_amd import utils

    enc = dict(feat_in=80, n_layers=1, d_model=128, n_heads=2, ff_expansion_factor=4, subsampling_factor=8, conv_kernel_size=9, subsampling_conv_channels=128,
               self_attention_model="rel_pos", subsampling="dw_striding")
    (tmp_path / "config.json").write_text(json.dumps(dict(encoder=enc, preprocessor=dict(sample_rate=16000, features=80))))
    monkeypatch.setattr(parakeet.Model, "from_pretrained", classmethod(lambda cls, d: ("routed", d)))
    assert utils.load_model(str(tmp_path)) == ("routed", str(tmp_path))


def test_preprocess_args_and_the_filter_bank():
    a = parakeet.PreprocessArgs.from_dict(dict(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=80,
                                               n_fft=512, dither=1e-5, other=1))
    assert (a.win_length, a.hop_length, a.pad_to) == (400, 160, 0)
    bank = parakeet.mel_filter_bank(16000, 512, 80)
    assert bank.shape == (80, 257) and abs(bank.max() - 1.0) < 0.2 and (bank >= 0).all()  # triangles with peaks near 1: no Slaney area normalisation
