"""Host surface of the SNAC codec (mlx-audio_amd/snac.py, kk_snac_* of include/kokoro_hip.h), no GPU: the ABI, what is refused, and the
parameter names `load_weights` consumes."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _snac_ref as R
from mlx_audio_amd import _lib, snac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["kk_snac_create", "kk_snac_destroy", "kk_snac_load_tensor", "kk_snac_finalize", "kk_snac_hop_length", "kk_snac_decode_samples",
           "kk_snac_decode_workspace_bytes", "kk_snac_decode", "kk_snac_encode_frames", "kk_snac_encode_workspace_bytes", "kk_snac_encode",
           "kk_snac_debug_info", "kk_snac_debug_fetch", "kk_op_snac_dw_conv", "kk_op_snac_residual_unit", "kk_op_snac_from_codes",
           "kk_op_snac_vq_search", "kk_op_snac_conv_cout1"]


def test_abi_minor_and_signatures():
    lib = _lib.load()
    assert lib.kk_abi_version() == 2 and lib.kk_abi_minor() >= 28
    hdr = open(os.path.join(ROOT, "include", "kokoro_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"{name}(" in hdr, name
    # argument counts follow the header's declarations
    import re

    for name in SYMBOLS:
        decl = re.search(r"\b" + name + r"\(([^;]*?)\);", hdr, re.S).group(1)
        n = 0 if decl.strip() in ("", "void") else decl.count(",") + 1
        assert len(_lib.SIGNATURES[name][1]) == n, (name, n)
    assert C.sizeof(_lib.KKSnacConfig) == 4 * (2 + 1 + 8 + 2 + 1 + 8 + 4 + 8 + 2 + 1)


def test_refusals_name_the_field_before_anything_runs():
    base = dict(R.CONFIGS["even"])
    with pytest.raises(NotImplementedError, match="attn_window_size"):
        snac.SNAC(snac.SNACConfig(**dict(base, attn_window_size=32)))
    with pytest.raises(NotImplementedError, match="attn_window_size"):
        snac.SNAC(snac.SNACConfig())  # the reference's defaults are the 44 kHz model with LocalMHA
    with pytest.raises(NotImplementedError, match="depthwise"):
        snac.SNAC(snac.SNACConfig(**dict(base, depthwise=False)))
    with pytest.raises(NotImplementedError, match="attn_window_size"):
        snac.param_shapes(snac.SNACConfig(**dict(base, attn_window_size=32)))
    m = snac.SNAC(snac.SNACConfig(**base))  # no weights, no GPU needed
    with pytest.raises(NotImplementedError, match="__call__"):
        m(torch.zeros(1, 1, 64))
    with pytest.raises(NotImplementedError, match="lengths"):
        m.encode(torch.zeros(2, 1, 64), lengths=[64, 32])
    with pytest.raises(NotImplementedError, match="lengths"):
        m.encode([torch.zeros(1, 64), torch.zeros(1, 32)])
    with pytest.raises(NotImplementedError, match="lengths"):
        m.decode([torch.zeros(2, 1), torch.zeros(2, 2), torch.zeros(2, 4)], lengths=[4, 2])
    with pytest.raises(ValueError, match="compute_dtype"):
        snac.SNAC(snac.SNACConfig(**base), compute_dtype="float16")
    # the library refuses the same fields on its own
    lib = _lib.load()
    kc = _lib.KKSnacConfig()
    kc.encoder_dim, kc.latent_dim, kc.decoder_dim, kc.codebook_size, kc.codebook_dim = 4, 16, 32, 37, 8
    kc.n_encoder_rates = kc.n_decoder_rates = kc.n_vq = 1
    kc.encoder_rates[0] = kc.decoder_rates[0] = 2
    kc.vq_strides[0] = 1
    kc.depthwise, kc.attn_window_size = 1, 32
    h = C.c_void_p()
    assert lib.kk_snac_create(C.byref(kc), C.byref(h)) != 0 and b"attn_window_size" in lib.kk_last_error()
    kc.depthwise, kc.attn_window_size = 0, 0
    assert lib.kk_snac_create(C.byref(kc), C.byref(h)) != 0 and b"depthwise" in lib.kk_last_error()
    kc.depthwise = 1
    assert lib.kk_snac_create(C.byref(kc), C.byref(h)) == 0
    assert lib.kk_snac_hop_length(h) == 2 and lib.kk_snac_decode_workspace_bytes(h, 1, 4) == 0  # not finalized
    assert lib.kk_snac_decode(h, None, 1, 4, None, None, None, 0, None) != 0 and b"finalized" in lib.kk_last_error()
    lib.kk_snac_destroy(h)


def test_load_weights_consumes_exactly_the_reference_parameter_names():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "snac_24khz_names.json")))
    cfg = snac.SNACConfig.from_dict(g["config"])
    assert cfg == snac.snac_24khz() and cfg.latent_dim == 768
    want = {k: list(v) for k, v in snac.param_shapes(cfg).items()}
    assert want == g["parameters"] and len(want) == 269
    # on a small tree: every name is required (a missing one fails with its name), a wrong shape fails with the name, extras are ignored
    small = snac.SNACConfig(**R.CONFIGS["even"])
    shapes = snac.param_shapes(small)
    w = R.synth_weights(shapes, 0)
    for name in list(shapes)[:: max(1, len(shapes) // 12)] + [list(shapes)[-1]]:
        with pytest.raises(ValueError, match="missing parameter: " + name.replace(".", r"\.") + "$"):
            snac.SNAC(small).load_weights({k: v for k, v in w.items() if k != name})
    bad = dict(w)
    bad["decoder.model.layers.1.weight_v"] = np.zeros((32, 1, 15), np.float32)
    with pytest.raises(ValueError, match=r"decoder\.model\.layers\.1\.weight_v"):
        snac.SNAC(small).load_weights(bad)
    if not torch.cuda.is_available():  # every name present: only the upload is left, and that needs the device
        with pytest.raises(_lib.KokoroHipError, match="GPU"):
            snac.SNAC(small).load_weights(dict(w, extra=np.zeros(3, np.float32)))


def test_from_config_and_from_pretrained_read_a_local_directory_only(tmp_path):
    json.dump(dict(R.CONFIGS["odd"]), open(tmp_path / "config.json", "w"))
    m = snac.SNAC.from_config(tmp_path / "config.json")
    assert m.cfg.encoder_rates == [3, 2] and m.cfg.noise is False and m.hop_length == 6 and m.noise_channels == []
    with pytest.raises(FileNotFoundError):
        snac.SNAC.from_pretrained("hubertsiuzdak/snac_24khz")  # a repository id is not a local directory: nothing is fetched
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        snac.SNAC.from_pretrained(str(tmp_path))


def test_draw_noise_is_per_item():
    m = snac.SNAC(snac.SNACConfig(**R.CONFIGS["even"]))
    a, b = m.draw_noise(3, seed=5), m.draw_noise(1, seed=6)
    assert [tuple(t.shape) for t in a] == [(3, 1, 16), (3, 1, 8)]
    assert all(torch.equal(x[1:2], y) for x, y in zip(a, b))  # item 1 of seed 5 is item 0 of seed 6
    assert not torch.equal(a[0][0], a[0][1])
