"""The host surface of Parakeet's text side (mlx-audio_amd/parakeet.py, csrc/kk_parakeet_text.hip) without a GPU: the ABI, the refusals made before any
launch, the gate-interleaved packing, the alignment data types and the float64 cell restatement against torch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _parakeet_text_ref as R  # noqa: E402

from mlx_audio_amd import _lib, parakeet  # noqa: E402

P = C.c_void_p(4096)  # an aligned pointer that is never followed: every call below is refused first


def test_abi_minor_and_signatures():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kokoro_hip.h")).read()
    assert lib.kk_abi_minor() >= 32 and _lib.PARAKEET_TEXT_MAX_ROWS == int(re.search(r"#define KK_PARAKEET_TEXT_MAX_ROWS (\d+)", hdr).group(1))
    for name in ("kk_op_lstm_pack", "kk_op_lstm_cell_rows", "kk_op_joint_argmax", "kk_op_ctc_argmax", "kk_parakeet_text_create", "kk_parakeet_text_load_tensor",
                 "kk_parakeet_text_finalize", "kk_parakeet_text_state_bytes", "kk_parakeet_text_begin", "kk_parakeet_text_steps", "kk_parakeet_text_read",
                 "kk_parakeet_text_ctc", "kk_parakeet_text_destroy"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, hdr)


@pytest.mark.parametrize("call,message", [
    (lambda lib: lib.kk_op_lstm_cell_rows(None, 1, 48, 64, P, P, None, 0, None, -1, P, 48, P, P, 64, P, P), "input width 48 is not a multiple of 32"),
    (lambda lib: lib.kk_op_lstm_cell_rows(None, 1, 64, 40, P, P, None, 0, None, -1, P, 64, P, P, 64, P, P), "H = 40 is not a multiple of 32"),
    (lambda lib: lib.kk_op_lstm_cell_rows(None, 17, 64, 64, P, P, None, 0, None, -1, P, 64, P, P, 17 * 64, P, P), "M = 17 must be in [1, 16]"),
    (lambda lib: lib.kk_op_joint_argmax(None, 17, 64, 10, 5, 0, P, P, P, 4, P, P, None, P, 1 << 20, P, P), "M = 17 must be in [1, 16]"),
    (lambda lib: lib.kk_op_joint_argmax(None, 1, 72, 10, 5, 0, P, P, P, 4, P, P, None, P, 1 << 20, P, P), "K = 72 is not a multiple of 32"),
    (lambda lib: lib.kk_op_joint_argmax(None, 1, 64, 10, 5, 3, P, P, P, 4, P, P, None, P, 1 << 20, P, P), "unknown activation 3"),
    (lambda lib: lib.kk_op_ctc_argmax(None, 4, 40, 10, P, P, P, 0, 40, None, P, 1 << 20, P), "K = 40 is not a multiple of 32"),
])
def test_refusals(call, message):
    lib = _lib.load()
    assert call(lib) != 0
    assert message in lib.kk_last_error().decode()


def test_gate_interleave_packing():
    g = np.random.default_rng(0)
    n_in, H = 32, 64
    wx, wh, b = g.standard_normal((4 * H, n_in)), g.standard_normal((4 * H, H)), g.standard_normal(4 * H)
    w, bp = parakeet.pack_lstm(wx, wh, b)
    w = (w.view(torch.int16).cpu().numpy() if hasattr(w, "cpu") else w).view(np.uint16)
    bp = bp.cpu().numpy() if hasattr(bp, "cpu") else bp
    perm = R.interleave_rows(H)
    assert sorted(perm) == list(range(4 * H)) and perm[16 + 4 * 2 + 3] == 3 * H + 4 + 2  # tile 1, unit 2 of it, gate o
    assert np.array_equal(bp, b[perm].astype(np.float32))
    cat = torch.tensor(np.concatenate([wx, wh], 1)[perm], dtype=torch.float32).bfloat16().view(torch.int16).numpy().view(np.uint16)
    KS = (n_in + H) // 32
    want = cat.reshape(H // 4, 16, KS, 4, 8).transpose(0, 2, 3, 1, 4)  # [tile][row lr][k-step][g][8] -> [tile][k-step][g][lr][8]
    assert np.array_equal(w.reshape(want.shape), want)


def test_cell_restatement_against_torch():
    g = np.random.default_rng(1)
    n_in, H, M = 32, 64, 3
    wx, wh, b = [R.bf16(g.standard_normal(s) * 0.3) for s in ((4 * H, n_in), (4 * H, H), (4 * H,))]
    x, h, c = R.bf16(g.standard_normal((M, n_in))), R.bf16(g.standard_normal((M, H))), g.standard_normal((M, H))
    cell = torch.nn.LSTMCell(n_in, H).double()
    with torch.no_grad():  # torch's gate order is i, f, g, o as well
        cell.weight_ih.copy_(torch.tensor(wx)), cell.weight_hh.copy_(torch.tensor(wh)), cell.bias_ih.copy_(torch.tensor(b)), cell.bias_hh.zero_()
        hn, cn = cell(torch.tensor(x), (torch.tensor(h), torch.tensor(c)))
    h2, c2 = R.lstm_cell(x, h, c, wx, wh, b)
    assert np.abs(h2 - hn.numpy()).max() < 1e-12 and np.abs(c2 - cn.numpy()).max() < 1e-12


def test_sentences_and_times():
    A = parakeet.AlignedToken
    vocab = ["▁he", "llo", ".", "▁how", "?", "▁3", ".", "5"]
    assert parakeet.decode_tokens([0, 1, 2], vocab) == " hello."
    toks = [A(i, parakeet.decode_tokens([i], vocab), 0.08 * n, 0.08) for n, i in enumerate([0, 1, 2, 3, 4, 5, 6, 7])]
    s = parakeet.tokens_to_sentences(toks)
    assert [x.text for x in s] == [" hello.", " how?", " 3.5"]  # the stop inside 3.5 is followed by a token without a space
    assert s[0].start == 0.0 and abs(s[0].end - 0.24) < 1e-12 and abs(s[1].duration - 0.16) < 1e-12
    r = parakeet.sentences_to_result(s)
    assert r.text == "hello. how? 3.5" and not r.truncated and toks[3].end == toks[3].start + toks[3].duration
    m = parakeet.Model(dict(encoder=ENC, preprocessor=PRE))
    assert m._seconds(7) == 7 * 8 / 16000 * 160  # frame * subsampling_factor / sample_rate * hop_length
    ids = [4, 1, 1, 4, 1, 2, 4, 4]
    assert parakeet.ctc_collapse(ids, 4) == R.ctc_tokens(ids, 4) == [(1, 1, 5), (2, 5, 8)]  # 1 _ 1 is one token; a last token with blanks behind it ends the row
    assert parakeet.ctc_collapse([4, 4], 4) == R.ctc_tokens([4, 4], 4) == []


ENC = dict(feat_in=80, n_layers=1, d_model=128, n_heads=2, ff_expansion_factor=4, subsampling_factor=8, conv_kernel_size=9, subsampling_conv_channels=128,
           self_attention_model="rel_pos", subsampling="dw_striding")
PRE = dict(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=80, n_fft=512)


def tdt_config(V=5, H=32, Hj=32):
    return dict(target="nemo.collections.asr.models.rnnt_bpe_models.EncDecRNNTBPEModel", model_defaults=dict(tdt_durations=[0, 1]), encoder=ENC, preprocessor=PRE,
                decoder=dict(blank_as_pad=True, vocab_size=V, prednet=dict(pred_hidden=H, pred_rnn_layers=1)),
                joint=dict(num_classes=V, vocabulary=[f"▁t{i}" for i in range(V)], num_extra_outputs=2,
                           jointnet=dict(joint_hidden=Hj, activation="relu", encoder_hidden=128, pred_hidden=H)),
                decoding=dict(model_type="tdt", durations=[0, 1], greedy=dict(max_symbols=2)))


def tdt_weights(cfg, g):
    V, H, Hj = cfg["decoder"]["vocab_size"], cfg["decoder"]["prednet"]["pred_hidden"], cfg["joint"]["jointnet"]["joint_hidden"]
    w = {"decoder.prediction.embed.weight": g.standard_normal((V + 1, H)), "joint.pred.weight": g.standard_normal((Hj, H)), "joint.pred.bias": np.zeros(Hj),
         "joint.enc.weight": g.standard_normal((Hj, 128)), "joint.enc.bias": np.zeros(Hj), "joint.joint_net.2.weight": g.standard_normal((V + 3, Hj)),
         "joint.joint_net.2.bias": np.zeros(V + 3)}
    for n, s in (("Wx", (4 * H, H)), ("Wh", (4 * H, H)), ("bias", (4 * H,))):
        w["decoder.prediction.dec_rnn.lstm.0." + n] = g.standard_normal(s)
    return w


def test_partial_set_stays_encoder_only_and_a_misshapen_tensor_is_named():
    cfg, g = tdt_config(), np.random.default_rng(2)
    w = tdt_weights(cfg, g)
    spec = parakeet.text_side_spec(cfg, w)
    assert spec[0]["kind"] == _lib.PARAKEET_TDT and spec[0]["max_symbols"] == 2 and spec[3] == [0, 1] and spec[1]["lstm.0.wx"].shape == (128, 32)
    assert parakeet.text_side_spec(cfg, {k: v for k, v in w.items() if k != "joint.pred.bias"}) is None  # partial: encoder-only, as before
    assert parakeet.text_side_spec(dict(encoder=ENC, preprocessor=PRE), w) is None
    with pytest.raises(ValueError, match="joint.joint_net.2.weight"):
        parakeet.text_side_spec(cfg, dict(w, **{"joint.joint_net.2.weight": np.zeros((9, 32))}))
    m = parakeet.Model(cfg)
    with pytest.raises(NotImplementedError, match="text side"):
        m.decode(np.zeros((16, 80), np.float32))
