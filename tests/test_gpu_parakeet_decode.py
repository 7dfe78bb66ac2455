"""Parakeet greedy decoding on the device (parakeet.Model.decode_features, kk_parakeet_text_*) against the float64 replay of the reference
loops in tests/_parakeet_text_ref.py: tiny synthetic models (pred_hidden 96, two LSTM layers, joint_hidden 64, 37 tokens, durations 0 .. 4, max_symbols 2, a
blank bias that makes blanks common), ragged lengths.  The (token, frame, duration) lists, the text and the times must be equal.  Two conditions are
asserted on the replay itself: every arg-maximum it takes has a top-1 / top-2 margin of at least 16 x LOGIT_ERR, and the walk holds a blank, an
emission, a duration-0 emission, a max_symbols forced advance and a skip of more than one frame."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _parakeet_ref as PR  # noqa: E402
import _parakeet_text_ref as R  # noqa: E402

from mlx_audio_amd import parakeet, utils  # noqa: E402

pytestmark = pytest.mark.gpu
LOGIT_ERR = 1.9e-6  # the largest logit error test_gpu_parakeet_text_kernels.py::test_joint_argmax measured
H, L, HJ, V, DE, DUR = 96, 2, 64, 37, 128, [0, 1, 2, 3, 4]
LENGTHS = [1, 7, 26]
SEEDS = {"tdt": 6, "rnnt": 0, "ctc": 2}  # chosen on the CPU: the replay alone meets both conditions
ENC = dict(self_attention_model="rel_pos", subsampling="dw_striding", pos_emb_max_len=5000, ff_expansion_factor=4, feat_in=80, d_model=DE, n_heads=2, n_layers=1,
           subsampling_factor=8, subsampling_conv_channels=128, conv_kernel_size=9, use_bias=True, xscaling=False)
PRE = dict(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=80, n_fft=512)
VOCAB = [("▁" if i % 3 == 0 else "") + "abcdefghijklmnopqrstuvwxyz"[i % 26] + ("." if i % 7 == 6 else "") for i in range(V)]
_made = {}


def case(kind, max_symbols=2, always_blank=False):
    """(config, weights, replay parameters, features [3][26][DE]), made once per kind"""
    key = (kind, max_symbols, always_blank)
    if key in _made:
        return _made[key]
    g = np.random.default_rng(SEEDS[kind])
    nd = len(DUR) if kind == "tdt" else 0
    u = lambda *s: g.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    feat = u(3, max(LENGTHS), DE)
    if kind == "ctc":
        w = {"decoder.decoder_layers.0.weight": u(V + 1, 1, DE), "decoder.decoder_layers.0.bias": u(V + 1)}
        w["decoder.decoder_layers.0.bias"][V] += 1.5
        cfg = dict(target="nemo.collections.asr.models.ctc_bpe_models.EncDecCTCModelBPE", encoder=ENC, preprocessor=PRE,
                   decoder=dict(feat_in=DE, num_classes=V, vocabulary=VOCAB), decoding=dict(greedy={}))
        _made[key] = (cfg, w, None, feat)
        return _made[key]
    pre = "decoder.prediction."
    w = {pre + "embed.weight": u(V + 1, H), "joint.pred.weight": u(HJ, H), "joint.pred.bias": u(HJ), "joint.enc.weight": u(HJ, DE) * 0.3, "joint.enc.bias": u(HJ),
         "joint.joint_net.2.weight": u(V + 1 + nd, HJ), "joint.joint_net.2.bias": u(V + 1 + nd)}
    w["joint.joint_net.2.bias"][V] += 4.0  # blanks are common
    if always_blank:
        w["joint.joint_net.2.weight"][:] = 0
        w["joint.joint_net.2.bias"][:] = 0
        w["joint.joint_net.2.bias"][[V, V + 1]] = 1.0  # the blank, duration 0: the reference would never leave the frame
    for i in range(L):
        for n, s in (("Wx", (4 * H, H)), ("Wh", (4 * H, H)), ("bias", (4 * H,))):
            w[pre + f"dec_rnn.lstm.{i}.{n}"] = u(*s) * 0.2
    cfg = dict(target="nemo.collections.asr.models.rnnt_bpe_models.EncDecRNNTBPEModel", model_defaults=dict(tdt_durations=DUR if kind == "tdt" else None),
               encoder=ENC, preprocessor=PRE, decoder=dict(blank_as_pad=True, vocab_size=V, prednet=dict(pred_hidden=H, pred_rnn_layers=L)),
               joint=dict(num_classes=V, vocabulary=VOCAB, num_extra_outputs=nd, jointnet=dict(joint_hidden=HJ, activation="relu", encoder_hidden=DE, pred_hidden=H)),
               decoding=dict(model_type=kind, durations=DUR, greedy=dict(max_symbols=max_symbols)))
    P = dict(embed=w[pre + "embed.weight"], lstm=[tuple(w[pre + f"dec_rnn.lstm.{i}.{n}"] for n in ("Wx", "Wh", "bias")) for i in range(L)],
             pred=(w["joint.pred.weight"], w["joint.pred.bias"]), enc=(w["joint.enc.weight"], w["joint.enc.bias"]),
             out=(w["joint.joint_net.2.weight"], w["joint.joint_net.2.bias"]), act="relu", V=V, durations=DUR)
    _made[key] = (cfg, w, P, feat)
    return _made[key]


def model_of(cfg, w, seed=5):
    return parakeet.Model(cfg).load_weights(dict(PR.Encoder(ENC, seed=seed).weights(), **w))


@pytest.mark.parametrize("rows", [[2], [0, 1, 2]])
@pytest.mark.parametrize("kind", ["tdt", "rnnt"])
def test_decode_against_the_replay(kind, rows):
    cfg, w, P, feat = case(kind)
    want, events, margin = [], set(), np.inf
    for b in rows:
        triples, margins, ev = R.greedy(P, feat[b], LENGTHS[b], kind, 2)
        want.append(triples)
        events |= ev
        margin = min(margin, min(margins))
    print(f"{kind} rows {rows}: smallest margin {margin:.3e} = {margin / LOGIT_ERR:.0f} x the logit error, events {sorted(events)}")
    assert margin >= 16 * LOGIT_ERR
    if len(rows) == 3:
        assert events >= ({"blank", "emission", "duration0", "forced", "skip"} if kind == "tdt" else {"blank", "emission", "forced"})
    model = model_of(cfg, w)
    f, lens = torch.from_numpy(feat[rows]).cuda(), [LENGTHS[b] for b in rows]
    got = model.decode_features_raw(f, lens)
    assert [g[0] for g in got] == want and not any(g[1] for g in got)
    res = model.decode_features(f, lens)
    for r, triples in zip(res, want):
        toks = [t for s in r.sentences for t in s.tokens]
        sec = lambda n: n * 8 / 16000 * 160  # noqa: E731
        assert r.text == "".join(VOCAB[t].replace("▁", " ") for t, _, _ in triples).strip()
        assert [(t.id, t.start, t.duration) for t in toks] == [(t, sec(fr), sec(DUR[d] if kind == "tdt" else 1)) for t, fr, d in triples]
        assert all(s.start == s.tokens[0].start and s.end == s.tokens[-1].end for s in r.sentences)
    if len(rows) == 3:  # a row decoded alone is bit-equal to the same row in the batch
        assert model.decode_features_raw(f[2:3], lens[2:3])[0] == got[2]


def test_no_max_symbols_ends_truncated():
    cfg, w, P, feat = case("tdt", max_symbols=None, always_blank=True)
    model = model_of(cfg, w)
    model.check_interval = 64
    (triples, truncated), = model.decode_features_raw(torch.from_numpy(feat[1:2, :4]).cuda(), [4])
    assert triples == [] and truncated  # 2 * 8 * 4 + 32 steps on frame 0, then the cap


def test_ctc_against_the_restatement():
    cfg, w, _, feat = case("ctc")
    model = model_of(cfg, w)
    z = R.linear(feat[:2].reshape(-1, DE), w["decoder.decoder_layers.0.weight"].reshape(V + 1, DE), w["decoder.decoder_layers.0.bias"]).reshape(2, -1, V + 1)
    s = np.sort(z, -1)
    assert (s[..., -1] - s[..., -2]).min() >= 16 * LOGIT_ERR
    lens = [26, 9]
    got = model.decode_features_raw(torch.from_numpy(feat[:2]).cuda(), lens)
    want = [R.ctc_tokens(z[b, :lens[b]].argmax(-1), V) for b in range(2)]
    assert [g[0] for g in got] == want and len(want[0]) > 3
    res = model.decode_features(torch.from_numpy(feat[:2]).cuda(), lens)
    toks = [t for s in res[0].sentences for t in s.tokens]
    assert [(t.id, t.start) for t in toks] == [(k, a * 8 / 16000 * 160) for k, a, _ in want[0]]
    assert np.allclose([t.duration for t in toks], [(e - a) * 0.08 for _, a, e in want[0]], rtol=0, atol=1e-12)


def test_from_pretrained_with_a_text_side(tmp_path):
    from safetensors.numpy import save_file

    cfg, w, _, _ = case("tdt")
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in dict(PR.Encoder(ENC, seed=5).weights(), **w).items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    model = utils.load_model(str(tmp_path))
    mel = torch.randn((1, 203, 80), generator=torch.Generator().manual_seed(1))
    res = model.decode(mel)
    assert isinstance(res[0], parakeet.AlignedResult) and isinstance(res[0].text, str)
    assert res[0].text == model_of(cfg, w).decode(mel)[0].text
    with pytest.raises(NotImplementedError, match="text side"):
        model.generate("clip.wav")
