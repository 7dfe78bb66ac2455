"""Parakeet (FastConformer) on the device: the encoder's hot blocks that no other kernel of the library serves
(mlx_audio/stt/models/parakeet/attention.py, conformer.py; csrc/kk_parakeet.hip) and the text side -- prediction network, joint and TDT / RNNT /
CTC greedy decoding (rnnt.py, ctc.py, parakeet.py:307-599; csrc/kk_parakeet_text.hip).  The arithmetic runs in libkokoro_hip.so; there is
no PyTorch fallback.  Tensors are torch tensors on the device; work is enqueued on torch's current stream.

    rel_pos_attention(qkv, pos, pos_bias_u, pos_bias_v, heads)   RelPositionMultiHeadAttention after its Linears, rel_shift included
    conformer_dwconv(x, w, bias)                                 silu(bn(depthwise_conv(glu(x)))) of the Convolution module
    conv2d_s2(x, w, bias, stem)                                  a 3 x 3 stride-2 Conv2d of DwStridingSubsampling, channels-last
    fold_batch_norm(...)                                         depth-wise taps and bias with the inference-form BatchNorm folded in (float64)
    rel_positions(T, d_model)                                    RelPositionalEncoding's table for positions T - 1 .. -(T - 1) (float64)
    subsampled_lengths(lengths, factor)                          DwStridingSubsampling's length formula
    pack_lstm(wx, wh, bias) / lstm_cell_rows(...)                one LSTM layer, one step, <= 16 rows, the cell in the matrix kernel's epilogue
    joint_argmax(...) / ctc_argmax(...)                          the joint's output Linear (or the CTC head) with its arg-maxima

    Model(config).load_weights(w) / Model.from_pretrained(dir)   encode(mel) -> (features, lengths); with a complete text side in the checkpoint also
                                                                 decode_features(features, lengths), decode(mel), decode_chunk(audio) -> AlignedResult

    PreprocessArgs, log_mel_spectrogram(audio, args)             parakeet/audio.py's features on the device; Model.encode_audio(audio) chains the two
    AlignedToken, AlignedSentence, AlignedResult, tokens_to_sentences, sentences_to_result, decode_tokens: alignment.py / tokenizer.py on the host

Decoding caps: a TDT / RNNT row holds at most ms * T + 16 tokens and takes at most 2 * ms * T + 32 steps, T its batch's frame count and ms = max_symbols
(8 when the config has none); with max_symbols set the reference itself stays below both, without it a row that would loop for ever ends `truncated`.

What is NOT built: generate (file loading, chunk merging), streaming caches, beam search; ragged masking in the encoder and sub-samplings other
than dw_striding."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field, fields

import numpy as np

from . import _lib

BN_EPS = 1e-5  # mlx.nn.BatchNorm's default, which conformer.py:68 takes


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _want(t, name, dtype, ndim):
    if not (t.is_cuda and t.dtype == dtype and t.dim() == ndim and t.is_contiguous()):
        raise ValueError(f"{name}: need a contiguous {ndim}-d {dtype} tensor on the device")


def rel_positions(T: int, d_model: int) -> np.ndarray:
    """attention.py:155-185: float64 [2 T - 1][d_model], row r is position T - 1 - r, sin in the even and cos in the odd channels.  The slice the
    reference takes from its max_len table depends on T alone, so the table is made for T."""
    pos = np.arange(T - 1, -T, -1, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, d_model, 2, dtype=np.float64) * -(math.log(10000.0) / d_model))
    pe = np.zeros((2 * T - 1, d_model))
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)
    return pe


def subsampled_lengths(lengths, factor: int):
    """conformer.py:241-248: log2(factor) times floor((n + 2 - 3) / 2) + 1"""
    n = np.asarray(lengths, dtype=np.int64)
    for _ in range(int(math.log(factor, 2))):
        n = (n - 1) // 2 + 1
    return n


def fold_batch_norm(dw_weight, dw_bias, bn_weight, bn_bias, running_mean, running_var, eps: float = BN_EPS):
    """Depth-wise Conv1d weight [D][k] (or MLX's [D][k][1]) and bias [D] or None, with y = (conv - mean) / sqrt(var + eps) * weight + bias folded in,
    in float64.  Returns (w fp32 [k][D], bias fp32 [D]) as kk_op_conformer_dwconv takes them."""
    w = np.asarray(dw_weight, dtype=np.float64)
    w = w.reshape(w.shape[0], -1)
    g = np.asarray(bn_weight, np.float64) / np.sqrt(np.asarray(running_var, np.float64) + eps)
    b0 = np.zeros(w.shape[0]) if dw_bias is None else np.asarray(dw_bias, np.float64)
    b = (b0 - np.asarray(running_mean, np.float64)) * g + np.asarray(bn_bias, np.float64)
    return np.ascontiguousarray((w * g[:, None]).T).astype(np.float32), b.astype(np.float32)


def rel_pos_attention(qkv, pos, pos_bias_u, pos_bias_v, heads: int, T: int | None = None, out=None):
    """qkv bf16 [B][T_rows][3 * heads * hd] (q | k | v), pos bf16 [2 T - 1][heads * hd] = linear_pos(rel_positions), pos_bias_u / _v fp32 [heads][hd],
    hd 64 or 128.  Returns bf16 [B][T_rows][heads * hd]; only the first T rows (default: all) are read and written."""
    import torch

    _want(qkv, "qkv", torch.bfloat16, 3)
    _want(pos, "pos", torch.bfloat16, 2)
    _want(pos_bias_u, "pos_bias_u", torch.float32, 2)
    _want(pos_bias_v, "pos_bias_v", torch.float32, 2)
    B, T_rows, ld = qkv.shape
    T = T_rows if T is None else T
    hs = ld // 3
    if ld != 3 * hs or hs % heads != 0:
        raise ValueError("qkv: the last axis must hold q | k | v of `heads` heads")
    hd = hs // heads
    if tuple(pos.shape) != (2 * T - 1, hs):
        raise ValueError(f"pos: need [2 T - 1 = {2 * T - 1}][{hs}], got {tuple(pos.shape)}")
    if tuple(pos_bias_u.shape) != (heads, hd) or tuple(pos_bias_v.shape) != (heads, hd):
        raise ValueError(f"pos_bias_u / pos_bias_v: need [{heads}][{hd}]")
    if out is None:
        out = torch.zeros((B, T_rows, hs), dtype=torch.bfloat16, device=qkv.device)
    else:
        _want(out, "out", torch.bfloat16, 3)
        if tuple(out.shape) != (B, T_rows, hs):
            raise ValueError(f"out: need {(B, T_rows, hs)}")
    lib = _lib.load()
    _lib.check(lib.kk_op_rel_pos_attention(_stream(), B, _p(qkv), ld, T_rows, T, heads, hd, _p(pos), hs, _p(pos_bias_u), _p(pos_bias_v), _p(out), hs),
               "kk_op_rel_pos_attention")
    return out


def conformer_dwconv(x, w, bias):
    """x bf16 [B][T][2 D] (pointwise_conv1's output), w fp32 [k][D] and bias fp32 [D] from fold_batch_norm -> bf16 [B][T][D]"""
    import torch

    _want(x, "x", torch.bfloat16, 3)
    _want(w, "w", torch.float32, 2)
    _want(bias, "bias", torch.float32, 1)
    B, T, D2 = x.shape
    k, D = w.shape
    if D2 != 2 * D or bias.shape[0] != D:
        raise ValueError(f"x has {D2} channels, w and bias are for D = {D}: need 2 D")
    out = torch.empty((B, T, D), dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    _lib.check(lib.kk_op_conformer_dwconv(_stream(), B, _p(x), D2, T, D, k, _p(w), _p(bias), _p(out), D), "kk_op_conformer_dwconv")
    return out


def conv2d_s2(x, w, bias, stem: bool):
    """stem: x fp32 [B][T][F] -> relu(conv) bf16 [B][T'][F'][C].  Otherwise x bf16 [B][T][F][C], depth-wise -> bf16 [B][T'][F'][C].  w fp32 [9][C]
    (tap ky * 3 + kx: a Conv2d weight [C][1][3][3] is w.reshape(C, 9).T), bias fp32 [C].  T' = (T - 1) // 2 + 1, F' likewise."""
    import torch

    _want(x, "x", torch.float32 if stem else torch.bfloat16, 3 if stem else 4)
    _want(w, "w", torch.float32, 2)
    _want(bias, "bias", torch.float32, 1)
    B, T, F = x.shape[:3]
    Cn = w.shape[1]
    if w.shape[0] != 9 or bias.shape[0] != Cn or (not stem and x.shape[3] != Cn):
        raise ValueError("w must be [9][C], bias [C] and a depth-wise input [B][T][F][C]")
    out = torch.empty((B, (T - 1) // 2 + 1, (F - 1) // 2 + 1, Cn), dtype=torch.bfloat16, device=x.device)
    lib = _lib.load()
    _lib.check(lib.kk_op_conv2d_s2(_stream(), B, _p(x), 1 if stem else 0, T, F, Cn, _p(w), _p(bias), _p(out)), "kk_op_conv2d_s2")
    return out


# --------------------------------------------------------------------------------------------------------------------------------- features
@dataclass
class PreprocessArgs:
    """parakeet/audio.py:16-35"""
    sample_rate: int
    normalize: str
    window_size: float
    window_stride: float
    window: str
    features: int
    n_fft: int
    dither: float = 0.0  # unused by the reference's log_mel_spectrogram, and here
    pad_to: int = 0
    pad_value: float = 0

    @property
    def win_length(self) -> int:
        return int(self.window_size * self.sample_rate)

    @property
    def hop_length(self) -> int:
        return int(self.window_stride * self.sample_rate)

    @classmethod
    def from_dict(cls, d: dict):
        return cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})


def window_table(name: str, size: int) -> np.ndarray:
    """mlx_audio/utils.py:10-47 in float64; an unknown name is the Hann window, as audio.py:46-47 has it"""
    n = np.arange(size, dtype=np.float64)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(2 * math.pi * n / (size - 1))
    if name == "blackman":
        return 0.42 - 0.5 * np.cos(2 * math.pi * n / (size - 1)) + 0.08 * np.cos(4 * math.pi * n / (size - 1))
    if name == "bartlett":
        return 1 - 2 * np.abs(n - (size - 1) / 2) / (size - 1)
    return 0.5 * (1 - np.cos(2 * math.pi * n / (size - 1)))


def mel_filter_bank(sample_rate: int, n_fft: int, n_mels: int) -> np.ndarray:
    """The float64 (n_mels, n_fft / 2 + 1) bank that mel_filters(sample_rate, n_fft, n_mels, norm=args.normalize, mel_scale=None) produces
    (mlx_audio/utils.py:165-237): a mel_scale other than "htk" takes the Slaney branch, and a norm other than "slaney" -- "per_feature", say -- leaves
    the triangles un-normalised, with peaks of 1."""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    to_mel = lambda f: min_log_hz / f_sp + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp  # noqa: E731
    freqs = np.linspace(0.0, sample_rate // 2, n_fft // 2 + 1)
    mels = np.linspace(to_mel(0.0), to_mel(sample_rate / 2), n_mels + 2)
    pts = np.where(mels >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (mels - min_log_hz / f_sp)), f_sp * mels)
    diff, slopes = pts[1:] - pts[:-1], pts[None, :] - freqs[:, None]
    return np.maximum(0.0, np.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:])).T


_front_tables = {}


def log_mel_spectrogram(audio, args: PreprocessArgs):
    """audio.py:38-70 on the device (kk_op_parakeet_log_mel): audio [n] or [B][n] samples (numpy or torch, host or device) -> fp32 device
    [1 or B][1 + max(n, pad_to) // hop][features], every row normalised on its own."""
    import torch

    x = torch.as_tensor(audio, dtype=torch.float32).cuda()
    x = (x[None] if x.dim() == 1 else x).contiguous()
    B, n = x.shape
    key = (args.sample_rate, args.n_fft, args.features, args.window, args.win_length)
    if key not in _front_tables:
        j = 2 * math.pi * np.arange(args.n_fft, dtype=np.float64) / args.n_fft
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
        _front_tables[key] = (dev(window_table(args.window, args.win_length)), dev(np.stack([np.cos(j), np.sin(j)])),
                              dev(mel_filter_bank(args.sample_rate, args.n_fft, args.features).T))
    win, cs, fbT = _front_tables[key]
    F = 1 + max(n, args.pad_to) // args.hop_length
    out = torch.empty((B, F, args.features), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().kk_op_parakeet_log_mel(_stream(), B, _p(x), n, n, int(args.pad_to), float(args.pad_value), args.n_fft, args.hop_length,
                                                  args.win_length, args.features, 1 if args.normalize == "per_feature" else 0, _p(win), _p(cs), _p(fbT),
                                                  _p(out)), "kk_op_parakeet_log_mel")
    return out


# ------------------------------------------------------------------------------------------------------------------------------- text side
def pack_lstm(wx, wh, bias=None):
    """MLX's Wx [4H][in], Wh [4H][H], bias [4H] (gates i, f, g, o) -> (w bf16 device, bias fp32 device) as lstm_cell_rows takes them: [Wx | Wh] with
    gate row g H + u at row 16 (u // 4) + 4 (u % 4) + g, in MFMA fragment order (kk_op_lstm_pack).  The packed matrix is also kept as int16 numpy in .host."""
    import torch

    wx, wh = np.ascontiguousarray(wx, dtype=np.float32), np.ascontiguousarray(wh, dtype=np.float32)
    H, n_in = wh.shape[1], wx.shape[1]
    if wx.shape[0] != 4 * H or wh.shape[0] != 4 * H:
        raise ValueError(f"Wx {wx.shape} / Wh {wh.shape}: need [4H][in] and [4H][H]")
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    lib = _lib.load()
    w_out, b_out = np.zeros(max(int(lib.kk_op_lstm_pack_elems(n_in, H)), 1), dtype=np.int16), np.zeros(4 * H, dtype=np.float32)
    _lib.check(lib.kk_op_lstm_pack(wx.ctypes.data, wh.ctypes.data, None if b is None else b.ctypes.data, n_in, H, w_out.ctypes.data, b_out.ctypes.data),
               "kk_op_lstm_pack")
    if not torch.cuda.is_available():
        return w_out, b_out
    return torch.from_numpy(w_out).cuda().view(torch.bfloat16), torch.from_numpy(b_out).cuda()


def lstm_cell_rows(w, bias, h, c, idx, mask, x=None, embed=None, token=None, blank=-1):
    """One LSTM step in place: w, bias from pack_lstm; h, c fp32 [2][M][H] (two copies); idx, mask int32 [M]; x fp32 [M][in], or embed bf16 [n][in] with
    token int32 [M] (a blank token is a zero input).  Row m reads copy idx[m] and writes copy 1 - idx[m]; rows with mask 0 are left alone."""
    M, H = h.shape[1], h.shape[2]
    n_in = (x if embed is None else embed).shape[1]
    _lib.check(_lib.load().kk_op_lstm_cell_rows(_stream(), M, n_in, H, _p(w), _p(bias), None if embed is None else _p(embed), 0 if embed is None else embed.shape[0],
                                                None if token is None else _p(token), int(blank), None if x is None else _p(x), n_in, _p(h), _p(c), M * H,
                                                _p(idx), _p(mask)), "kk_op_lstm_cell_rows")


def joint_argmax(w, bias, encp, t, predp, n_token: int, activation: str = "relu", want_logits: bool = False):
    """w bf16 [C][Hj], bias fp32 [C], encp fp32 [M][T][Hj], t int32 [M], predp fp32 [M][Hj] -> (tok int32 [M] over classes [0, n_token), dur int32 [M] over
    [n_token, C) counted from n_token, logits fp32 [M][C] or None)"""
    import torch

    if activation not in _lib.JOINT_ACTIVATIONS:
        raise ValueError(f"unknown activation {activation!r}: relu, sigmoid or tanh")
    M, T, Hj = encp.shape
    Cn = w.shape[0]
    lib = _lib.load()
    scratch = torch.empty(max(int(lib.kk_op_joint_argmax_scratch_bytes(M, Cn)), 16), dtype=torch.uint8, device="cuda")
    tok, dur = torch.empty(M, dtype=torch.int32, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
    logits = torch.empty((M, Cn), dtype=torch.float32, device="cuda") if want_logits else None
    _lib.check(lib.kk_op_joint_argmax(_stream(), M, Hj, Cn, n_token, _lib.JOINT_ACTIVATIONS[activation], _p(w), _p(bias), _p(encp), T, _p(t), _p(predp),
                                      None if logits is None else _p(logits), _p(scratch), scratch.numel(), _p(tok), _p(dur)), "kk_op_joint_argmax")
    return tok, dur, logits


def ctc_argmax(w, bias, feat, want_logits: bool = False):
    """The CTC head: w bf16 [C][K], bias fp32 [C], feat fp32 or bf16 [rows][K] -> (ids int32 [rows], logits or None)"""
    import torch

    rows, K = feat.shape
    Cn = w.shape[0]
    lib = _lib.load()
    scratch = torch.empty(max(int(lib.kk_op_joint_argmax_scratch_bytes(rows, Cn)), 16), dtype=torch.uint8, device="cuda")
    ids = torch.empty(rows, dtype=torch.int32, device="cuda")
    logits = torch.empty((rows, Cn), dtype=torch.float32, device="cuda") if want_logits else None
    _lib.check(lib.kk_op_ctc_argmax(_stream(), rows, K, Cn, _p(w), _p(bias), _p(feat), _lib.KK_BF16 if feat.dtype == torch.bfloat16 else _lib.KK_F32, K,
                                    None if logits is None else _p(logits), _p(scratch), scratch.numel(), _p(ids)), "kk_op_ctc_argmax")
    return ids, logits


@dataclass
class AlignedToken:
    id: int
    text: str
    start: float
    duration: float
    end: float = 0.0

    def __post_init__(self):
        self.end = self.start + self.duration


@dataclass
class AlignedSentence:
    text: str
    tokens: list
    start: float = 0.0
    end: float = 0.0
    duration: float = 0.0

    def __post_init__(self):
        self.tokens = sorted(self.tokens, key=lambda t: t.start)
        self.start, self.end = self.tokens[0].start, self.tokens[-1].end
        self.duration = self.end - self.start


@dataclass
class AlignedResult:
    text: str
    sentences: list = field(default_factory=list)
    truncated: bool = False  # the row ended at a cap of the device loop, not at its last frame

    def __post_init__(self):
        self.text = self.text.strip()


SENTENCE_ENDS = "!?。？！"


def decode_tokens(tokens, vocabulary) -> str:
    """tokenizer.decode: the pieces joined, the word-start mark as a space"""
    return "".join(vocabulary[t].replace("▁", " ") for t in tokens)


def tokens_to_sentences(tokens) -> list:
    """A sentence ends behind a token that holds one of ! ? and their CJK forms, or a full stop that is last or followed by a token with a space."""
    out, cur = [], []
    for i, tok in enumerate(tokens):
        cur.append(tok)
        if any(ch in tok.text for ch in SENTENCE_ENDS) or ("." in tok.text and (i + 1 == len(tokens) or " " in tokens[i + 1].text)):
            out.append(AlignedSentence("".join(t.text for t in cur), cur))
            cur = []
    if cur:
        out.append(AlignedSentence("".join(t.text for t in cur), cur))
    return out


def sentences_to_result(sentences, truncated: bool = False) -> AlignedResult:
    return AlignedResult("".join(s.text for s in sentences), sentences, truncated)


def ctc_collapse(ids, blank: int):
    """parakeet.py:526-594 on one row's per-frame best ids: [(token, first frame, end frame)] with repeats and blanks dropped.  A token ends where the next one
    starts; the last one ends behind the row's last non-blank frame."""
    ids = np.asarray(ids)
    out, prev = [], -1
    for t in np.flatnonzero(ids != blank):
        if ids[t] != prev:  # (prev survives blanks, as in the reference: a b _ b is one b)
            out.append([int(ids[t]), int(t), 0])
            prev = ids[t]
    for i, e in enumerate(out):
        e[2] = out[i + 1][1] if i + 1 < len(out) else 0
    if out:  # the last non-blank frame behind the last token's first one; the row's last frame when there is none, as in the reference
        later = np.flatnonzero(ids[out[-1][1] + 1:] != blank)
        out[-1][2] = (out[-1][1] + 1 + int(later[-1]) if len(later) else len(ids) - 1) + 1
    return [tuple(e) for e in out]


def text_side_spec(config: dict, w: dict):
    """None when the config or the checkpoint lacks a complete text side; else (KKParakeetTextConfig fields, canonical tensors, vocabulary, durations).
    A complete set with a misshapen tensor raises ValueError naming the checkpoint's tensor."""
    target, tdt = config.get("target", ""), (config.get("model_defaults") or {}).get("tdt_durations")
    dec, joint, decoding = config.get("decoder"), config.get("joint"), config.get("decoding")
    De = config["encoder"]["d_model"]
    f32 = lambda name: np.asarray(w[name], dtype=np.float32)  # noqa: E731

    def shaped(name, shape):
        a = f32(name)
        a = a.reshape(a.shape[0], -1) if a.ndim == 3 else a  # a 1-wide conv, MLX or PyTorch layout
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(np.shape(w[name]))} does not fit the config, need {tuple(shape)}")
        return np.ascontiguousarray(a)

    if target.endswith("EncDecCTCModelBPE"):
        if not (isinstance(dec, dict) and "vocabulary" in dec and "feat_in" in dec):
            return None
        names = ["decoder.decoder_layers.0.weight", "decoder.decoder_layers.0.bias"]
        if any(n not in w for n in names):
            return None
        vocab = list(dec["vocabulary"])
        cfg = dict(kind=_lib.PARAKEET_CTC, vocab=len(vocab), encoder_hidden=int(dec["feat_in"]))
        return cfg, {"ctc.w": shaped(names[0], (len(vocab) + 1, dec["feat_in"])), "ctc.b": shaped(names[1], (len(vocab) + 1,))}, vocab, []
    if not (target.endswith("EncDecRNNTBPEModel") or (target.endswith("EncDecHybridRNNTCTCBPEModel") and tdt is not None)):
        return None
    if not (isinstance(dec, dict) and isinstance(joint, dict) and isinstance(decoding, dict)):
        return None
    net, jn = dec["prednet"], joint["jointnet"]
    H, L, Hj = int(net["pred_hidden"]), int(net["pred_rnn_layers"]), int(jn["joint_hidden"])
    pre = "decoder.prediction."
    names = [pre + "embed.weight", "joint.pred.weight", "joint.pred.bias", "joint.enc.weight", "joint.enc.bias", "joint.joint_net.2.weight", "joint.joint_net.2.bias"]
    names += [pre + f"dec_rnn.lstm.{i}.{n}" for i in range(L) for n in ("Wx", "Wh", "bias")]
    if any(n not in w for n in names):
        return None
    if net.get("rnn_hidden_size") and int(net["rnn_hidden_size"]) != H:
        raise NotImplementedError("decoder.prednet.rnn_hidden_size other than pred_hidden is not built")
    if jn["activation"] not in _lib.JOINT_ACTIVATIONS:
        raise ValueError(f"joint.jointnet.activation = {jn['activation']!r}: relu, sigmoid or tanh")
    vocab = list(joint["vocabulary"])
    durations = [int(d) for d in decoding.get("durations", [])] if tdt is not None else []
    V, n_embed = len(vocab), int(dec["vocab_size"]) + (1 if dec.get("blank_as_pad", True) else 0)
    Cn = V + 1 + len(durations)
    ms = (decoding.get("greedy") or {}).get("max_symbols")
    cfg = dict(kind=_lib.PARAKEET_TDT if tdt is not None else _lib.PARAKEET_RNNT, vocab=V, n_embed=n_embed, pred_hidden=H, pred_layers=L, joint_hidden=Hj,
               encoder_hidden=int(jn.get("encoder_hidden", De)), activation=_lib.JOINT_ACTIVATIONS[jn["activation"]], n_durations=len(durations),
               durations=durations, max_symbols=-1 if ms is None else int(ms))
    t = {"embed": shaped(names[0], (n_embed, H)), "joint.pred.w": shaped(names[1], (Hj, H)), "joint.pred.b": shaped(names[2], (Hj,)),
         "joint.enc.w": shaped(names[3], (Hj, cfg["encoder_hidden"])), "joint.enc.b": shaped(names[4], (Hj,)), "joint.out.w": shaped(names[5], (Cn, Hj)),
         "joint.out.b": shaped(names[6], (Cn,))}
    for i in range(L):
        for src, dst, shape in (("Wx", "wx", (4 * H, H)), ("Wh", "wh", (4 * H, H)), ("bias", "b", (4 * H,))):
            t[f"lstm.{i}.{dst}"] = shaped(pre + f"dec_rnn.lstm.{i}.{src}", shape)
    return cfg, t, vocab, durations


# ---------------------------------------------------------------------------------------------------------------------------------- encoder
CONFORMER_KEYS = ("feat_in", "n_layers", "d_model", "n_heads", "ff_expansion_factor", "subsampling_factor", "conv_kernel_size", "subsampling_conv_channels")
TEXT_SIDE = "the text side of this model is not built (no complete decoder / joint tensor set in the checkpoint): Model.encode gives the encoder states"
GENERATE = "generate (the text side's file loading and chunk merging) is not built: decode_chunk(audio) transcribes one clip"


def is_parakeet_config(config: dict) -> bool:
    enc = config.get("encoder")
    return isinstance(enc, dict) and "preprocessor" in config and "subsampling" in enc and "self_attention_model" in enc


def check_conformer_args(enc: dict):
    """The Conformer variants that are served; anything else is refused by the name of its field."""
    if enc.get("subsampling", "dw_striding") != "dw_striding":
        raise NotImplementedError(f"subsampling = {enc['subsampling']!r}: only 'dw_striding' is built")
    if enc.get("causal_downsampling", False):
        raise NotImplementedError("causal_downsampling = True is not built")
    if enc.get("self_attention_model", "rel_pos") != "rel_pos":
        raise NotImplementedError(f"self_attention_model = {enc['self_attention_model']!r}: only 'rel_pos' is built")
    missing = [k for k in CONFORMER_KEYS if k not in enc]
    if missing:
        raise ValueError(f"encoder config lacks {missing}")


def canonical_tensors(enc: dict, w: dict) -> dict:
    """The reference's encoder parameters (names of conformer.py under `encoder.`, MLX or PyTorch conv layouts: every conv here has one input channel per
    group or a 1-wide kernel, so both flatten alike) -> the float32 tensors kk_parakeet_load_tensor takes, folded in float64:
    BatchNorm into the depth-wise taps, the 1/2 of `x += 0.5 ff(x)` into linear2, sqrt(d_model) of xscaling into pre_encode.out, the columns of
    pre_encode.out from (c, f) to (f, c), q | k | v stacked, absent biases as zeros."""
    D, Cc, n_sub = enc["d_model"], enc["subsampling_conv_channels"], int(math.log2(enc["subsampling_factor"]))
    f64 = lambda name: np.asarray(w[name], dtype=np.float64)  # noqa: E731
    bias = lambda name, n: f64(name) if name in w else np.zeros(n)  # noqa: E731
    out = {}

    def lin(dst, src, n, scale=1.0):
        m = f64(src + ".weight")
        out[dst + ".w"], out[dst + ".b"] = m.reshape(m.shape[0], -1) * scale, bias(src + ".bias", n) * scale

    pre = "encoder.pre_encode."
    out["pre.stem.w"], out["pre.stem.b"] = f64(pre + "conv.0.weight").reshape(Cc, 9).T, bias(pre + "conv.0.bias", Cc)
    for i in range(1, n_sub):
        out[f"pre.{i}.dw.w"], out[f"pre.{i}.dw.b"] = f64(pre + f"conv.{3 * i - 1}.weight").reshape(Cc, 9).T, bias(pre + f"conv.{3 * i - 1}.bias", Cc)
        lin(f"pre.{i}.pw", pre + f"conv.{3 * i}", Cc)
    xs = math.sqrt(D) if enc.get("xscaling", False) else 1.0
    wo = f64(pre + "out.weight")
    f_out = wo.shape[1] // Cc
    out["pre.out.w"], out["pre.out.b"] = wo.reshape(D, Cc, f_out).transpose(0, 2, 1).reshape(D, -1) * xs, bias(pre + "out.bias", D) * xs
    for li in range(enc["n_layers"]):
        s, d = f"encoder.layers.{li}.", f"L{li}."
        for dst, src in (("ff1.ln", "norm_feed_forward1"), ("att.ln", "norm_self_att"), ("conv.ln", "norm_conv"), ("ff2.ln", "norm_feed_forward2"),
                         ("out.ln", "norm_out")):
            out[d + dst + ".w"], out[d + dst + ".b"] = f64(s + src + ".weight"), f64(s + src + ".bias")
        for ff in ("1", "2"):
            lin(d + f"ff{ff}.a", s + f"feed_forward{ff}.linear1", D * enc["ff_expansion_factor"])
            lin(d + f"ff{ff}.b", s + f"feed_forward{ff}.linear2", D, 0.5)
        a = s + "self_attn."
        out[d + "qkv.w"] = np.concatenate([f64(a + f"linear_{n}.weight") for n in "qkv"])
        out[d + "qkv.b"] = np.concatenate([bias(a + f"linear_{n}.bias", D) for n in "qkv"])
        out[d + "pos.w"], out[d + "pos.b"] = f64(a + "linear_pos.weight"), np.zeros(D)
        lin(d + "o", a + "linear_out", D)
        out[d + "u"], out[d + "v"] = f64(a + "pos_bias_u").reshape(-1), f64(a + "pos_bias_v").reshape(-1)
        lin(d + "pw1", s + "conv.pointwise_conv1", 2 * D)
        lin(d + "pw2", s + "conv.pointwise_conv2", D)
        bn = s + "conv.batch_norm."
        out[d + "dw.w"], out[d + "dw.b"] = fold_batch_norm(f64(s + "conv.depthwise_conv.weight"), w.get(s + "conv.depthwise_conv.bias"), f64(bn + "weight"),
                                                           f64(bn + "bias"), f64(bn + "running_mean"), f64(bn + "running_var"))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


class Model:
    """parakeet.py's model, audio side: `encode(mel) -> (features, lengths)` on the device (kk_parakeet_*).  config: the checkpoint's config.json as a dict
    (its `encoder` block is ConformerArgs)."""

    def __init__(self, config: dict):
        self.config = config
        self.enc = dict(config["encoder"])
        check_conformer_args(self.enc)
        self.preprocessor = PreprocessArgs.from_dict(config["preprocessor"]) if config.get("preprocessor") else None
        self._h, self._pos, self._ws, self.text_side_weights = None, {}, {}, {}
        self._text, self.vocabulary, self.durations, self.check_interval = None, [], [], 32

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().kk_parakeet_destroy(self._h)
        if getattr(self, "_text", None):
            _lib.load().kk_parakeet_text_destroy(self._text)

    def load_weights(self, weights: dict):
        """weights: name -> array (numpy, or anything np.asarray takes).  `decoder.*`, `joint.*` and `ctc.*` are kept in text_side_weights; the text side is
        built when the config has its blocks and the checkpoint its complete tensor set (text_side_spec), else the model stays encoder-only."""
        import torch

        lib = _lib.load()
        w = {k: (v.float().cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in weights.items()}
        self.text_side_weights = {k: v for k, v in w.items() if k.split(".")[0] in ("decoder", "joint", "ctc")}
        h = C.c_void_p()
        _lib.check(lib.kk_parakeet_create(C.byref(_lib.KKParakeetConfig(*[int(self.enc[k]) for k in CONFORMER_KEYS])), C.byref(h)), "kk_parakeet_create")
        self._h = h
        for name, a in canonical_tensors(self.enc, w).items():
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _lib.check(lib.kk_parakeet_load_tensor(h, name.encode(), shape, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_parakeet_load_tensor")
        torch.cuda.init()
        _lib.check(lib.kk_parakeet_finalize(h, _stream()), "kk_parakeet_finalize")
        spec = text_side_spec(self.config, w)
        if spec is not None:
            cfg, tensors, self.vocabulary, self.durations = spec
            c = _lib.KKParakeetTextConfig()
            for k, v in cfg.items():
                setattr(c, k, (C.c_int32 * 16)(*v) if k == "durations" else v)
            th = C.c_void_p()
            _lib.check(lib.kk_parakeet_text_create(C.byref(c), C.byref(th)), "kk_parakeet_text_create")
            self._text, self._text_cfg = th, cfg
            for name, a in tensors.items():
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(lib.kk_parakeet_text_load_tensor(th, name.encode(), shape, a.ndim, a.ctypes.data_as(C.c_void_p)), "kk_parakeet_text_load_tensor")
            _lib.check(lib.kk_parakeet_text_finalize(th, _stream()), "kk_parakeet_text_finalize")
        return self

    @classmethod
    def from_pretrained(cls, local_dir):
        """A local directory with config.json and *.safetensors"""
        import glob
        import json
        import os

        from safetensors import safe_open

        with open(os.path.join(local_dir, "config.json")) as f:
            model = cls(json.load(f))
        weights = {}
        for path in sorted(glob.glob(os.path.join(local_dir, "*.safetensors"))):
            with safe_open(path, framework="np") as f:
                weights.update({k: f.get_tensor(k) for k in f.keys()})
        if not weights:
            raise FileNotFoundError(f"No safetensors found in {local_dir}")
        return model.load_weights(weights)

    def encode(self, mel, cache=None):
        """mel [B][T_mel][feat_in] or [T_mel][feat_in] (torch or numpy; every item has T_mel frames, no mask is applied, as in the reference) ->
        (features fp32 device [B][T'][d_model], lengths int64 numpy [B])"""
        import torch

        if cache is not None:
            raise NotImplementedError("cache: streaming caches are not built")
        if self._h is None:
            raise RuntimeError("load_weights first")
        mel = torch.as_tensor(mel, dtype=torch.float32).cuda()
        mel = (mel[None] if mel.dim() == 2 else mel).contiguous()
        B, T_mel, F = mel.shape
        if F != self.enc["feat_in"]:
            raise ValueError(f"mel has {F} features, feat_in = {self.enc['feat_in']}")
        lib = _lib.load()
        T, D = lib.kk_parakeet_encode_frames(self._h, T_mel), self.enc["d_model"]
        if T not in self._pos:
            self._pos[T] = torch.from_numpy(rel_positions(T, D)).to(torch.float32).cuda().to(torch.bfloat16).contiguous()
        if (B, T_mel) not in self._ws:  # the workspace of the last shape is kept across calls
            self._ws = {(B, T_mel): torch.empty(lib.kk_parakeet_encode_workspace_bytes(self._h, B, T_mel), dtype=torch.uint8, device="cuda")}
        ws = self._ws[(B, T_mel)]
        nbytes = ws.numel()
        out = torch.empty((B, T, D), dtype=torch.float32, device="cuda")
        _lib.check(lib.kk_parakeet_encode(self._h, _stream(), B, T_mel, _p(mel), _p(self._pos[T]), _p(ws), nbytes, _p(out)), "kk_parakeet_encode")
        return out, subsampled_lengths([T_mel] * B, self.enc["subsampling_factor"])

    def encode_audio(self, audio):
        """samples [n] or [B][n] at preprocessor.sample_rate -> encode(log_mel_spectrogram(audio, preprocessor))"""
        if self.preprocessor is None:
            raise ValueError("the config has no preprocessor block")
        return self.encode(log_mel_spectrogram(audio, self.preprocessor))

    def _seconds(self, frames):
        """frame count -> seconds, as the reference writes it: frames * subsampling_factor / sample_rate * hop_length"""
        return frames * self.enc["subsampling_factor"] / self.preprocessor.sample_rate * self.preprocessor.hop_length

    def _result(self, triples, truncated=False):
        toks = [AlignedToken(tok, decode_tokens([tok], self.vocabulary), self._seconds(start), dur) for tok, start, dur in triples]
        return sentences_to_result(tokens_to_sentences(toks), truncated)

    def decode_features_raw(self, features, lengths):
        """The device loop alone: per row ([(token, frame, duration index)], truncated) for TDT / RNNT, ([(token, first frame, end frame)], False) for CTC"""
        import torch

        if self._text is None:
            raise NotImplementedError(TEXT_SIDE)
        lib, cfg = _lib.load(), self._text_cfg
        features = torch.as_tensor(features, dtype=torch.float32).cuda().contiguous()
        B, T, D = features.shape
        lengths = np.asarray(lengths, dtype=np.int32)
        if D != cfg["encoder_hidden"] or lengths.shape != (B,) or lengths.min() < 0 or lengths.max() > T:
            raise ValueError(f"features {tuple(features.shape)} / lengths {lengths.tolist()}: need [B][T][{cfg['encoder_hidden']}] and B lengths in [0, T]")
        if cfg["kind"] == _lib.PARAKEET_CTC:
            ws = torch.empty(lib.kk_parakeet_text_state_bytes(self._text, B * T, 1, 1), dtype=torch.uint8, device="cuda")
            ids = torch.empty(B * T, dtype=torch.int32, device="cuda")
            _lib.check(lib.kk_parakeet_text_ctc(self._text, _stream(), B * T, _p(features), _p(ids), _p(ws), ws.numel()), "kk_parakeet_text_ctc")
            ids = ids.cpu().numpy().reshape(B, T)
            return [(ctc_collapse(ids[b, :lengths[b]], cfg["vocab"]), False) for b in range(B)]
        out = []
        for b0 in range(0, B, _lib.PARAKEET_TEXT_MAX_ROWS):  # batches of up to 16 rows in lock step
            n = min(_lib.PARAKEET_TEXT_MAX_ROWS, B - b0)
            ms = cfg["max_symbols"] if cfg["max_symbols"] > 0 else 8
            cap, step_cap = ms * T + 16, 2 * ms * T + 32
            state = torch.empty(lib.kk_parakeet_text_state_bytes(self._text, n, T, cap), dtype=torch.uint8, device="cuda")
            lens = np.ascontiguousarray(lengths[b0:b0 + n])
            _lib.check(lib.kk_parakeet_text_begin(self._text, _stream(), n, T, _p(features[b0:b0 + n]), lens.ctypes.data, cap, step_cap, _p(state), state.numel()),
                       "kk_parakeet_text_begin")
            live = C.c_int32(1)
            while live.value > 0:  # the only host reads inside the loop: one counter every check_interval steps
                _lib.check(lib.kk_parakeet_text_steps(self._text, _stream(), self.check_interval, C.byref(live)), "kk_parakeet_text_steps")
            counts, flags, toks = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, cap, 3), np.int32)
            _lib.check(lib.kk_parakeet_text_read(self._text, _stream(), counts.ctypes.data, flags.ctypes.data, toks.ctypes.data), "kk_parakeet_text_read")
            out += [([tuple(int(v) for v in toks[b, i]) for i in range(counts[b])], bool(flags[b] == 2)) for b in range(n)]
        return out

    def decode_features(self, features, lengths):
        """features fp32 [B][T][d_model] on the device, lengths [B] (ragged) -> [AlignedResult]: greedy TDT / RNNT / CTC decoding (a hybrid TDT-CTC checkpoint
        decodes with TDT, as in the reference)"""
        if self._text is not None and self.preprocessor is None:
            raise ValueError("the config has no preprocessor block: token times need its sample_rate and hop")
        res, kind = [], self._text_cfg["kind"] if self._text is not None else None
        for triples, truncated in self.decode_features_raw(features, lengths):
            if kind == _lib.PARAKEET_CTC:
                res.append(self._result([(tok, a, self._seconds(e) - self._seconds(a)) for tok, a, e in triples]))
            else:
                res.append(self._result([(tok, t, self._seconds(self.durations[d] if kind == _lib.PARAKEET_TDT else 1)) for tok, t, d in triples], truncated))
        return res

    def decode(self, mel):
        """mel [B][T_mel][feat_in] or [T_mel][feat_in] -> [AlignedResult]"""
        if self._text is None:
            raise NotImplementedError(TEXT_SIDE)
        return self.decode_features(*self.encode(mel))

    def decode_chunk(self, audio, verbose: bool = False):
        """samples [n] at preprocessor.sample_rate -> AlignedResult"""
        if self._text is None:
            raise NotImplementedError(TEXT_SIDE)
        result = self.decode(log_mel_spectrogram(audio, self.preprocessor))[0]
        if verbose:
            print(result.text)
        return result

    def generate(self, *a, **k):
        raise NotImplementedError(GENERATE if self._text is not None else TEXT_SIDE)
