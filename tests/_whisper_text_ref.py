"""CPU references of the Whisper text side (mlx-audio_amd/whisper_decoding.py, csrc/kk_whisper_text.hip and kk_whisper_text_kernels.hip): synthetic decoder weights under
the MLX names, transformers' WhisperDecoder carrying them (the independent yardstick of the GPU tests), and a numpy restatement of the logit filters and
the greedy update of mlx_audio/stt/models/whisper/decoding.py:255-395 in this repository's own words.  tests/test_whisper_text_cpu.py pins the
restatement against transformers' logits processors; the GPU tests compare the pick kernel against it."""
import math

import numpy as np

from _whisper_ref import bf16_round

NEG = -np.inf


# ---- synthetic decoders ---------------------------------------------------------------------------------------------------------------------
def dims(width, heads, layers, n_vocab, audio_ctx, text_ctx=448):
    from mlx_audio_amd.whisper import ModelDimensions

    return ModelDimensions(80, audio_ctx, width, heads, 1, n_vocab, text_ctx, width, heads, layers)


SHAPE_A = dict(width=128, heads=2, layers=2, n_vocab=51865, audio_ctx=100)
SHAPE_B = dict(width=384, heads=6, layers=1, n_vocab=51866, audio_ctx=1500)


def decoder_weights(d, seed):
    """MLX-named decoder parameters, pre-rounded to bf16: matrices N(0, 1 / fan_in), the embedding N(0, 4 / D) (logits with a standard deviation of about 2 behind
    the final LayerNorm), LayerNorm gains 1 + 0.2 N, biases and positions 0.1 N; no key bias."""
    g = np.random.default_rng(seed)
    D, V = d.n_text_state, d.n_vocab

    def mat(*shape, fan_in):
        return bf16_round((g.standard_normal(shape) / math.sqrt(fan_in)).astype(np.float32))

    def vec(n, gain=False):
        return bf16_round(((1.0 if gain else 0.0) + (0.2 if gain else 0.1) * g.standard_normal(n)).astype(np.float32))

    w = {"decoder.token_embedding.weight": mat(V, D, fan_in=D / 4.0),
         "decoder.positional_embedding": bf16_round((0.1 * g.standard_normal((d.n_text_ctx, D))).astype(np.float32)),
         "decoder.ln.weight": vec(D, gain=True), "decoder.ln.bias": vec(D)}
    for i in range(d.n_text_layer):
        p = f"decoder.blocks.{i}."
        for att in ("attn", "cross_attn"):
            for lin in ("query", "key", "value", "out"):
                w[p + f"{att}.{lin}.weight"] = mat(D, D, fan_in=D)
                if lin != "key":
                    w[p + f"{att}.{lin}.bias"] = vec(D)
        w[p + "mlp1.weight"], w[p + "mlp1.bias"] = mat(4 * D, D, fan_in=D), vec(4 * D)
        w[p + "mlp2.weight"], w[p + "mlp2.bias"] = mat(D, 4 * D, fan_in=4 * D), vec(D)
        for ln in ("attn_ln", "cross_attn_ln", "mlp_ln"):
            w[p + ln + ".weight"], w[p + ln + ".bias"] = vec(D, gain=True), vec(D)
    return w


HF_NAMES = {"attn.query": "self_attn.q_proj", "attn.key": "self_attn.k_proj", "attn.value": "self_attn.v_proj", "attn.out": "self_attn.out_proj",
            "cross_attn.query": "encoder_attn.q_proj", "cross_attn.key": "encoder_attn.k_proj", "cross_attn.value": "encoder_attn.v_proj",
            "cross_attn.out": "encoder_attn.out_proj", "mlp1": "fc1", "mlp2": "fc2", "attn_ln": "self_attn_layer_norm",
            "cross_attn_ln": "encoder_attn_layer_norm", "mlp_ln": "final_layer_norm"}


def hf_config(d):
    from transformers import WhisperConfig

    return WhisperConfig(vocab_size=d.n_vocab, d_model=d.n_text_state, decoder_layers=d.n_text_layer, decoder_attention_heads=d.n_text_head,
                         decoder_ffn_dim=4 * d.n_text_state, max_target_positions=d.n_text_ctx, max_source_positions=d.n_audio_ctx, encoder_layers=1,
                         encoder_attention_heads=d.n_text_head, encoder_ffn_dim=8, activation_function="gelu", dropout=0.0, attention_dropout=0.0,
                         activation_dropout=0.0, decoder_layerdrop=0.0, scale_embedding=False, pad_token_id=0, bos_token_id=0, eos_token_id=0, decoder_start_token_id=0, attn_implementation="eager")


def hf_state_dict(d, w):
    import torch

    t = lambda k: torch.from_numpy(np.ascontiguousarray(w[k]))  # noqa: E731
    sd = {"embed_tokens.weight": t("decoder.token_embedding.weight"), "embed_positions.weight": t("decoder.positional_embedding"),
          "layer_norm.weight": t("decoder.ln.weight"), "layer_norm.bias": t("decoder.ln.bias")}
    for i in range(d.n_text_layer):
        for ours, theirs in HF_NAMES.items():
            for part in ("weight", "bias"):
                k = f"decoder.blocks.{i}.{ours}.{part}"
                if k in w:
                    sd[f"layers.{i}.{theirs}.{part}"] = t(k)
    return sd


def hf_decoder(d, w):
    """transformers' WhisperDecoder (fp32, CPU, eval, eager attention) carrying the MLX-named weights `w`"""
    from transformers.models.whisper.modeling_whisper import WhisperDecoder

    dec = WhisperDecoder(hf_config(d)).eval()
    missing, unexpected = dec.load_state_dict(hf_state_dict(d, w), strict=False)
    assert not unexpected and all(m.endswith("k_proj.bias") for m in missing), (missing, unexpected)
    return dec


def hf_logits(dec, tokens, feats, bf16=False):
    """tokens (B, S) ints, feats (B, ctx, D) float32 numpy -> logits (B, S, V) float32 numpy = hidden @ embed_tokens.T; bf16: the module converted
    with .bfloat16() and run on the CPU (the yardstick of what bf16 arithmetic costs)"""
    import copy

    import torch

    ids = torch.from_numpy(np.ascontiguousarray(tokens)).long()
    xa = torch.from_numpy(np.ascontiguousarray(feats))
    with torch.no_grad():
        if bf16:
            m = copy.deepcopy(dec).bfloat16()
            h = m(input_ids=ids, encoder_hidden_states=xa.bfloat16(), use_cache=False).last_hidden_state
            return (h @ m.embed_tokens.weight.T).float().numpy()
        h = dec(input_ids=ids, encoder_hidden_states=xa, use_cache=False).last_hidden_state
        return (h @ dec.embed_tokens.weight.T).numpy()


def features(d, B, seed):
    """encoder-like features: unit-variance rows (the encoder ends in a LayerNorm)"""
    g = np.random.default_rng(seed)
    return g.standard_normal((B, d.n_audio_ctx, d.n_audio_state)).astype(np.float32)


# ---- the filters and the greedy update ------------------------------------------------------------------------------------------------------
def pick_params(tok, n_vocab, *, without_timestamps=False, suppress_blank=True, max_initial_timestamp_index=None):
    return dict(n_vocab=n_vocab, eot=tok.eot, blank=220, no_timestamps=tok.no_timestamps, timestamp_begin=tok.timestamp_begin,
                max_initial_timestamp_index=-1 if max_initial_timestamp_index is None else max_initial_timestamp_index,
                without_timestamps=int(without_timestamps), suppress_blank=int(suppress_blank))


def filter_logits(logits, sampled, P, suppress=(), mass_on="masked"):
    """The filters of decoding.py:302-395 in their order on ONE row: logits (V,), sampled = the tokens sampled so far (tokens[sample_begin:]).
    -> float64 (V,) with -inf at masked ids.

    SuppressBlank: " " and eot at the first sampled position.  SuppressTokens: the given ids.  ApplyTimestampRules (unless without_timestamps):
    <|notimestamps|>; after a timestamp, another timestamp is forbidden if the one before was a timestamp too (or absent), else text below eot is
    forbidden; timestamps below the last timestamp SEEN are forbidden (equal ones too unless a pair is being closed); at the first position only
    timestamps up to max_initial_timestamp_index; and if the timestamps' total probability exceeds the best text token's, text is forbidden.

    Two places where the reference's text differs from OpenAI's original and from transformers, which agree with each other; both are restated
    in the original's form.  (1) The non-decreasing rule: the reference's lines 359-368 collect the POSITIONS of the timestamps in `seq` where the
    original collects their token VALUES, so its slice timestamp_begin:last_timestamp is always empty and the rule never fires; what its comment
    states ("forbid timestamp tokens smaller than the last") is what is restated.  (2) The probability-mass rule: the reference takes both sides
    from the logits the filter was HANDED (lines 383-389, mass_on="handed"), the original after the masks above (mass_on="masked", the default and
    what the kernel does).  Handed, a row that must not emit a timestamp (one timestamp so far) but whose timestamps outweigh the best text token
    loses EVERY token and its arg-maximum is taken over NaNs; masked, forbidden timestamps carry no weight and that cannot happen."""
    x = np.asarray(logits, np.float64).copy()
    n, tb, eot = len(sampled), P["timestamp_begin"], P["eot"]
    if P["suppress_blank"] and n == 0:
        x[[P["blank"], eot]] = NEG
    if len(suppress):
        x[list(suppress)] = NEG
    if P["without_timestamps"]:
        return x
    handed = x.copy()
    x[P["no_timestamps"]] = NEG
    last_ts = n >= 1 and sampled[-1] >= tb
    pen_ts = n < 2 or sampled[-2] >= tb
    if last_ts:
        if pen_ts:
            x[tb:] = NEG
        else:
            x[:eot] = NEG
    seen = [t for t in sampled if t >= tb]
    if seen:
        x[tb:(seen[-1] if last_ts and not pen_ts else seen[-1] + 1)] = NEG
    if n == 0:
        x[:tb] = NEG
        if P["max_initial_timestamp_index"] >= 0:
            x[tb + P["max_initial_timestamp_index"] + 1:] = NEG
    src = handed if mass_on == "handed" else x
    if logsumexp(src[tb:]) > src[:tb].max():
        x[:tb] = NEG
    return x


def logsumexp(v):
    v = np.asarray(v, np.float64)
    m = v.max()
    return NEG if m == NEG else m + math.log(np.exp(v - m).sum())


class GreedyRow:
    """GreedyDecoder.update (decoding.py:260-278) for one row at temperature 0"""

    def __init__(self, eot):
        self.eot, self.sampled, self.sum_logprob, self.ended = eot, [], 0.0, False

    def update(self, filtered):
        t = int(np.argmax(filtered))  # numpy returns the lowest index of the maximum
        lp = float(filtered[t] - logsumexp(filtered))
        if self.ended:
            t = self.eot
        else:
            self.sum_logprob += lp
        self.sampled.append(t)
        self.ended = self.ended or t == self.eot
        return t


# ---- kernel references ------------------------------------------------------------------------------------------------------------------------
def attn_row(q, k, v):
    """float64 softmax(q k^T / 8) v of one query: q (64,), k, v (len, 64)"""
    s = k.astype(np.float64) @ q.astype(np.float64) / 8.0
    p = np.exp(s - s.max())
    return (p / p.sum()) @ v.astype(np.float64)


def gelu(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
