"""Quantised CSM checkpoints on the host, no GPU: the quantised fragment pack (kk_csm_qfrag_pack / kk_csm_qfrag_bytes) against a numpy restatement
of its layout; the decode rule  bf16_rne(fp32(q) * scale + bias)  (fp32 multiply, then fp32 add) applied to that pack against the bf16 fragment
pack (kk_csm_frag_pack) of `dequantize_affine`'s matrix, bit for bit; which tensors of a CSM checkpoint are quantised and how the loader routes
the triplets; the pack sizes of every Linear of CSM-1B."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import mlx_audio_amd.params as P
from mlx_audio_amd import _lib, quant


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def seed(*parts):
    return zlib.crc32(repr(parts).encode())


def bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def qfrag_bytes(lib, K, N, nsub, group, bits):
    qb, pb = C.c_size_t(0), C.c_size_t(0)
    assert lib.kk_csm_qfrag_bytes(K, N, nsub, group, bits, C.byref(qb), C.byref(pb)) == 0, lib.kk_last_error()
    return qb.value, pb.value


def qfrag_pack(lib, words, scales, biases, K, N, nsub, group, bits):
    qb, pb = qfrag_bytes(lib, K, N, nsub, group, bits)
    q = np.full(qb, 0xAB, np.uint8)  # (every byte must be written, padding included)
    pairs = np.full(pb // 4, np.float32(-7.5), np.float32)
    words, scales, biases = (np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(scales, np.float32), np.ascontiguousarray(biases, np.float32))
    rc = lib.kk_csm_qfrag_pack(words.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p), biases.ctypes.data_as(C.c_void_p), K, N, nsub, group,
                               bits, q.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.kk_last_error()
    return q, pairs


def frag_pack(lib, w, nsub):
    K, N = w.shape
    w = np.ascontiguousarray(w, np.float32)
    out = np.zeros(-(-N // (16 * nsub)) * 16 * nsub * K, np.uint16)
    assert lib.kk_csm_frag_pack(w.ctypes.data_as(C.c_void_p), K, N, nsub, out.ctypes.data_as(C.c_void_p)) == 0, lib.kk_last_error()
    return out


def unpack_q(words, bits):
    """[N][K bits / 32] uint32 -> [N][K] integers (value j of a word in bits [j bits, (j + 1) bits))"""
    per = 32 // bits
    q = np.empty((words.shape[0], words.shape[1] * per), np.uint32)
    for j in range(per):
        q[:, j::per] = (words >> np.uint32(j * bits)) & np.uint32(2**bits - 1)
    return q


def qfrag_ref(words, scales, biases, K, N, nsub, group, bits):
    """The layout, restated: integers [block][K / 32][nsub][64 lanes][8 values] (lane L of chunk c, sub-block s: k = 32 c + 8 (L / 16) + j, column
    16 s + L % 16), one byte per value (8-bit) or two values per byte, the even one in the low nibble (4-bit); pairs [block][K / group][nsub][16
    columns][scale, bias]; padding columns all zero."""
    cb = 16 * nsub
    nblk = -(-N // cb)
    qp = np.zeros((K, nblk * cb), np.uint8)
    qp[:, :N] = unpack_q(words, bits).T
    t = qp.reshape(K // 32, 4, 8, nblk, nsub, 16).transpose(3, 0, 4, 1, 5, 2).reshape(-1, 8)  # [blk][c][s][q][l] x j
    qb = t if bits == 8 else (t[:, 0::2] | (t[:, 1::2] << 4))
    G = K // group
    pr = np.zeros((G, nblk * cb, 2), np.float32)
    pr[:, :N, 0], pr[:, :N, 1] = scales.T, biases.T
    pr = pr.reshape(G, nblk, nsub, 16, 2).transpose(1, 0, 2, 3, 4)
    return np.ascontiguousarray(qb).reshape(-1), np.ascontiguousarray(pr).reshape(-1)


def decode_ref(q, pairs, K, N, nsub, group, bits):
    """The kernels' decode of a quantised pack, in numpy float32: value -> fp32, times the lane's scale (rounded to fp32), plus its bias (rounded to
    fp32), then bf16 round-to-nearest-even.  Returns the uint16 bits in bf16-fragment-pack order [block][chunk][sub][lane][8]."""
    cb = 16 * nsub
    nblk, nch, G = -(-N // cb), K // 32, K // group
    v = q.reshape(-1, 8) if bits == 8 else np.stack([(q >> 0) & 15, (q >> 4) & 15], -1).reshape(-1, 8)
    v = v.reshape(nblk, nch, nsub, 4, 16, 8).astype(np.float32)
    pr = pairs.reshape(nblk, G, nsub, 16, 2)
    g_of_c = (np.arange(nch) * 32) // group
    s = pr[..., 0][:, g_of_c][:, :, :, None, :, None]  # [blk][c][s][1][l][1]
    b = pr[..., 1][:, g_of_c][:, :, :, None, :, None]
    prod = (v * s).astype(np.float32)
    return bf16_bits((prod + b).astype(np.float32)).reshape(-1)


def make_triplet(rng, N, K, group, bits, scale_dtype):
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    words, scales, biases = quant.quantize_affine(w, group, bits)
    if scale_dtype == "bf16":
        scales, biases = (torch.from_numpy(a).to(torch.bfloat16).float().numpy() for a in (scales, biases))
    elif scale_dtype == "fp16":
        scales, biases = (a.astype(np.float16).astype(np.float32) for a in (scales, biases))
    return words, scales, biases


@pytest.mark.parametrize("N", [16, 48, 2051])
@pytest.mark.parametrize("nsub", [1, 2, 4])
@pytest.mark.parametrize("group", [32, 64, 128])
@pytest.mark.parametrize("bits", [4, 8])
def test_qfrag_pack_layout_matches_numpy(lib, bits, group, nsub, N):
    rng = np.random.default_rng(seed("layout", bits, group, nsub, N))
    K = 256
    words, scales, biases = make_triplet(rng, N, K, group, bits, "fp32")
    q, pairs = qfrag_pack(lib, words, scales, biases, K, N, nsub, group, bits)
    rq, rp = qfrag_ref(words, scales, biases, K, N, nsub, group, bits)
    np.testing.assert_array_equal(q, rq)
    np.testing.assert_array_equal(pairs.view(np.uint32), rp.view(np.uint32))
    # the rule itself at single elements, independent of the reshape above
    cb, nch, G = 16 * nsub, K // 32, K // group
    qv = unpack_q(words, bits)
    for k, n in [(0, 0), (37, N - 1), (255, N // 2), (8, min(N - 1, 17))]:
        blk, s, c, L, j = n // cb, (n % cb) // 16, k // 32, 16 * ((k % 32) // 8) + n % 16, k % 8
        lane = ((blk * nch + c) * nsub + s) * 64 + L
        got = q[lane * 8 + j] if bits == 8 else (q[lane * 4 + j // 2] >> (4 * (j % 2))) & 15
        assert got == qv[n, k]
        at = (((blk * G + k // group) * nsub + s) * 16 + n % 16) * 2
        assert pairs[at] == scales[n, k // group] and pairs[at + 1] == biases[n, k // group]
    # padding columns decode to +0
    dec = decode_ref(q, pairs, K, N, nsub, group, bits).reshape(-(-N // cb), nch, nsub, 4, 16, 8)
    npad = -(-N // cb) * cb - N
    if npad:
        cols = np.arange(N, N + npad)
        assert not dec[cols // cb, :, (cols % cb) // 16, :, cols % 16].any()


@pytest.mark.parametrize("scale_dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("bits,group,nsub,N", [(8, 64, 1, 48), (4, 64, 4, 2051), (4, 32, 2, 100), (8, 128, 2, 16), (8, 32, 4, 130), (4, 128, 1, 2051)])
def test_decoded_qfrag_equals_the_bf16_pack_of_the_dequantised_matrix(lib, scale_dtype, bits, group, nsub, N):
    rng = np.random.default_rng(seed("decode", scale_dtype, bits, group, nsub, N))
    K = 384
    words, scales, biases = make_triplet(rng, N, K, group, bits, scale_dtype)
    q, pairs = qfrag_pack(lib, words, scales, biases, K, N, nsub, group, bits)
    w = quant.dequantize_affine(words, scales, biases, group, bits)  # [N][K]
    np.testing.assert_array_equal(decode_ref(q, pairs, K, N, nsub, group, bits), frag_pack(lib, w.T, nsub))


def fma_sensitive_triplet(rng, N, K, group, bits):
    """fp32 scales / biases with full mantissas on which fma(q, s, b) and (q * s rounded to fp32) + b give DIFFERENT bf16 values wherever q = 3:
    s = 1 + 2^-23, so 3 s = 3 + 3 * 2^-23 is a tie of the fp32 grid at 3 (spacing 2^-22) and rounds to 3 + 2^-21; with
    b = (1 + 3 * 2^-8) - (3 + 2^-21) (exact in fp32) the two-step sum is exactly 1 + 3 * 2^-8, a tie of the bf16 grid that rounds to the even
    1 + 2^-6, while the exact sum is 2^-23 below the tie and rounds to 1 + 2^-7."""
    q = rng.integers(0, 2**bits, (N, K)).astype(np.uint32)
    q[:, ::5] = 3
    per = 32 // bits
    words = np.zeros((N, K // per), np.uint32)
    for j in range(per):
        words |= q[:, j::per] << np.uint32(j * bits)
    s = np.float32(1.0) + np.float32(2.0**-23)
    b = np.float32((1 + 3 * 2.0**-8) - (3 + 2.0**-21))
    assert float(b) == (1 + 3 * 2.0**-8) - (3 + 2.0**-21)
    return words, np.full((N, K // group), s, np.float32), np.full((N, K // group), b, np.float32)


def test_mul_then_add_differs_from_fma_with_full_mantissa_scales():
    rng = np.random.default_rng(seed("fma"))
    N, K, group, bits = 64, 256, 64, 8
    words, scales, biases = fma_sensitive_triplet(rng, N, K, group, bits)
    q = unpack_q(words, bits).astype(np.float64)
    s, b = np.repeat(scales, group, 1).astype(np.float64), np.repeat(biases, group, 1).astype(np.float64)
    fma = bf16_bits((q * s + b).astype(np.float32))  # one rounding to fp32 (the product of a <= 8-bit and a 24-bit number is exact in float64)
    two = bf16_bits(quant.dequantize_affine(words, scales, biases, group, bits))
    assert (fma != two)[q == 3].all() and (fma != two).mean() >= 0.2


# ------------------------------------------------------------------------------------------------------------- predicate / routing
def torchtune(k):
    k = k.replace("self_attn.o_proj", "attn.output_proj").replace("self_attn", "attn")
    k = k.replace("gate_proj", "w1").replace("down_proj", "w2").replace("up_proj", "w3")
    k = k.replace("input_layernorm.weight", "sa_norm.scale").replace("post_attention_layernorm.weight", "mlp_norm.scale")
    return k.replace("backbone.norm.weight", "backbone.norm.scale").replace("decoder.norm.weight", "decoder.norm.scale")


def tiny_quantised(bits=8, group=64, seed_=0):
    cfg = P.csm_tiny_config()
    w = P.csm_synth_checkpoint(cfg, seed_)
    w["_audio_tokenizer.decoder_transformer.layers.0.linear1.weight"] = np.ones((64, 64), np.float32)
    names = quant.csm_quantised_layer_names(w, group)
    return cfg, w, names, quant.quantize_checkpoint(w, group, bits, names=names)


def test_csm_predicate_picks_linears_and_embeddings_only():
    cfg, w, names, qw = tiny_quantised()
    inv = P.csm_param_inventory(cfg)
    want = {k for k, shp in inv.items() if len(shp) == 2}  # every Linear and both embedding tables; norms are 1-D, audio_head 3-D and unsuffixed
    assert set(names) == want and "audio_head" not in names and "text_embeddings.weight" in names
    assert all(not n.startswith("_audio_tokenizer") for n in names)
    for k in names:
        p = k[: -len(".weight")]
        assert qw[k].dtype == np.uint32 and p + ".scales" in qw and p + ".biases" in qw
    assert qw["audio_head"] is w["audio_head"] and qw["_audio_tokenizer.decoder_transformer.layers.0.linear1.weight"].dtype == np.float32
    # `model.`-prefixed names: the same set
    pref = {"model." + k: v for k, v in w.items()}
    assert set(quant.csm_quantised_layer_names(pref, 64)) == {"model." + k for k in names}
    # a width the group does not divide is left alone
    odd = dict(w, **{"projection.weight": np.ones((256, 96), np.float32)})
    assert "projection.weight" not in quant.csm_quantised_layer_names(odd, 64)


@pytest.mark.parametrize("naming", ["torchtune", "mlx_prefixed"])
def test_loader_routes_triplets_after_sanitize(monkeypatch, naming):
    """sesame.Model.load_weights renames all three keys of a quantised layer together, keeps the words as uint32 bit patterns, hands the per-layer
    overrides on under the renamed paths, and leaves `audio_head` and the codec's tensors alone."""
    from mlx_audio_amd import sesame

    cfg, w, names, qw = tiny_quantised()
    seen = {}

    class Fake:
        def __init__(self, cfg_, weights, weight_dtype="float32", quantization=None, weight_storage="packed"):
            seen.update(weights=weights, quantization=quantization, storage=weight_storage)

    class FakeMimi:
        pass

    monkeypatch.setattr(sesame, "SesameModel", Fake)
    ren = torchtune if naming == "torchtune" else (lambda k: "model." + k)
    ck = {ren(k): (torch.from_numpy(v.view(np.int32)).view(torch.uint32) if v.dtype == np.uint32 else torch.from_numpy(np.ascontiguousarray(v)))
          for k, v in qw.items()}
    layer = "backbone.layers.1.self_attn.k_proj"
    qcfg = {"group_size": 64, "bits": 8, ren(layer + ".weight")[: -len(".weight")]: {"group_size": 32, "bits": 4},
            ren("decoder.layers.0.mlp.up_proj.weight")[: -len(".weight")]: False}
    sesame.Model(dict(cfg, quantization=qcfg), mimi=FakeMimi()).load_weights(ck)
    got = seen["weights"]
    assert set(got) == {k for k in qw if not k.startswith("_audio_tokenizer.")}
    assert seen["quantization"][layer] == {"group_size": 32, "bits": 4} and seen["quantization"]["decoder.layers.0.mlp.up_proj"] is False
    for k in names:
        if k != "decoder.layers.0.mlp.up_proj.weight":
            assert got[k].dtype == np.uint32
            np.testing.assert_array_equal(got[k], qw[k])
    assert got["audio_head"].dtype == np.float32 and got["backbone.norm.weight"].dtype == np.float32
    plain, trip = quant.split_triplets(got, 64, 8, {k: v for k, v in seen["quantization"].items() if k not in ("group_size", "bits")})
    assert set(trip) == set(names) - {"decoder.layers.0.mlp.up_proj.weight"}
    assert trip[layer + ".weight"][3:] == (32, 4) and trip["projection.weight"][3:] == (64, 8)
    assert "audio_head" in plain and "decoder.layers.0.mlp.up_proj.weight" in plain and "decoder.layers.0.mlp.up_proj.scales" in plain
    assert not any(k.endswith((".scales", ".biases")) for k in plain if not k.startswith("decoder.layers.0.mlp.up_proj"))


@pytest.mark.parametrize("bits", [3, 6])
def test_bits_outside_the_word_layout_raise(bits):
    cfg, w, names, qw = tiny_quantised()
    with pytest.raises(ValueError, match="word"):
        quant.split_triplets(qw, 64, bits)
    with pytest.raises(ValueError, match="word"):
        quant.dequantize_checkpoint(qw, 64, bits)
    assert quant.check_bits(2) == 2


def test_dequantize_round_trips_two_bits():
    rng = np.random.default_rng(seed("two"))
    w = rng.standard_normal((8, 128)).astype(np.float32)
    words, s, b = quant.quantize_affine(w, 64, 2)
    back = quant.dequantize_affine(words, s, b, 64, 2)
    assert np.all(np.abs(back - w) <= 0.5 * np.repeat(s, 64, 1) + 1e-6)


# ------------------------------------------------------------------------------------------------------------- sizes
def _linears(cfg):
    out = []
    for stack in ("backbone", "decoder"):
        a = cfg[stack]
        H, KV, hd, D, I = a["num_heads"], a["num_kv_heads"], a["head_dim"], a["hidden"], a["intermediate"]
        out += [(f"{stack}.qkv", D, (H + 2 * KV) * hd, False), (f"{stack}.o", H * hd, D, False), (f"{stack}.gate_up", D, 2 * I, False),
                (f"{stack}.down", I, D, True)]
    D, Dd, V = cfg["backbone"]["hidden"], cfg["decoder"]["hidden"], cfg["audio_vocab_size"]
    return out + [("projection", D, Dd, False), ("codebook0_head", D, V, False), ("audio_head", Dd, V, False)]


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("group", [32, 64, 128])
def test_qfrag_bytes_of_every_csm_1b_linear(lib, bits, group):
    for name, K, N, split_ok in _linears(P.csm_config()):
        ks, nsub = C.c_int32(-1), C.c_int32(-1)
        assert lib.kk_csm_frag_choice(K, N, int(split_ok), C.byref(ks), C.byref(nsub)) == 0
        npad = -(-N // (16 * nsub.value)) * 16 * nsub.value
        assert qfrag_bytes(lib, K, N, nsub.value, group, bits) == (K * npad * bits // 8, npad * (K // group) * 8), name


def test_qfrag_entry_points_refuse_what_the_kernels_cannot_decode(lib):
    qb, pb = C.c_size_t(0), C.c_size_t(0)
    for K, N, nsub, group, bits in [(256, 16, 1, 48, 8), (256, 16, 1, 64, 2), (256, 16, 3, 64, 8), (96, 16, 1, 64, 8), (256, 0, 1, 64, 4), (256, 16, 1, 16, 4)]:
        assert lib.kk_csm_qfrag_bytes(K, N, nsub, group, bits, C.byref(qb), C.byref(pb)) != 0, (K, N, nsub, group, bits)
