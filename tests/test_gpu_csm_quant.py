"""Quantised CSM checkpoints on the GPU: packed 4- / 8-bit weights decoded inside the matrix-core kernels must give THE BITS of bf16 weight mode on
the dequantised checkpoint -- kernel level (kk_op_csm_gemv_q / kk_op_csm_gemm_prompt_q against kk_op_csm_gemv / kk_op_csm_gemm_prompt on the bf16
fragment pack of `dequantize_affine`'s matrix) and model level (logits and codes) --, load_model on a written quantised checkpoint, the
fallbacks to host dequantisation, and the device bytes held."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import mlx_audio_amd.params as P  # noqa: E402
from _util import err_stats, report  # noqa: E402
from mlx_audio_amd import quant  # noqa: E402
from test_csm_quant_cpu import bf16_bits, fma_sensitive_triplet, frag_pack, qfrag_pack, unpack_q  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def seed(*parts):
    return zlib.crc32(repr(parts).encode())


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def Pn(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def frag_choice(lib, K, N, split_ok):
    ks, nsub = C.c_int32(-1), C.c_int32(-1)
    assert lib.kk_csm_frag_choice(K, N, int(split_ok), C.byref(ks), C.byref(nsub)) == 0
    return ks.value, nsub.value


class Packs:
    """One nn.Linear [N][K] quantised at (bits, group): its quantised fragment pack + pairs, and the bf16 fragment pack of the dequantised matrix,
    both on the device, in the (ks, nsub) the generator picks."""

    def __init__(self, lib, K, N, bits, group, split_ok, triplet=None, scale_dtype="bf16"):
        rng = np.random.default_rng(seed("packs", K, N, bits, group))
        self.K, self.N, self.bits, self.group = K, N, bits, group
        self.ks, self.nsub = frag_choice(lib, K, N, split_ok)
        assert self.nsub
        if triplet is None:
            w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
            words, s, b = quant.quantize_affine(w, group, bits)
            if scale_dtype == "bf16":
                s, b = (torch.from_numpy(a).to(torch.bfloat16).float().numpy() for a in (s, b))
            triplet = (words, s, b)
        q, pairs = qfrag_pack(lib, *triplet, K, N, self.nsub, group, bits)
        self.q, self.pairs = torch.from_numpy(q).cuda(), torch.from_numpy(pairs).cuda()
        self.wdq = quant.dequantize_affine(*triplet, group, bits)  # [N][K]
        self.wf = torch.from_numpy(frag_pack(lib, self.wdq.T, self.nsub).view(np.int16)).cuda()


def gemv_pair(lib, pk, M, pro, epi, rng):
    """the same launch on the quantised pack and on the bf16 pack of the dequantised matrix -> (got, want) as uint32 bit patterns"""
    K, N, ks, nsub = pk.K, pk.N, pk.ks, pk.nsub
    x = rng.standard_normal((M, 2 * K if pro == 2 else K)).astype(np.float32)
    if pro == 2:
        x[:, :K] *= 3
    nw = dev(rng.uniform(0.5, 1.5, K)) if pro == 1 else None
    codes = emb = None
    rows, V, cb, cstride = 1, 0, 0, 1
    if pro == 3:
        rows = 2 if M % 2 == 0 else 1
        V, cb, cstride = 11, 1, 3
        codes = dev(rng.integers(0, V, (M // rows, cstride)).astype(np.int32), torch.int32)
        emb = dev(rng.standard_normal((3 * V, K)).astype(np.float32))
        x = x[: M // rows]
    xd = dev(x)
    res0 = rng.standard_normal((M, N)).astype(np.float32)
    outs = []
    for q in (True, False):
        out = dev(res0) if epi else torch.full((M, N), 7.0, device="cuda")
        part = torch.full((ks, M, N), 3.0, device="cuda") if ks > 1 else None
        r = out if epi == 1 else None
        tail = (Pn(xd), x.shape[1], Pn(nw), 1e-5, Pn(codes), cstride, cb, V, rows, Pn(emb), None, Pn(r), N, Pn(out), N, Pn(part))
        if q:
            rc = lib.kk_op_csm_gemv_q(stream(), pro, epi, ks, nsub, K, N, M, Pn(pk.q), Pn(pk.pairs), pk.group, pk.bits, *tail)
        else:
            rc = lib.kk_op_csm_gemv(stream(), pro, epi, ks, nsub, K, N, M, Pn(pk.wf), *tail)
        assert rc == 0, lib.kk_last_error()
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().view(np.uint32))
    return outs


def gemm_pair(lib, pk, M, with_res, rng):
    K, N = pk.K, pk.N
    xd = dev(rng.standard_normal((M, K)).astype(np.float32))
    res = dev(rng.standard_normal((M, N)).astype(np.float32)) if with_res else None
    outs = []
    for q in (True, False):
        out = torch.full((M, N), 7.0, device="cuda")
        if q:
            rc = lib.kk_op_csm_gemm_prompt_q(stream(), K, N, M, pk.nsub, Pn(pk.q), Pn(pk.pairs), pk.group, pk.bits, Pn(xd), K, Pn(res), N, Pn(out), N)
        else:
            rc = lib.kk_op_csm_gemm_prompt(stream(), K, N, M, pk.nsub, Pn(pk.wf), Pn(xd), K, Pn(res), N, Pn(out), N)
        assert rc == 0, lib.kk_last_error()
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().view(np.uint32))
    return outs


ALL6 = [(b, g) for b in (4, 8) for g in (32, 64, 128)]
# K = 1024 / 2048 / 2240: one / two / three straight-line rounds; K = 8192: 8 split-K slices (the down projections); N = 3072 (nsub 1), 16384 (nsub 4),
# 2051 (a partly filled last block); every (bits, group) that divides K on the small matrices, two or three of them on the large ones
MATRICES = [(1024, 3072, ALL6), (2048, 2051, ALL6), (2240, 3072, [(8, 32), (4, 64), (8, 64), (4, 32)]), (2240, 2051, [(4, 32), (8, 64)]),
            (1024, 16384, [(4, 64), (8, 128)]), (2048, 16384, [(8, 64), (4, 32)]), (1024, 2051, [(4, 128), (8, 32)]), (2048, 3072, [(4, 64), (8, 128)]),
            (8192, 3072, [(8, 64), (4, 128), (4, 32)]), (8192, 2051, [(4, 64), (8, 32)])]
CASES = [(K, N, b, g) for K, N, bg in MATRICES for b, g in bg]
FORMS = [(1, 0), (0, 1), (2, 1), (3, 0), (0, 0)]  # (PRO, EPI) of q|k|v / gate|up / audio heads, o, down, projection, codebook0 head; (2, 2): split-K down


@pytest.mark.parametrize("K,N,bits,group", CASES)
def test_gemv_q_and_gemm_prompt_q_bitexact_vs_bf16_pack_of_dequantised(lib, K, N, bits, group):
    split = K >= 4096
    pk = Packs(lib, K, N, bits, group, split)
    assert (pk.ks > 1) == split
    rng = np.random.default_rng(seed("x", K, N, bits, group))
    for pro, epi in ([(2, 2)] if split else FORMS):
        for M in (1, 8, 17):
            got, want = gemv_pair(lib, pk, M, pro, epi, rng)
            np.testing.assert_array_equal(got, want, err_msg=f"gemv pro {pro} epi {epi} M {M}")
    for M, with_res in ((5, False), (64, True), (190 * 8, False)):
        got, want = gemm_pair(lib, pk, M, with_res, rng)
        np.testing.assert_array_equal(got, want, err_msg=f"gemm_prompt M {M}")
    report(f"csm_quant/kernels/K{K}_N{N}_q{bits}_g{group}", bitexact=True, ks=pk.ks, nsub=pk.nsub)


@pytest.mark.parametrize("bits", [4, 8])
def test_device_decode_does_not_contract_multiply_and_add(lib, bits):
    """fp32 scales / biases on which fma(q, s, b) and fl(q s) + b differ in the bf16 value (asserted here on the CPU): the device must give the
    two-rounding result, i.e. the bf16 pack of dequantize_affine's matrix."""
    rng = np.random.default_rng(seed("fma", bits))
    K, N, group = 1024, 48, 64
    trip = fma_sensitive_triplet(rng, N, K, group, bits)
    q = unpack_q(trip[0], bits).astype(np.float64)
    fma = bf16_bits((q * np.float64(trip[1][0, 0]) + np.float64(trip[2][0, 0])).astype(np.float32))
    assert (fma != bf16_bits(quant.dequantize_affine(*trip, group, bits)))[q == 3].all()
    pk = Packs(lib, K, N, bits, group, False, triplet=trip)
    for pro, epi in ((0, 0), (1, 0)):
        got, want = gemv_pair(lib, pk, 8, pro, epi, rng)
        np.testing.assert_array_equal(got, want)
    got, want = gemm_pair(lib, pk, 70, False, rng)
    np.testing.assert_array_equal(got, want)
    # and the contracted decode would NOT have passed: the same launch on the bf16 pack of the fma matrix gives other bits
    wf_fma = (q * np.float64(trip[1][0, 0]) + np.float64(trip[2][0, 0])).astype(np.float32)
    pk.wf = torch.from_numpy(frag_pack(lib, wf_fma.T, pk.nsub).view(np.int16)).cuda()
    got, other = gemv_pair(lib, pk, 8, 0, 0, rng)
    assert (got != other).any()


# ------------------------------------------------------------------------------------------------------------- model level
def quantised_tiny(bits, group, seed_=0, cfg=None, scales="bf16", per_layer=None):
    """(cfg, quantised checkpoint, config["quantization"], dequantised checkpoint)"""
    cfg = cfg or P.csm_tiny_config()
    w = P.csm_synth_checkpoint(cfg, seed_)
    names = quant.csm_quantised_layer_names(w, group)
    qw = quant.quantize_checkpoint(w, group, bits, names=names)
    per_layer = per_layer or {}
    for p, own in per_layer.items():
        words, s, b = quant.quantize_affine(w[p + ".weight"], own["group_size"], own["bits"])
        qw[p + ".weight"], qw[p + ".scales"], qw[p + ".biases"] = words, s, b
    if scales == "bf16":  # what real MLX checkpoints hold
        for k in list(qw):
            if k.endswith((".scales", ".biases")):
                qw[k] = torch.from_numpy(qw[k]).to(torch.bfloat16).float().numpy()
    qcfg = dict({"group_size": group, "bits": bits}, **per_layer)
    return cfg, qw, qcfg, quant.dequantize_checkpoint(qw, group, bits, per_layer)


def ragged_prompt(cfg, rng, lens):
    n, B, S = cfg["audio_num_codebooks"], len(lens), max(lens)
    tok = np.zeros((B, S, n + 1), np.int64)
    msk = np.zeros((B, S, n + 1), np.float32)
    for b, L in enumerate(lens):
        nt = max(1, L // 2)
        tok[b, S - L : S - L + nt, -1] = rng.integers(0, cfg["text_vocab_size"], nt)
        msk[b, S - L : S - L + nt, -1] = 1
        tok[b, S - L + nt :, :n] = rng.integers(0, cfg["audio_vocab_size"], (L - nt, n))
        msk[b, S - L + nt :, :n] = 1
    return tok, msk, [S - L for L in lens]


def run_frames(model, cfg, tok, msk, pads, us, graph, frames=5):
    """prompt block + `frames` single-token frames (odd ones sampled on injected uniforms) -> codes [1 + frames][B][n], logits as uint32 bits"""
    n, B = cfg["audio_num_codebooks"], tok.shape[0]
    if model.max_batch < B:
        model.setup_caches(B)
    model.reset_caches()
    model.set_graph_mode(graph)
    model.set_padding(pads)
    codes = [model.generate_frame(torch.tensor(tok), torch.tensor(msk)).clone()]
    logits = [model.debug_logits().clone()]
    for i in range(frames):
        t_in = torch.zeros((B, 1, n + 1), dtype=torch.int32, device="cuda")
        t_in[:, 0, :n] = codes[-1]
        m_in = torch.zeros((B, 1, n + 1), dtype=torch.float32, device="cuda")
        m_in[:, 0, :n] = 1
        temp, u = (0.9, torch.tensor(us[i])) if i % 2 else (0.0, None)
        codes.append(model.generate_frame(t_in, m_in, temperature=temp, top_k=10, uniforms=u).clone())
        logits.append(model.debug_logits().clone())
    torch.cuda.synchronize()
    return torch.stack(codes).cpu().numpy(), torch.stack(logits).cpu().numpy().view(np.uint32)


def assert_same_frames(name, a, b):
    np.testing.assert_array_equal(a[1], b[1], err_msg=name + ": logits")
    np.testing.assert_array_equal(a[0], b[0], err_msg=name + ": codes")


@pytest.mark.parametrize("bits,group,scales", [(8, 64, "bf16"), (4, 64, "bf16"), (4, 32, "fp32")])
def test_packed_model_gives_the_bits_of_bf16_mode_on_the_dequantised_checkpoint(bits, group, scales):
    from mlx_audio_amd.csm import SesameModel

    cfg, qw, qcfg, dq = quantised_tiny(bits, group, seed("model", bits, group) % 1000, scales=scales)
    packed = SesameModel(cfg, qw, quantization=qcfg)
    assert packed.weight_format == f"q{bits}" and packed.weight_fallback is None
    ref = SesameModel(cfg, dq, weight_dtype="bfloat16")
    assert ref.weight_format == "bf16" and ref.weight_fallback is None
    assert packed.weight_bytes["linear"] < ref.weight_bytes["linear"]
    rng = np.random.default_rng(seed("frames", bits, group))
    n = cfg["audio_num_codebooks"]
    for lens in ([9], [12, 7, 12, 5, 9, 12, 3, 10]):  # B = 1; B = 8 with ragged padding
        tok, msk, pads = ragged_prompt(cfg, rng, lens)
        us = rng.uniform(size=(5, len(lens), n)).astype(np.float32)
        want = run_frames(ref, cfg, tok, msk, pads, us, False)
        assert_same_frames(f"B{len(lens)} eager", run_frames(packed, cfg, tok, msk, pads, us, False), want)
        for rep in range(3):  # eager, capture, replay
            got = run_frames(packed, cfg, tok, msk, pads, us, True)
        assert_same_frames(f"B{len(lens)} graph", got, want)
        other = packed.share()
        assert other.weight_format == f"q{bits}"
        assert_same_frames(f"B{len(lens)} shared", run_frames(other, cfg, tok, msk, pads, us, False), want)
        del other
    report(f"csm_quant/model/q{bits}_g{group}_{scales}", bitexact=True, linear_bytes=packed.weight_bytes["linear"], bf16_linear_bytes=ref.weight_bytes["linear"])


@pytest.mark.parametrize("bits,group", [(8, 64), (4, 64), (4, 32)])
def test_packed_model_matches_the_fp32_oracle(bits, group):
    """The bar of test_csm_tiny_frames_match_oracle[bfloat16], unchanged: logits within 2e-4 of their range, every code equal, against the fp32-arithmetic
    CPU oracle.  As there, the oracle multiplies by the matrices the mode holds -- that test feeds a bf16 checkpoint, on which bf16 storage is
    lossless; here they are the dequantised weights with the Linears and the audio heads rounded to bf16 (tables and norms stay fp32, as in the
    engine).  The distance to the oracle on the UNROUNDED dequantised weights is bf16 storage error, not kernel error; it is reported, not asserted
    (measured: 2.8e-3 .. 3.4e-3 of the logits' range -- one bf16 rounding per weight -- against 4e-7 .. 6e-7 for the held weights; where that second
    oracle samples another code inside a frame its later logits of the frame are another sequence's)."""
    import csm_oracle as CO
    from mlx_audio_amd.csm import SesameModel

    cfg, qw, qcfg, dq = quantised_tiny(bits, group, 0)
    as_held = {k: (torch.tensor(v).to(torch.bfloat16).float().numpy() if (v.ndim >= 2 and not k.endswith("embeddings.weight")) else v) for k, v in dq.items()}
    rng = np.random.default_rng(seed("oracle", bits, group))
    B, n = 3, cfg["audio_num_codebooks"]
    tok, msk, pads = ragged_prompt(cfg, rng, [8, 8, 8])
    model = SesameModel(cfg, qw, quantization=qcfg)
    model.setup_caches(B)
    orc, orc_raw = CO.CsmOracle(as_held, cfg), CO.CsmOracle(dq, cfg)
    t_in, m_in = tok, msk
    for step in range(5):
        temp, u = (0.9, rng.uniform(size=(B, n)).astype(np.float32)) if step % 2 else (0.0, None)
        trace, trace_raw = {}, {}
        ref = orc.generate_frame(t_in, m_in, temp=temp, top_k=10, uniforms=u, trace=trace)
        orc_raw.generate_frame(t_in, m_in, temp=temp, top_k=10, uniforms=u, trace=trace_raw)
        got = model.generate_frame(torch.tensor(t_in), torch.tensor(m_in), temperature=temp, top_k=10, uniforms=None if u is None else torch.tensor(u))
        torch.cuda.synchronize()
        lg = model.debug_logits().cpu().numpy()
        e = err_stats(lg, np.stack([trace["c0_logits"]] + trace["ci_logits"], 0))
        e_raw = err_stats(lg, np.stack([trace_raw["c0_logits"]] + trace_raw["ci_logits"], 0))
        report(f"csm_quant/oracle/q{bits}_g{group}/frame{step}/logits", **e)
        report(f"csm_quant/oracle_unrounded_weights/q{bits}_g{group}/frame{step}/logits", **e_raw)
        print(f"q{bits} g{group} frame {step}: rel_max {e['rel_max']:.3e} (oracle on the held weights), {e_raw['rel_max']:.3e} (unrounded dequantised weights)")
        assert e["rel_max"] < 2e-4, (step, e)
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
        t_in = np.zeros((B, 1, n + 1), np.int64)
        t_in[:, 0, :n] = ref
        m_in = np.zeros((B, 1, n + 1), np.float32)
        m_in[:, 0, :n] = 1  # (both oracles continue from the same codes)


def test_load_model_on_a_quantised_sesame_directory(tmp_path):
    """config.json with model_type "sesame" and "quantization", safetensors with uint32 `weight` and bf16 `scales` / `biases` under torchtune-style
    names: load_model returns a packed model whose frames carry the bits of bf16 mode on the dequantised checkpoint."""
    from safetensors.torch import save_file

    from mlx_audio_amd.csm import SesameModel
    from mlx_audio_amd.sesame import Model
    from mlx_audio_amd.utils import load_model
    from test_csm_quant_cpu import torchtune

    cfg, qw, qcfg, dq = quantised_tiny(8, 64, 3)
    d = tmp_path / "csm-tiny-8bit"
    d.mkdir()
    tensors = {}
    for k, v in qw.items():
        if v.dtype == np.uint32:
            t = torch.from_numpy(v.view(np.int32)).view(torch.uint32)
        elif k.endswith((".scales", ".biases")):
            t = torch.from_numpy(v).to(torch.bfloat16)
        else:
            t = torch.from_numpy(np.ascontiguousarray(v))
        tensors[torchtune(k)] = t.contiguous()
    save_file(tensors, str(d / "model.safetensors"))
    json.dump(dict(cfg, model_type="sesame", quantization=qcfg), open(d / "config.json", "w"))
    model = load_model(str(d))
    assert isinstance(model, Model) and model.model.weight_format == "q8" and model.model.weight_fallback is None
    ref = SesameModel(cfg, dq, weight_dtype="bfloat16")
    rng = np.random.default_rng(seed("load"))
    tok, msk, pads = ragged_prompt(cfg, rng, [10, 6])
    us = rng.uniform(size=(5, 2, cfg["audio_num_codebooks"])).astype(np.float32)
    assert_same_frames("load_model", run_frames(model.model, cfg, tok, msk, pads, us, False), run_frames(ref, cfg, tok, msk, pads, us, False))
    # the opt-out dequantises at load: the same bits, bf16 storage
    plain = load_model(str(d), weight_storage="dequantized")
    assert plain.model.weight_format == "bf16"
    assert_same_frames("dequantized", run_frames(plain.model, cfg, tok, msk, pads, us, False), run_frames(ref, cfg, tok, msk, pads, us, False))
    with pytest.raises(ValueError):
        load_model(str(d), weight_storage="fp8")
    json.dump(dict(cfg, model_type="sesame", quantization={"group_size": 64, "bits": 3}), open(d / "config.json", "w"))
    with pytest.raises(ValueError, match="word"):
        load_model(str(d))


def _fallback_case(which):
    tiny = P.csm_tiny_config()
    if which == "hidden2304":  # q|k|v, gate|up and the projection get no fragment pack (tests/test_gpu_csm.py: ..._has_no_gemv_pack_...)
        return quantised_tiny(8, 64, 12, cfg=dict(tiny, backbone=dict(tiny["backbone"], num_layers=1, hidden=2304, intermediate=512)))
    if which == "mixed_qkv":  # k_proj of one layer at 4 bits, q / v at 8: the stacked q|k|v cannot share a format
        return quantised_tiny(8, 64, 13, per_layer={"backbone.layers.1.self_attn.k_proj": {"group_size": 64, "bits": 4}})
    return quantised_tiny(2, 64, 14)


@pytest.mark.parametrize("which", ["hidden2304", "mixed_qkv", "bits2"])
def test_checkpoints_that_cannot_stay_packed_fall_back_to_dequantised(which):
    from mlx_audio_amd.csm import SesameModel

    cfg, qw, qcfg, dq = _fallback_case(which)
    model = SesameModel(cfg, qw, quantization=qcfg)
    assert model.weight_format == "bf16" and model.weight_fallback, (model.weight_format, model.weight_fallback)
    ref = SesameModel(cfg, dq, weight_dtype="bfloat16")
    rng = np.random.default_rng(seed("fallback", which))
    tok, msk, pads = ragged_prompt(cfg, rng, [9, 6])
    us = rng.uniform(size=(3, 2, cfg["audio_num_codebooks"])).astype(np.float32)
    assert_same_frames(which, run_frames(model, cfg, tok, msk, pads, us, False, frames=3), run_frames(ref, cfg, tok, msk, pads, us, False, frames=3))
    assert model.weight_bytes == ref.weight_bytes
    report(f"csm_quant/fallback/{which}", bitexact=True, reason=model.weight_fallback)


def test_weight_bytes_of_csm_1b_widths(lib):
    """CSM-1B's layer widths with 2 + 1 layers: the Linears' device bytes are the sum of their quantised packs (kk_csm_qfrag_bytes) plus the bf16 packs
    of the audio heads -- no fp32 and no bf16 copy of a packed matrix -- and q4 < q8 < bf16 mode."""
    from mlx_audio_amd.csm import SesameModel
    from test_csm_quant_cpu import _linears, qfrag_bytes

    full = P.csm_config()
    cfg = dict(full, text_vocab_size=512, audio_num_codebooks=3, max_seq_len=64, backbone=dict(full["backbone"], num_layers=2),
               decoder=dict(full["decoder"], num_layers=1))
    got = {}
    for bits in (8, 4):
        _, qw, qcfg, dq = quantised_tiny(bits, 64, 5, cfg=cfg)
        m = SesameModel(cfg, qw, quantization=qcfg)
        assert m.weight_format == f"q{bits}"
        want = 0
        for name, K, N, split_ok in _linears(cfg):
            ks, nsub = frag_choice(lib, K, N, split_ok)
            if name == "audio_head":
                want += (cfg["audio_num_codebooks"] - 1) * (-(-N // (16 * nsub)) * 16 * nsub * K * 2)
            else:
                layers = cfg[name.split(".")[0]]["num_layers"] if "." in name else 1
                want += layers * sum(qfrag_bytes(lib, K, N, nsub, 64, bits))
        got[bits] = m.weight_bytes
        assert got[bits]["linear"] == want
        del m, qw
    bf = SesameModel(cfg, dq, weight_dtype="bfloat16").weight_bytes
    assert got[4]["linear"] < got[8]["linear"] < bf["linear"] and got[4]["total"] < got[8]["total"] < bf["total"]
    report("csm_quant/weight_bytes", q4=got[4], q8=got[8], bf16=bf)
