"""The packed-weight kernels of the Whisper text side (csrc/kk_whisper_text_kernels.hip) on their own, through the raw kk_op_* entries: the skinny-M
Linear and the token gather on an MLX affine-quantised matrix must carry, bit for bit, what their bf16 twins give on the dequantised matrix rounded to
bf16 -- every value is decoded to exactly that bf16 and the arithmetic behind it is the bf16 kernel's, in its order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

from _whisper_ref import bf16_round  # noqa: E402

from mlx_audio_amd import _lib, quant  # noqa: E402

EPS = 2.0 ** -23
N = 40  # two full column blocks and a tail of 8
KS = (128, 640, 2176)  # 4, 20 and 68 k-steps over 16 waves: a wave gets 0 or 1, 1 or 2, 4 or 5 of them
EPILOGUES = ((0, 0, 0), (1, 0, 0), (1, 2, 0), (1, 0, 1), (1, 2, 1))  # bias, act (2: GELU), residual


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pairs(scales, biases):
    return np.ascontiguousarray(np.stack([scales, biases], axis=-1), dtype=np.float32)  # [N][K / group][2]


def _dev_u32(words):
    import torch

    return torch.from_numpy(words.view(np.int32)).cuda()  # the bits are what matters


_data = {}


def _matrix(K, group, bits):
    """a quantised [N][K] matrix, its dequantised bf16 twin on the device, inputs, and the float64 product on what the kernels multiply"""
    import torch

    key = (K, group, bits)
    if key not in _data:
        g = np.random.default_rng(K * 131 + group * 7 + bits)
        words, scales, biases = quant.quantize_affine((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), group, bits)
        w = bf16_round(quant.dequantize_affine(words, scales, biases, group, bits))
        x = g.standard_normal((16, K)).astype(np.float32)
        bias = (0.5 * g.standard_normal(N)).astype(np.float32)
        res = g.standard_normal((16, N)).astype(np.float32)
        xb = bf16_round(x).astype(np.float64)
        _data[key] = dict(acc=xb @ w.astype(np.float64).T, mag=np.abs(xb) @ np.abs(w.astype(np.float64)).T, bias=bias, res=res,
                          wd=torch.from_numpy(w).cuda().bfloat16(), qd=_dev_u32(words), pd=torch.from_numpy(_pairs(scales, biases)).cuda(),
                          xd=torch.from_numpy(x).cuda(), bd=torch.from_numpy(bias).cuda(), rd=torch.from_numpy(res).cuda())
    return _data[key]


def _run(d, quantised, M, K, group, bits, use_bias, act, use_res, store=None, want_f32=True):
    import torch

    lib = _lib.load()
    x = d["xd"][:M].contiguous()
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda") if want_f32 else None
    ob, ldb, rows, nrows = (None, 0, None, 0) if store is None else store
    tail = (_p(d["bd"]) if use_bias else None, act, _p(d["rd"][:M].contiguous()) if use_res else None, N, _p(out), N, _p(ob), ldb, _p(rows), nrows)
    if quantised:
        rc = lib.kk_op_whisper_linear_rows_q(_st(), M, N, K, _p(x), K, _p(d["qd"]), _p(d["pd"]), group, bits, *tail)
    else:
        rc = lib.kk_op_whisper_linear_rows(_st(), M, N, K, _p(x), K, _p(d["wd"]), *tail)
    assert rc == 0, lib.kk_last_error()
    return out


def _erf(a):
    import torch

    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


@pytest.mark.parametrize("group", [32, 64, 128])
@pytest.mark.parametrize("bits", [4, 8])
def test_linear_rows_q_is_bit_equal_to_the_bf16_kernel_on_the_dequantised_matrix(bits, group):
    """K in {128, 640, 2176}, M in {1, 5, 16}, N = 40; plain, bias, bias + GELU, bias + residual, bias + GELU + residual: the fp32 rows are `==`.
    Then the bf16 strided store through a row table with one destination outside the store: the two stores are `==`, the skipped row and the unnamed
    rows untouched."""
    import torch

    for K in KS:
        d = _matrix(K, group, bits)
        for M in (1, 5, 16):
            for use_bias, act, use_res in EPILOGUES:
                want = _run(d, False, M, K, group, bits, use_bias, act, use_res).cpu().numpy()
                got = _run(d, True, M, K, group, bits, use_bias, act, use_res).cpu().numpy()
                assert np.isfinite(want).all()
                assert np.array_equal(got, want), (K, M, use_bias, act, use_res, float(np.abs(got - want).max()))
        stores = []
        rows = torch.tensor([7, 2, 99, -1, 0], dtype=torch.int32, device="cuda")  # 99 and -1 are outside the store of 10 rows
        for quantised in (False, True):
            store = torch.full((10, 2 * N + 8), -7.0, dtype=torch.bfloat16, device="cuda")
            f32 = _run(d, quantised, 5, K, group, bits, 1, 0, 0, store=(store[:, N:], 2 * N + 8, rows, 10))
            only = torch.full((10, 2 * N + 8), -7.0, dtype=torch.bfloat16, device="cuda")
            _run(d, quantised, 5, K, group, bits, 1, 0, 0, store=(only[:, N:], 2 * N + 8, rows, 10), want_f32=False)
            assert torch.equal(store, only)
            s = store.float().cpu().numpy()
            for m, row in ((0, 7), (1, 2), (4, 0)):
                assert np.array_equal(s[row, N: 2 * N], bf16_round(f32.cpu().numpy()[m]))
            untouched = np.ones_like(s, bool)
            for row in (7, 2, 0):
                untouched[row, N: 2 * N] = False
            assert (s[untouched] == -7.0).all()
            stores.append(s)
        assert np.array_equal(stores[0], stores[1])


@pytest.mark.parametrize("bits,group", [(4, 32), (4, 128), (8, 64)])
def test_linear_rows_q_against_float64(bits, group):
    """Against the float64 product of the dequantised matrix (rounded to bf16, as the matrix of the bf16 kernel's own test is), on x rounded as the kernel
    rounds it, at that test's bound: (K + 4) 2^-23 (sum_k |x_k w_k| + |bias| + |res|), kept for GELU (tests/test_gpu_whisper_text_kernels.py)."""
    worst = 0.0
    for K in KS:
        d = _matrix(K, group, bits)
        for M in (1, 5, 16):
            for use_bias, act, use_res in EPILOGUES:
                out = _run(d, True, M, K, group, bits, use_bias, act, use_res).cpu().numpy().astype(np.float64)
                ref = d["acc"][:M] + (d["bias"].astype(np.float64) if use_bias else 0.0)
                if act:
                    ref = ref * 0.5 * (1.0 + _erf(ref / np.sqrt(2.0)))
                if use_res:
                    ref = ref + d["res"][:M]
                bound = (K + 4) * EPS * (d["mag"][:M] + (np.abs(d["bias"]) if use_bias else 0.0) + (np.abs(d["res"][:M]) if use_res else 0.0))
                err = np.abs(out - ref)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (K, M, use_bias, act, use_res, float((err / bound).max()))
    print(f"bits {bits} group {group}: worst measured / bound = {worst:.3f}")


def test_linear_rows_q_checks_its_arguments():
    import torch

    lib = _lib.load()
    d = _matrix(128, 64, 4)
    x = d["xd"][:1].contiguous()
    out = torch.zeros((1, N), dtype=torch.float32, device="cuda")

    def call(M=1, K=128, group=64, bits=4, words=d["qd"], pairs=d["pd"], xx=x):
        return lib.kk_op_whisper_linear_rows_q(_st(), M, N, K, _p(xx), K, _p(words), _p(pairs), group, bits, None, 0, None, N, _p(out), N, None, 0, None, 0)

    assert call() == 0
    for kw, word in ((dict(M=17), b"M <= 16"), (dict(bits=2), b"bits is not 4 or 8"), (dict(bits=3), b"bits is not 4 or 8"), (dict(group=16), b"group size"),
                     (dict(group=256), b"group size"), (dict(K=80), b"multiple of 32"), (dict(K=64, group=128), b"multiple of the group"),
                     (dict(words=None), b"null"), (dict(pairs=None), b"null")):
        assert call(**kw) != 0 and word in lib.kk_last_error(), (kw, lib.kk_last_error())
    assert lib.kk_op_whisper_linear_rows_q(_st(), 1, N, 128, _p(x), 128, C.c_void_p(d["qd"].data_ptr() + 4), _p(d["pd"]), 64, 4, None, 0, None, N, _p(out), N, None, 0,
                                           None, 0) != 0  # words off their 8-byte alignment


@pytest.mark.parametrize("group", [32, 64, 128])
@pytest.mark.parametrize("bits", [4, 8])
def test_embed_q_is_bit_equal_to_the_bf16_gather_and_clamps_bad_ids(bits, group):
    import torch

    lib = _lib.load()
    V, D, ctx = 1000, 384, 48
    g = np.random.default_rng(5 + bits + group)
    words, scales, biases = quant.quantize_affine(g.standard_normal((V, D)).astype(np.float32), group, bits)
    table = bf16_round(quant.dequantize_affine(words, scales, biases, group, bits))
    pos = g.standard_normal((ctx, D)).astype(np.float32)
    tok = np.array([0, 999, 17, 1000, -3, 2 ** 31 - 1, 5, -2 ** 31], np.int32)
    at = np.array([0, 47, 3, 1, 2, 48, -1, 7], np.int32)
    R = len(tok)
    got = torch.full((R, D), float("nan"), dtype=torch.float32, device="cuda")
    want = torch.full((R, D), float("nan"), dtype=torch.float32, device="cuda")
    td, pd, tokd, atd = torch.from_numpy(table).cuda().bfloat16(), torch.from_numpy(pos).cuda(), torch.from_numpy(tok).cuda(), torch.from_numpy(at).cuda()
    qd, sd = _dev_u32(words), torch.from_numpy(_pairs(scales, biases)).cuda()
    assert lib.kk_op_whisper_embed(_st(), R, D, _p(tokd), _p(atd), _p(td), V, _p(pd), ctx, _p(want)) == 0
    assert lib.kk_op_whisper_embed_q(_st(), R, D, _p(tokd), _p(atd), _p(qd), _p(sd), group, bits, V, _p(pd), ctx, _p(got)) == 0, lib.kk_last_error()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), table[np.clip(tok, 0, V - 1)] + pos[np.clip(at, 0, ctx - 1)])
    assert lib.kk_op_whisper_embed_q(_st(), R, D, _p(tokd), _p(atd), _p(qd), _p(sd), 256, bits, V, _p(pd), ctx, _p(got)) != 0
    assert lib.kk_op_whisper_embed_q(_st(), R, D, _p(tokd), _p(atd), _p(qd), _p(sd), group, 2, V, _p(pd), ctx, _p(got)) != 0
