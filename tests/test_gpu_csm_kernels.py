"""GPU parity tests, kernel level, of the CSM frame step (kk_csm.hip, kk_csm_gemvm.h, kk_attn_cache.hip) through its kk_op_csm_* entry points -- the launchers
the frame itself runs -- against float64 numpy statements of the same operation.  u = 2^-24.

* Matrix-core GEMV (gemvm_kernel), prompt GEMM (gemmp_kernel), fp32 skinny GEMM: BIT-EXACT on integer-valued data whose every partial sum
  stays below 2^24 (any correct fp32 summation order is exact there), with inputs whose low bits only the third term of the exact three-way
  bf16 split carries; on random data within gamma * T, T = sum_k |x_k w_kn| (+ |res|), gamma = (K + 2) u -- the classic bound of a K-term
  fp32 dot product (the split's second and third terms are 2^-8 and 2^-16 smaller) -- plus the prologue's input perturbation for PRO 1 / 2.
  The observed maximum of err / (gamma T) goes to the parity report (_util.report).
* Batch invariance: a row's output bits do not depend on its position in the launch nor on the other rows.
* Attention (attn_step_kernel, attn_decode_kernel + attn_merge_kernel, attn_cache_kernel<true / false> + rope_append_kernel): RoPE with the
  same table, causal GQA softmax attention over the slots >= pad, within 1e-5 of max|V| for moderate scores and 2e-4 for scores up to ~80;
  the cache rows a single-token kernel appends are bit-identical to rope_append_kernel's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _attn_ref import attn_ref, make_attn_case, rope_table, rot32, rot64
from _util import report

pytestmark = pytest.mark.gpu

U = 2.0**-24


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def frag(lib, w, nsub):
    """kk_csm_frag_pack of w [K][N] (host) -> device buffer"""
    K, N = w.shape
    out = np.zeros(-(-N // (16 * nsub)) * 16 * nsub * K, np.uint16)
    assert lib.kk_csm_frag_pack(np.ascontiguousarray(w, np.float32).ctypes.data_as(C.c_void_p), K, N, nsub, out.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(out.view(np.int16)).cuda()


def gemv(lib, wf, K, N, M, x, *, pro=0, epi=0, ks=1, nsub=1, xrs=None, nw=None, eps=0.0, codes=None, cstride=1, cb=0, V=0, rows=1, emb=None,
         gather_out=None, res=None, out=None, part=None, expect_ok=True):
    """kk_op_csm_gemv; `out` (device, [M][N]) doubles as `res` when res is "out" (in place).  Returns out as numpy, or the rc on expect_ok=False."""
    if out is None:
        out = torch.full((M, N), 7.0, device="cuda")
    r = out if isinstance(res, str) else res
    if xrs is None and x is not None:
        xrs = x.shape[-1]
    if ks > 1 and part is None:
        part = torch.full((ks, M, N), 3.0, device="cuda")
    rc = lib.kk_op_csm_gemv(stream(), pro, epi, ks, nsub, K, N, M, P(wf), P(x), xrs or 0, P(nw), eps, P(codes), cstride, cb, V, rows, P(emb),
                            P(gather_out), P(r), N, P(out), N, P(part))
    if not expect_ok:
        torch.cuda.synchronize()
        return rc
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def gemm_prompt(lib, wf, K, N, M, nsub, x, res=None):
    out = torch.full((M, N), 7.0, device="cuda")
    rc = lib.kk_op_csm_gemm_prompt(stream(), K, N, M, nsub, P(wf), P(x), x.shape[-1], P(res), N, P(out), N)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


SCRATCH = 2 * 1024 * 256 * 16  # what a frame gives the skinny GEMM (run_frame)


def skinny(lib, w, x, res=None):
    K, N = w.shape
    M = x.shape[0]
    wd, xd = dev(w), dev(x)
    out = torch.full((M, N), 7.0, device="cuda")
    scratch = torch.empty(SCRATCH, device="cuda")
    rd = dev(res) if res is not None else None  # (every device buffer held until the launch has run)
    rc = lib.kk_op_csm_linear_skinny(stream(), K, N, M, P(wd), N, P(xd), P(rd), P(out), P(scratch), SCRATCH)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_bound(name, got, ref, T, gamma):
    """|got - ref| <= gamma T elementwise (float64 reference); logs the worst ratio and the rms error / rms T"""
    got = np.asarray(got, np.float64)
    d = np.abs(got - ref)
    bar = gamma * T + 1e-300
    ratio = float((d / bar).max())
    rms = float(np.sqrt((d**2).mean()) / max(1e-300, np.sqrt((T**2).mean())))
    report(name, max_ratio=ratio, rms_err_over_rms_T=rms, gamma_over_u=gamma / U)
    assert np.isfinite(got).all(), name
    assert ratio <= 1.0, (name, ratio)


# ------------------------------------------------------------------------------------------------------------- exact data
def exact_case(rng, kind, K, N, M, scale=1.0):
    """Integer data on which every fp32 partial sum is exact.  (a): |x| in [2^19, 2^20) (so the split's third term carries the low 4 bits),
    <= 15 nonzero +-1 weights per column at random k (over K slices, chunks and waves), x then scaled by `scale` (a power of two);
    (b): |x| < 2^9, dense weights in [-2, 2]."""
    if kind == "a":
        x = rng.integers(2**19, 2**20, (M, K)) * rng.choice([-1, 1], (M, K))
        w = np.zeros((K, N))
        for n in range(N):
            ks = rng.choice(K, min(15, K), replace=False)
            w[ks, n] = rng.choice([-1, 1], ks.size)
        x = x * scale
    else:
        x = rng.integers(-(2**9) + 1, 2**9, (M, K))
        w = rng.integers(-2, 3, (K, N))
    return x.astype(np.float64), w.astype(np.float64)


EXACT_GEMV = [
    # kind, K, N, M, nsub, scale
    ("a", 32, 16, 1, 1, 1.0),
    ("a", 64, 40, 9, 2, 1.0),
    ("a", 1056, 2051, 17, 1, 1.0),
    ("a", 2240, 80, 8, 4, 2.0**-30),
    ("a", 2080, 48, 33, 1, 2.0**-30),
    ("b", 2048, 3072, 7, 1, 1.0),
    ("b", 96, 16384, 2, 4, 1.0),
]


@pytest.mark.parametrize("kind,K,N,M,nsub,scale", EXACT_GEMV)
def test_gemv_bitexact_on_integer_data(lib, kind, K, N, M, nsub, scale):
    rng = np.random.default_rng(K + N + M)
    x, w = exact_case(rng, kind, K, N, M, scale)
    wf, xd = frag(lib, w, nsub), dev(x)
    got = gemv(lib, wf, K, N, M, xd, nsub=nsub)
    np.testing.assert_array_equal(got.astype(np.float64), x @ w)
    # EPI 1 in place (res == out), the o projection's form
    res = rng.integers(-(2**20), 2**20, (M, N)).astype(np.float64) * scale
    got = gemv(lib, wf, K, N, M, xd, nsub=nsub, epi=1, res="out", out=dev(res))
    np.testing.assert_array_equal(got.astype(np.float64), x @ w + res)
    report(f"csm_kernels/gemv_exact/{kind}/K{K}_N{N}_M{M}_nsub{nsub}", bitexact=True)


@pytest.mark.parametrize("ks,K,N,M,nsub", [(2, 4096, 48, 3, 1), (5, 5120, 40, 9, 2), (8, 8192, 2048, 8, 4), (16, 16384, 64, 2, 1)])
def test_gemv_split_k_bitexact_on_integer_data(lib, ks, K, N, M, nsub):
    """Split-K (EPI 2 slices + combine_slices_kernel: out += sum of the slices) of the down projection's SwiGLU prologue: with gate = 32,
    silu(gate) rounds to exactly 32 in fp32, so the staged input is 32 * up -- integer data (a) again."""
    rng = np.random.default_rng(ks)
    up, w = exact_case(rng, "a", K, N, M)
    x = np.concatenate([np.full((M, K), 32.0), up], 1)
    res = rng.integers(-(2**19), 2**19, (M, N)).astype(np.float64) * 32  # (every partial sum: a multiple of 32 below 2^29)
    got = gemv(lib, frag(lib, w, nsub), K, N, M, dev(x), pro=2, epi=2, ks=ks, nsub=nsub, out=dev(res))
    np.testing.assert_array_equal(got.astype(np.float64), (32 * up) @ w + res)
    report(f"csm_kernels/gemv_splitk_exact/ks{ks}_K{K}_N{N}_M{M}", bitexact=True)


@pytest.mark.parametrize("rows", [1, 2])
def test_gemv_pro3_gathers_clamped_embedding_rows_bitexact(lib, rows):
    """PRO 3 (the projection of the depth decoder's first step): an item's last row is emb[code + cb V], its other row x[item]; code ids < 0 and
    >= V read the clamped row."""
    rng = np.random.default_rng(rows)
    K, N, V, cb, items, cstride = 1024, 1024, 37, 2, 9, 3
    x, w = exact_case(rng, "a", K, N, items)
    emb, _ = exact_case(rng, "a", K, N, 4 * V)
    codes = rng.integers(0, V, (items, cstride))
    codes[:4, 0] = [-5, V, V + 100, -1]
    M = items * rows
    got = gemv(lib, frag(lib, w, 1), K, N, M, dev(x), pro=3, rows=rows, codes=dev(codes.astype(np.int32), torch.int32), cstride=cstride, cb=cb,
               V=V, emb=dev(emb))
    inp = np.zeros((M, K))
    for i in range(items):
        inp[i * rows + rows - 1] = emb[np.clip(codes[i, 0], 0, V - 1) + cb * V]
        if rows == 2:
            inp[i * rows] = x[i]
    np.testing.assert_array_equal(got.astype(np.float64), inp @ w)


def test_gemv_pro3_refuses_items_of_more_than_two_rows(lib):
    K, N = 64, 16
    wf = frag(lib, np.ones((K, N)), 1)
    x, emb = dev(np.ones((2, K))), dev(np.ones((4, K)))
    codes = dev(np.zeros(8, np.int32), torch.int32)
    for rows in (4, 8):
        rc = gemv(lib, wf, K, N, 8, x, pro=3, rows=rows, codes=codes, V=4, emb=emb, expect_ok=False)
        assert rc != 0 and b"item rows" in lib.kk_last_error()


def test_gemv_refuses_inconsistent_slices(lib):
    x = dev(np.ones((1, 2 * 4096)))
    for K, ks, nsub, epi in [(2304, 1, 1, 0), (4096, 3, 1, 2), (4096, 1, 1, 2), (4096, 4, 1, 0), (4096, 4, 3, 2), (4096, 32, 1, 2), (1000, 1, 1, 0)]:
        wf = torch.zeros(4096 * 64, dtype=torch.int16, device="cuda")
        part = torch.zeros(32 * 64, device="cuda")
        rc = gemv(lib, wf, K, 16, 1, x, pro=2, epi=epi, ks=ks, nsub=nsub, part=part, res=None, expect_ok=False)
        assert rc != 0, (K, ks, nsub, epi)


@pytest.mark.parametrize("kind,K,N,M,nsub", [("a", 96, 40, 63, 2), ("a", 2048, 80, 65, 4), ("b", 2048, 200, 130, 1), ("a", 32, 16, 3, 1)])
def test_gemm_prompt_bitexact_on_integer_data(lib, kind, K, N, M, nsub):
    rng = np.random.default_rng(K * 3 + M)
    x, w = exact_case(rng, kind, K, N, M)
    res = rng.integers(-(2**20), 2**20, (M, N)).astype(np.float64)
    wf, xd = frag(lib, w, nsub), dev(x)
    np.testing.assert_array_equal(gemm_prompt(lib, wf, K, N, M, nsub, xd).astype(np.float64), x @ w)
    np.testing.assert_array_equal(gemm_prompt(lib, wf, K, N, M, nsub, xd, dev(res)).astype(np.float64), x @ w + res)
    for s in (2.0**-30, -1.0):
        np.testing.assert_array_equal(gemm_prompt(lib, wf, K, N, M, nsub, dev(x * s)).astype(np.float64), (x * s) @ w)


@pytest.mark.parametrize("kind,K,N,M", [("a", 2048, 2051, 1), ("a", 1056, 300, 17), ("b", 8192, 1024, 2), ("b", 100, 70, 33)])
def test_skinny_bitexact_on_integer_data(lib, kind, K, N, M):
    rng = np.random.default_rng(K + M)
    x, w = exact_case(rng, kind, K, N, M)
    res = rng.integers(-(2**20), 2**20, (M, N)).astype(np.float64)
    np.testing.assert_array_equal(skinny(lib, w, x, res).astype(np.float64), x @ w + res)
    np.testing.assert_array_equal(skinny(lib, w, -x * 2.0**-30).astype(np.float64), (-x * 2.0**-30) @ w)


# ------------------------------------------------------------------------------------------------------------- random data
def rand_w(rng, K, N):
    return bf16(rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float64)


GEMV_RANDOM = [
    # pro, epi, K, N, M, nsub
    (0, 0, 32, 16, 1, 1),
    (0, 0, 64, 40, 2, 2),
    (0, 1, 96, 2051, 7, 1),
    (0, 0, 1024, 3072, 8, 1),
    (0, 1, 1056, 48, 9, 1),
    (0, 0, 2240, 16384, 16, 4),
    (1, 0, 1024, 1536, 17, 1),
    (1, 0, 2048, 3072, 33, 1),
    (1, 0, 2080, 2051, 9, 2),
    (1, 0, 32, 40, 1, 4),
    (2, 1, 96, 1024, 8, 2),
    (2, 1, 2048, 2051, 2, 1),
    (2, 1, 1056, 64, 17, 4),
]


def gemv_ref(pro, x, w, nw=None, eps=0.0, res=None):
    """(ref, T) in float64 of the GEMV's operation; T = the sum of |terms| the fp32 arithmetic meets"""
    K = w.shape[0]
    if pro == 2:
        g, up = x[:, :K], x[:, K:]
        x = g / (1.0 + np.exp(-g)) * up
    if pro == 1:
        s = 1.0 / np.sqrt((x * x).mean(1, keepdims=True) + eps)
        ref, T = ((x * nw) @ w) * s, (np.abs(x * nw) @ np.abs(w)) * s
    else:
        ref, T = x @ w, np.abs(x) @ np.abs(w)
    if res is not None:
        ref, T = ref + res, T + np.abs(res)
    return ref, T


# the prologue's input perturbation in units of u, on top of (K + 2) u: PRO 1 -- x * nw (1), the sum of squares (<= K, halved by sqrtf), sqrtf,
# the division and the scale multiply (<= 4); PRO 2 -- __expf (v_exp_f32 of |g| log2 e <= 12: ~9), 1 + e, rcpf, two products (<= 64 in all).
# Measured on MI355X: at most 1.3 % of these bars (PRO 1, K = 32; PRO 2, K = 96), none needed loosening.
def prologue_u(pro, K):
    return K / 2 + 8 if pro == 1 else (64 if pro == 2 else 0)


@pytest.mark.parametrize("pro,epi,K,N,M,nsub", GEMV_RANDOM)
def test_gemv_random_within_fp32_bound(lib, pro, epi, K, N, M, nsub):
    rng = np.random.default_rng(pro * 1000 + K + M)
    w = rand_w(rng, K, N)
    if pro == 2:
        x = np.concatenate([rng.uniform(-8, 8, (M, K)), rng.standard_normal((M, K))], 1).astype(np.float32).astype(np.float64)
    else:
        x = rng.standard_normal((M, K)).astype(np.float32).astype(np.float64)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32).astype(np.float64) if pro == 1 else None
    res = rng.standard_normal((M, N)).astype(np.float32).astype(np.float64) if epi == 1 else None
    got = gemv(lib, frag(lib, w, nsub), K, N, M, dev(x), pro=pro, epi=epi, nsub=nsub, nw=dev(nw) if nw is not None else None, eps=1e-5,
               res="out" if epi == 1 else None, out=dev(res) if epi == 1 else None)
    ref, T = gemv_ref(pro, x, w, nw, 1e-5, res)
    check_bound(f"csm_kernels/gemv_random/pro{pro}_epi{epi}/K{K}_N{N}_M{M}_nsub{nsub}", got, ref, T, (K + 2 + prologue_u(pro, K)) * U)


@pytest.mark.parametrize("ks,K,N,M,nsub", [(4, 4096, 2048, 1, 4), (5, 5120, 80, 9, 2), (8, 8192, 1024, 8, 2), (16, 16384, 40, 3, 1)])
def test_gemv_split_k_random_within_fp32_bound(lib, ks, K, N, M, nsub):
    rng = np.random.default_rng(ks * 7 + M)
    w = rand_w(rng, K, N)
    x = np.concatenate([rng.uniform(-8, 8, (M, K)), rng.standard_normal((M, K))], 1).astype(np.float32).astype(np.float64)
    h = rng.standard_normal((M, N)).astype(np.float32).astype(np.float64)
    got = gemv(lib, frag(lib, w, nsub), K, N, M, dev(x), pro=2, epi=2, ks=ks, nsub=nsub, out=dev(h))
    ref, T = gemv_ref(2, x, w, res=h)
    check_bound(f"csm_kernels/gemv_splitk_random/ks{ks}_K{K}_N{N}_M{M}", got, ref, T, (K + 2 + ks + prologue_u(2, K)) * U)


def test_gemv_pro1_gathers_rows_by_code(lib):
    """PRO 1 with codes (the depth decoder's later steps): row m is emb[code_m + cb V], clamped; column block 0 writes it to gather_out."""
    rng = np.random.default_rng(5)
    K, N, V, cb, M = 1024, 1536, 40, 3, 9
    w = rand_w(rng, K, N)
    emb = rng.standard_normal((5 * V, K)).astype(np.float32).astype(np.float64)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32).astype(np.float64)
    codes = rng.integers(0, V, (M, 2))
    codes[:3, 0] = [-1, V, 3 * V]
    gout = torch.full((M, K), 9.0, device="cuda")
    got = gemv(lib, frag(lib, w, 1), K, N, M, None, pro=1, nw=dev(nw), eps=1e-5, codes=dev(codes.astype(np.int32), torch.int32), cstride=2, cb=cb,
               V=V, emb=dev(emb), gather_out=gout)
    rows = emb[np.clip(codes[:, 0], 0, V - 1) + cb * V]
    np.testing.assert_array_equal(gout.cpu().numpy().astype(np.float64), rows)
    ref, T = gemv_ref(1, rows, w, nw, 1e-5)
    check_bound("csm_kernels/gemv_random/pro1_codes", got, ref, T, (K + 2 + prologue_u(1, K)) * U)


@pytest.mark.parametrize("K,N,M,nsub,with_res", [(32, 40, 3, 1, False), (96, 2051, 63, 2, True), (2048, 1024, 64, 4, False), (96, 300, 65, 1, True),
                                                 (2048, 80, 200, 2, True), (1056, 3072, 17, 1, False)])
def test_gemm_prompt_random_within_fp32_bound(lib, K, N, M, nsub, with_res):
    rng = np.random.default_rng(K + M + nsub)
    w = rand_w(rng, K, N)
    x = rng.standard_normal((M, K)).astype(np.float32).astype(np.float64)
    res = rng.standard_normal((M, N)).astype(np.float32).astype(np.float64) if with_res else None
    got = gemm_prompt(lib, frag(lib, w, nsub), K, N, M, nsub, dev(x), dev(res) if with_res else None)
    ref, T = gemv_ref(0, x, w, res=res)
    check_bound(f"csm_kernels/gemm_prompt_random/K{K}_N{N}_M{M}_nsub{nsub}", got, ref, T, (K + 2) * U)


@pytest.mark.parametrize("K,N,M", [(2048, 3072, 1), (1024, 16384, 2), (8192, 2048, 17), (2048, 2051, 33), (100, 70, 5)])
def test_skinny_random_within_fp32_bound(lib, K, N, M):
    rng = np.random.default_rng(K + N + M)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32).astype(np.float64)
    x = rng.standard_normal((M, K)).astype(np.float32).astype(np.float64)
    res = rng.standard_normal((M, N)).astype(np.float32).astype(np.float64)
    got = skinny(lib, w, x, res)
    ref, T = gemv_ref(0, x, w, res=res)
    check_bound(f"csm_kernels/skinny_random/K{K}_N{N}_M{M}", got, ref, T, (K + 2) * U)


# ------------------------------------------------------------------------------------------------------------- batch invariance
def _probe_everywhere(rng, M, K, run):
    """run(x [M][K]) -> out [M][N] for the probe row at every position among other random rows; every result row of the probe must have the bits
    of the M = 1 launch"""
    probe = rng.standard_normal(K).astype(np.float32)
    alone = run(probe[None])[0]
    for p in range(M):
        x = rng.standard_normal((M, K)).astype(np.float32) * rng.uniform(0.1, 10)
        x[p] = probe
        got = run(x)[p]
        np.testing.assert_array_equal(got.view(np.uint32), alone.view(np.uint32), err_msg=f"row {p} of {M}")


def test_batch_invariance_gemv_gemm_prompt_skinny(lib):
    rng = np.random.default_rng(77)
    K, N = 1056, 80
    w = rand_w(rng, K, N)
    nw = dev(rng.uniform(0.5, 1.5, K))
    wf2, wf1 = frag(lib, w, 2), frag(lib, w, 1)
    _probe_everywhere(rng, 17, K, lambda x: gemv(lib, wf2, K, N, x.shape[0], dev(x), pro=1, nw=nw, eps=1e-5, nsub=2))
    _probe_everywhere(rng, 130, K, lambda x: gemm_prompt(lib, wf1, K, N, x.shape[0], 1, dev(x)))
    for M in (3, 12, 20):
        _probe_everywhere(rng, M, K, lambda x: skinny(lib, w, x))
    # split-K (down projection form): the probe row's SwiGLU input and its residual row at every position of M = 17
    K2, ks = 4096, 4
    w2 = rand_w(rng, K2, N)
    wf = frag(lib, w2, 1)
    h = rng.standard_normal(N).astype(np.float32)

    def run_split(x):  # x = [gate | up] rows
        return gemv(lib, wf, K2, N, x.shape[0], dev(x), pro=2, epi=2, ks=ks, out=dev(np.tile(h, (x.shape[0], 1))))

    _probe_everywhere(rng, 17, 2 * K2, run_split)
    report("csm_kernels/batch_invariance", bitexact=True)


# ------------------------------------------------------------------------------------------------------------- attention
def attn_single_ref(qkv, kc, vc, rope, H, KV, hd, offset, pads):
    B = qkv.shape[0]
    scale = float(1.0 / np.sqrt(np.float32(hd)))
    out = np.zeros((B, H * hd))
    for b in range(B):
        nk = offset + 1 - pads[b]
        if nk <= 0:
            continue
        cs = rope[offset - pads[b]]
        q = rot64(qkv[b, : H * hd].reshape(H, hd), cs)
        kn = rot64(qkv[b, H * hd : (H + KV) * hd].reshape(KV, hd), cs)
        vn = qkv[b, (H + KV) * hd :].reshape(KV, hd).astype(np.float64)
        keys = np.concatenate([kc[b, pads[b] : offset].reshape(-1, KV, hd).astype(np.float64), kn[None]], 0)
        vals = np.concatenate([vc[b, pads[b] : offset].reshape(-1, KV, hd).astype(np.float64), vn[None]], 0)
        out[b] = attn_ref(q, keys, vals, scale).reshape(-1)
    return out


def run_attn_single(lib, form, qkv, kc, vc, rope, H, KV, hd, offset, pads):
    B, max_pos = kc.shape[0], kc.shape[1]
    kd, vd = dev(kc), dev(vc)
    out = torch.full((B, H * hd), 7.0, device="cuda")
    part = torch.full((8 * B * H * (hd + 2),), 5.0, device="cuda")
    qd, rd, pd = dev(qkv), dev(rope), dev(np.asarray(pads, np.int32), torch.int32)
    rc = lib.kk_op_csm_attn_single(stream(), form, B, H, KV, hd, P(qd), P(kd), P(vd), max_pos, offset, P(rd), P(pd), P(out), P(part))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy()


def rope_append_rows(lib, qkv, kc, vc, rope, H, KV, hd, offset, pads):
    """what rope_append_kernel (through kk_op_csm_attn_prompt, S = 1) writes: caches, rotated q"""
    B, max_pos = kc.shape[0], kc.shape[1]
    qd, kd, vd = dev(qkv), dev(kc), dev(vc)
    out = torch.empty((B, H * hd), device="cuda")
    rd, pd = dev(rope), dev(np.asarray(pads, np.int32), torch.int32)
    rc = lib.kk_op_csm_attn_prompt(stream(), B, 1, H, KV, hd, P(qd), P(kd), P(vd), max_pos, offset, P(rd), P(pd), P(out))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return qd.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy()


def check_attn_single(lib, name, form, qkv, kc, vc, rope, H, KV, hd, offset, pads, bar):
    got, kd, vd = run_attn_single(lib, form, qkv, kc, vc, rope, H, KV, hd, offset, pads)
    ref = attn_single_ref(qkv, kc, vc, rope, H, KV, hd, offset, pads)
    vmax = max(float(np.abs(vc[b, pads[b] : offset]).max(initial=0.0)) for b in range(len(pads)))
    vmax = max(vmax, float(np.abs(qkv[:, (H + KV) * hd :]).max()))
    err = float(np.abs(got - ref).max()) / vmax
    report(name, err_over_vmax=err, bar=bar, ratio=err / bar)
    assert np.isfinite(got).all() and err <= bar, (name, err)
    # the appended rows: bit-identical to rope_append_kernel's, and to the same fp32 expressions on the host; nothing else of the caches changed
    qr, kr, vr = rope_append_rows(lib, qkv, kc, vc, rope, H, KV, hd, offset, pads)
    np.testing.assert_array_equal(kd.view(np.uint32), kr.view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(vd.view(np.uint32), vr.view(np.uint32), err_msg=name)
    for b in range(len(pads)):
        cs = rope[max(offset - pads[b], 0)]
        kn = rot32(qkv[b, H * hd : (H + KV) * hd].reshape(KV, hd), cs).reshape(-1)
        np.testing.assert_array_equal(kd[b, offset].view(np.uint32), kn.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(qr[b, : H * hd].view(np.uint32), rot32(qkv[b, : H * hd].reshape(H, hd), cs).reshape(-1).view(np.uint32))
    keep = np.ones(kc.shape[:2], bool)
    keep[:, offset] = False
    np.testing.assert_array_equal(kd[keep], kc[keep])
    np.testing.assert_array_equal(vd[keep], vc[keep])


STEP, DECODE, CACHE = 1, 2, 3


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("max_pos", [17, 33, 64])
def test_attn_short_cache_forms(lib, hd, G, max_pos):
    """attn_step_kernel (the step's choice at max_pos <= 64), and attn_cache_kernel<true> / attn_decode_kernel on the same cases: one key (offset 0)
    and a full cache with three different pads, moderate scores"""
    rng = np.random.default_rng(hd + G * 10 + max_pos)
    KV = 2
    H = G * KV
    for offset, pads in [(0, [0, 0, 0]), (max_pos - 1, [0, 5, max_pos - 1]), (max_pos // 2, [1, 0, 3])]:
        qkv, kc, vc, rope = make_attn_case(rng, 3, H, KV, hd, max_pos, offset, pads, "moderate")
        for form in (0, STEP, CACHE, DECODE):
            check_attn_single(lib, f"csm_kernels/attn_short/form{form}/hd{hd}_G{G}_mp{max_pos}_off{offset}", form, qkv, kc, vc, rope, H, KV, hd,
                              offset, pads, 1e-5)


# max_pos per (hd, wanted key splits): chunks of 8192 / hd keys, one split per 2 chunks, at most 8
DECODE_CASES = [(64, 200, 1), (64, 400, 2), (64, 700, 3), (64, 2048, 8), (128, 100, 1), (128, 250, 2), (128, 330, 3), (128, 1100, 8)]


@pytest.mark.parametrize("hd,max_pos,nsplit", DECODE_CASES)
@pytest.mark.parametrize("regime", ["moderate", "large"])
def test_attn_long_cache_decode_and_merge(lib, hd, max_pos, nsplit, regime):
    """attn_decode_kernel (+ attn_merge_kernel over its key splits; the step's choice past 64 positions) and attn_cache_kernel<true>: items whose
    key counts are CH - 1, CH, CH + 1, 2 CH, 1, 3 CH + 5 and the whole cache (CH = 8192 / hd keys per chunk), so that a chunk ends at, before
    and after the new key and whole splits hold no key; large scores with the dominant key in the first chunk, the last chunk, a late split."""
    CH = 8192 // hd
    nch = -(-max_pos // CH)
    assert min(max((nch + 1) // 2, 1), 8) == nsplit
    rng = np.random.default_rng(hd * 7 + max_pos + (regime == "large"))
    G, KV = 4, 2
    H = G * KV
    offset = max_pos - 1
    nks = [n for n in (CH - 1, CH, CH + 1, 2 * CH, 1, 3 * CH + 5, max_pos) if n <= max_pos]
    pads = [offset + 1 - n for n in nks]
    dom = None
    if regime == "large":  # dominant key: first chunk of the item's keys, its last chunk, or the start of the last split's first chunk
        late = [p + (nsplit - 1) * CH if p + (nsplit - 1) * CH < offset else offset for p in pads]
        choice = [pads, [max(p, offset - 3) for p in pads], late]
        dom = [choice[i % 3][i] for i in range(len(pads))]
    qkv, kc, vc, rope = make_attn_case(rng, len(pads), H, KV, hd, max_pos, offset, pads, regime, dom)
    bar = 1e-5 if regime == "moderate" else 2e-4
    for form in (0, DECODE, CACHE):
        check_attn_single(lib, f"csm_kernels/attn_long/{regime}/form{form}/hd{hd}_mp{max_pos}", form, qkv, kc, vc, rope, H, KV, hd, offset, pads, bar)
    # a shorter cache in the same buffers (offset inside the second split), pads 0 / 1 / 7
    off2 = min(CH * 2 + 3, max_pos - 1)
    pads2 = [0, 1, 7]
    qkv, kc, vc, rope = make_attn_case(rng, 3, H, KV, hd, max_pos, off2, pads2, regime, [5, off2 - 1, off2] if regime == "large" else None)
    check_attn_single(lib, f"csm_kernels/attn_long/{regime}/off{off2}/hd{hd}_mp{max_pos}", DECODE, qkv, kc, vc, rope, H, KV, hd, off2, pads2, bar)


def test_attn_single_refuses_forms_whose_preconditions_fail(lib):
    B, H, KV, hd, max_pos = 1, 16, 1, 64, 65
    qkv = torch.zeros((B, (H + 2 * KV) * 128), device="cuda")
    kc = torch.zeros((B, max_pos, KV * 128), device="cuda")
    vc, rope = torch.zeros_like(kc), torch.zeros((max_pos, 64, 2), device="cuda")
    out, part = torch.zeros((B, H * 128), device="cuda"), torch.zeros(8 * B * H * 130, device="cuda")

    def call(form, H_, KV_, hd_, mp):
        return lib.kk_op_csm_attn_single(stream(), form, B, H_, KV_, hd_, P(qkv), P(kc), P(vc), mp, 0, P(rope), None, P(out), P(part))

    assert call(STEP, 4, 1, 64, 65) != 0      # short-cache kernel past 64 positions
    assert call(STEP, 16, 1, 64, 64) != 0     # G = 16
    assert call(DECODE, 16, 1, 64, 64) != 0
    assert call(DECODE, 4, 1, 96, 64) != 0    # head_dim 96
    assert call(CACHE, 4, 1, 96, 64) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,offset,pads,G,hd", [(2, 0, [0, 1], 4, 64), (9, 0, [0, 4, 8], 8, 128), (64, 7, [0, 3], 4, 128), (190, 0, [0, 60], 8, 64),
                                                (9, 30, [2, 0, 29], 8, 64)])
def test_attn_prompt_block(lib, S, offset, pads, G, hd):
    """rope_append_kernel + attn_cache_kernel<false> (S > 1): causal attention of the block over the cache slots >= pad[b]; the appended rows and the
    rotated q bit-identical to the fp32 expressions (padding rows rotated with position 0)"""
    rng = np.random.default_rng(S + offset + hd)
    KV = 2
    H, B = G * KV, len(pads)
    max_pos = offset + S + 5
    W = (H + 2 * KV) * hd
    rope = rope_table(rng, max_pos, hd)
    qkv = rng.standard_normal((B, S, W)).astype(np.float32)
    kc = (rng.standard_normal((B, max_pos, KV * hd)) * 1e3).astype(np.float32)
    vc = (rng.standard_normal((B, max_pos, KV * hd)) * 1e3).astype(np.float32)
    for b in range(B):
        if pads[b] < offset:
            kc[b, pads[b] : offset] = rng.standard_normal((offset - pads[b], KV * hd))
            vc[b, pads[b] : offset] = rng.standard_normal((offset - pads[b], KV * hd))
    qd, kd, vd = dev(qkv), dev(kc), dev(vc)
    out = torch.full((B, S, H * hd), 7.0, device="cuda")
    rd, pd = dev(rope), dev(np.asarray(pads, np.int32), torch.int32)
    rc = lib.kk_op_csm_attn_prompt(stream(), B, S, H, KV, hd, P(qd), P(kd), P(vd), max_pos, offset, P(rd), P(pd), P(out))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    got, qg, kg, vg = out.cpu().numpy(), qd.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy()
    scale = float(1.0 / np.sqrt(np.float32(hd)))
    err = 0.0
    for b in range(B):
        cs = rope[np.maximum(offset + np.arange(S) - pads[b], 0)]  # [S][hd/2][2]
        q32 = rot32(qkv[b, :, : H * hd].reshape(S, H, hd), cs[:, None])
        k32 = rot32(qkv[b, :, H * hd : (H + KV) * hd].reshape(S, KV, hd), cs[:, None])
        np.testing.assert_array_equal(qg[b, :, : H * hd].view(np.uint32), q32.reshape(S, -1).view(np.uint32))
        np.testing.assert_array_equal(kg[b, offset : offset + S].view(np.uint32), k32.reshape(S, -1).view(np.uint32))
        np.testing.assert_array_equal(vg[b, offset : offset + S], qkv[b, :, (H + KV) * hd :])
        keys = kg[b].reshape(max_pos, KV, hd).astype(np.float64)
        vals = vg[b].reshape(max_pos, KV, hd).astype(np.float64)
        for s in range(S):
            hi = offset + s + 1
            if hi <= pads[b]:  # a padding row: no key, output zero
                assert not got[b, s].any()
                continue
            q = rot64(qkv[b, s, : H * hd].reshape(H, hd), cs[s])
            ref = attn_ref(q, keys[pads[b] : hi], vals[pads[b] : hi], scale).reshape(-1)
            vmax = float(np.abs(vals[pads[b] : hi]).max())
            err = max(err, float(np.abs(got[b, s] - ref).max()) / vmax)
    report(f"csm_kernels/attn_prompt/S{S}_off{offset}_G{G}_hd{hd}", err_over_vmax=err, bar=1e-5, ratio=err / 1e-5)
    assert err <= 1e-5, err
    keep = np.ones(kc.shape[:2], bool)
    keep[:, offset : offset + S] = False
    np.testing.assert_array_equal(kg[keep], kc[keep])
