"""GPU parity tests of the streaming matrix-core Linear (csrc/kk_linear_rows.hip: Albert's and the text side's Linears while few rows are in flight)
through kk_op_linear_rows, against tests/_conv_ref.linear_rows (float64 on the bf16-rounded operands; pinned by tests/test_conv_ref_cpu.py).  The
conventions are those of tests/test_gpu_kokoro_kernels.py.

Layout of a case.  x [B][rows][K] sits in a buffer of row pitch ldx and item pitch xbs, the output in one of row pitch ldo and item pitch obs, with
two guard rows behind the last item.  The entry takes the flat form (one row axis over all items, a 16-row wave tile may span two utterances) when
both item pitches are dense (xbs = rows ldx, obs = rows ldo) and the per-item form otherwise.  The kernel loads 16 bytes per lane and stores packed
bf16 pairs, so the pitches are multiples of 8 (x) and of 2 (out): the padded cases add 8 to ldx and 16 to ldo, the per-item ones 64 and 128
elements behind each item.  NaN fills the pad columns of x, its rows from len[b] on and the space between items; the output starts as the sentinel
-512 (exact in bf16).  Checked per case: nothing outside [row < rows][col < N] of each item was written, rows [len[b], rows) are exactly zero, every
value is finite, |got - ref| <= bound on the live rows; report() logs worst error / bound.

Which shapes take which path (kk_launch_linear_rows_mfma): M = B rows (flat) or rows (per item); M <= 256 runs <NS 2, PD 12> (a wave owns 32
columns, 12 K chunks of 32 in flight), M > 256 runs <NS 4, PD 6> (64 columns, 6 chunks).  K = 32, 64, 96: the ring is deeper than the K loop and
its slots past the end are clamped duplicates; K = 416 (13 chunks) and 768 (24): no multiple of 12 / a multiple of 12 and 6.  N = 2 .. 66: the
last 16-column sub-block is partial, and the wave's last sub-blocks repeat the last real one and must not be stored.

Not reachable: Nb < N (a bias shorter than the output, the columns past it carrying zero weights).  kk_op_linear_rows sets Nb = N; only the
model's own fused q|k|v launch passes a smaller Nb, so that clamp (`col < Nb ? col : 0`) is exercised here only at col >= N, where nothing is stored.

Bound (u = 2^-24; nothing here is measured).  The products of two bf16 values are exact in fp32; one matrix instruction adds 32 of them to the
accumulator, K / 32 instructions in a chain, then the bias add:
  e = (K / 32 + 2) u S,  S = sum_k |x_k w_k|
  GELU (exact erf): e <- 1.13 e + |v| / 2 (6u + u |v|) + 2u |g|  (max g' = 1.129; erff within 2 ulp of a value <= 1, its rounded argument, the
  rounded 1 + erf, two products: the derivation in tests/test_gpu_conv_generic.py)
  + 2^-8 |ref| for the bf16 store;  bound = 2 e (a factor 2 of slack); assert worst <= 1.0."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import _conv_ref as R
from _util import report

pytestmark = pytest.mark.gpu

SENT = -512.0
U24 = 2.0**-24
GUARD = 2
ACT_NONE, ACT_GELU = 0, 2


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def bdev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def lens_of(B, rows):
    """{full, a third, 0}, repeated with other short lengths for more items."""
    pat = [rows, max(1, rows // 3), 0, rows, 1, rows, rows // 2, rows]
    return [pat[b % 8] for b in range(B)]


def case_data(key, B, rows, K, N, bias=True):
    rng = np.random.default_rng(seed_of(*key))
    return {"x": R.bf16_round(rng.standard_normal((B, rows, K))), "w": R.bf16_round(rng.standard_normal((N, K)) / np.sqrt(K)),
            "bias": rng.standard_normal(N).astype(np.float32) if bias else None}


def launch(lib, d, lens, *, act=ACT_NONE, padded=False, per_item=False):
    """One kk_op_linear_rows call -> (the blocks [B][rows][ldo], everything else of the output buffer as one flat array), float32."""
    x, w, bias = d["x"], d["w"], d["bias"]
    B, rows, K = x.shape
    N = w.shape[0]
    ldx, ldo = K + (8 if padded else 0), N + (16 if padded else 0)
    xbs, obs = rows * ldx + (64 if per_item else 0), rows * ldo + (128 if per_item else 0)
    xb = np.full((B, xbs), np.nan, np.float32)
    xv = xb[:, : rows * ldx].reshape(B, rows, ldx)
    xv[:, :, :K] = x
    for b, n in enumerate(lens if lens is not None else []):
        xv[b, n:] = np.nan
    xd, wd = bdev(xb), bdev(w)
    bd = torch.tensor(bias).cuda() if bias is not None else None
    ld = torch.tensor(np.asarray(lens, np.int32)).cuda() if lens is not None else None
    scratch = torch.zeros(((N + 15) // 16 * 16) * K, dtype=torch.bfloat16, device="cuda")
    out = torch.full((B * obs + GUARD * ldo,), SENT, dtype=torch.bfloat16, device="cuda")
    rc = lib.kk_op_linear_rows(stream(), B, P(xd), xbs, ldx, rows, P(ld), P(wd), N, K, P(bd), act, P(scratch), P(out), obs, ldo)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    o = out.float().cpu().numpy()
    items = o[: B * obs].reshape(B, obs)
    return items[:, : rows * ldo].reshape(B, rows, ldo), np.concatenate([items[:, rows * ldo :].ravel(), o[B * obs :]])


def layout_ok(blocks, rest, N, lens):
    assert np.all(rest == SENT), "written behind an item's rows"
    assert np.all(blocks[:, :, N:] == SENT), "a pad column of the output was written"
    blk = blocks[:, :, :N]
    assert np.isfinite(blk).all(), "non-finite output (a NaN pad element or a row past the length leaked)"
    assert np.all(blk != SENT), "an output element inside [rows][N] was left unwritten"
    for b, n in enumerate(lens if lens is not None else []):
        assert np.all(blk[b, n:] == 0.0), f"item {b}: rows from len on are not zero"
    return blk


def check(lib, name, B, rows, K, N, *, act=ACT_NONE, padded=False, per_item=False, bias=True, lens="ragged"):
    lens = lens_of(B, rows) if lens == "ragged" else lens
    d = case_data((name,), B, rows, K, N, bias)
    blk = layout_ok(*launch(lib, d, lens, act=act, padded=padded, per_item=per_item), N, lens)
    ref, S, pre = R.linear_rows(d["x"], d["w"], d["bias"], act, lens, parts=True)
    e = (K // 32 + 2) * U24 * S
    if act == ACT_GELU:
        e = 1.13 * e + 0.5 * np.abs(pre) * (6 * U24 + U24 * np.abs(pre)) + 2 * U24 * np.abs(R.gelu(pre))
    bound = 2.0 * (e + 2.0**-8 * np.abs(R.activation(pre, act)))
    worst = 0.0
    for b in range(B):
        n = lens[b] if lens is not None else rows
        if n:
            worst = max(worst, float((np.abs(blk[b, :n].astype(np.float64) - ref[b, :n]) / (bound[b, :n] + 1e-300)).max()))
    report(f"linear_rows/{name}", ratio=worst)
    assert worst <= 1.0, worst
    return blk


# (items, rows): M = items * rows at 16 k +- 1, 64 k +- 1, the switch of instantiations 256 / 257, and 1000.  rows 5, 21, 85 and 125 are no
# multiples of 16: a 16-row wave tile spans two utterances, the first of them shorter than its rows
FLAT_M = [(1, 1), (1, 15), (3, 5), (1, 16), (1, 17), (1, 63), (3, 21), (1, 64), (1, 65), (1, 255), (3, 85), (1, 256), (2, 128), (1, 257), (1, 1000),
          (8, 125)]


@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("B,rows", FLAT_M, ids=lambda v: str(v))
def test_flat_rows(lib, B, rows, padded):
    check(lib, f"flat/M{B}x{rows}_{'padded' if padded else 'dense'}", B, rows, 64, 34, padded=padded)


def test_flat_single_item_short_and_null_len(lib):
    """One item shorter than its rows (the tail of the only tile is zeros), and len == NULL (every row)."""
    check(lib, "flat/M1x65_short", 1, 65, 64, 34, lens=[40])
    check(lib, "flat/M3x21_null_len", 3, 21, 64, 34, lens=None)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU], ids=["none", "gelu"])
@pytest.mark.parametrize("rows", [37, 257, 300])
def test_per_item_form(lib, rows, act):
    """Item pitch larger than rows * ld, ldx = K + 8, ldo = N + 16: above 256 rows the per-item form runs the <4, 1, 6> instantiation per item."""
    check(lib, f"per_item/rows{rows}_act{act}", 3, rows, 96, 34, act=act, padded=True, per_item=True)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU], ids=["none", "gelu"])
@pytest.mark.parametrize("M", [37, 300])
@pytest.mark.parametrize("K", [32, 64, 96, 416, 768])
def test_k_chunks(lib, K, M, act):
    check(lib, f"k/K{K}_M{M}_act{act}", 1, M, K, 34, act=act, lens=[M - 5])


@pytest.mark.parametrize("M", [37, 300])
@pytest.mark.parametrize("N", [2, 14, 16, 18, 30, 34, 62, 66, 768])
def test_n_columns(lib, N, M):
    check(lib, f"n/N{N}_M{M}", 3 if M == 300 else 1, M // 3 if M == 300 else M, 64, N, padded=True, act=ACT_GELU if N in (18, 66) else ACT_NONE)


def test_no_bias(lib):
    check(lib, "flat/no_bias", 3, 21, 96, 34, bias=False)


@pytest.mark.parametrize("rows", [85, 125])
def test_batch_invariance(lib, rows):
    """An item inside the flat batch (its rows share wave tiles with its neighbours) has the bits of the item run alone; the kernel's header
    promises that a row's result depends on nothing but its own input row.  3 x 85 runs <2, 1, 12>, 3 x 125 runs <4, 1, 6>."""
    B, K, N = 3, 96, 34
    lens = lens_of(B, rows)
    d = case_data(("invariance", rows), B, rows, K, N)
    g3 = layout_ok(*launch(lib, d, lens, act=ACT_GELU), N, lens)
    for b in (0, 1):
        d1 = {"x": d["x"][b : b + 1], "w": d["w"], "bias": d["bias"]}
        g1 = layout_ok(*launch(lib, d1, lens[b : b + 1], act=ACT_GELU, padded=True), N, lens[b : b + 1])
        assert np.any(g1[0, : lens[b]] != 0) and same_bits(g3[b], g1[0])
    report(f"linear_rows/invariance/rows{rows}", worst=0.0)


@pytest.mark.parametrize("K,N,rows", [(48, 34, 4), (64, 33, 4), (64, 34, 0)], ids=["K48", "N33", "rows0"])
def test_refusals(lib, K, N, rows):
    """K % 32 != 0, an odd N and rows < 1 are refused with a message before anything is launched: the output keeps the sentinel."""
    x, w = bdev(np.zeros((1, 4, 64))), bdev(np.zeros((34, 64)))
    scratch = torch.zeros(48 * 64, dtype=torch.bfloat16, device="cuda")
    out = torch.full((4 * 34 + 8,), SENT, dtype=torch.bfloat16, device="cuda")
    rc = lib.kk_op_linear_rows(stream(), 1, P(x), rows * K, K, rows, None, P(w), N, K, None, ACT_NONE, P(scratch), P(out), rows * N, N)
    torch.cuda.synchronize()
    assert rc != 0 and lib.kk_last_error()
    assert bool((out == SENT).all())
