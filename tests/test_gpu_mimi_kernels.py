"""GPU parity tests of mlx-audio_amd/csrc/kk_mimi.hip on its own: the codec's conv dispatch (Run::conv, through kk_op_mimi_conv, which reports the
kernel it launched) and every file-local kernel (through kk_op_mimi_*), against the references of tests/_mimi_ref.py on the operands the kernel
sees (bf16 RNE where it reads bf16).  tests/test_mimi_ref_cpu.py pins those references.

Every input carries NaN in its pad columns, in rows outside the valid range and in the unused columns of the weight pack; every output starts as
a sentinel, so a leak or a stray write shows.  Each case reports its worst error as a fraction of its bound (report()).

Bits (the build has -ffp-contract=off, numpy float32 reproduces the kernels' operations): rvq_sum, upsample_dw, edge_pad, rvq_argmin, the carry
kernels, and the few-rows kernel's batch invariance.

Bounds (u24 = 2^-24 is the unit round-off of fp32, 2^-23 its spacing at 1; S = sum |x w| over the taps of an output):
  rope        8 * 2^-23 (|x0| + |x1|): three fp32 roundings of the two-product sum and up to 4 ulp on cosf / sinf of magnitude <= 1; bf16 adds
              2^-8 |ref| for the one output rounding.  A pair or position slip of one moves the slowest frequency's angle by 1.3e-4.
  last conv   (K Cin + 2) u24 (S + |bias|): one fp32 FMA chain.  With elu the staged form multiplies bf16(elu(x)), which the reference knows
              exactly (inputs are moved off bf16 ties, _mimi_ref.avoid_elu_ties); the other two keep elu(x) in fp32, whose exp adds
              2^-21 sum |w| (a few ulp of a value <= 1 per operand).
  few rows    (K' + 4) 2^-23 (S + |bias| + |res| + |old|), K' = taps * Cin: sixteen fp32 partial chains met in slice order, bias, residual, old
              output.  Kept for tanh-GELU (slope < 1.13, tanhf a few ulp of a value no larger than the sum).  With an ELU on an fp32 input the
              operand itself carries the exp's error: + 2^-21 sum |w| over the taps that reach the output row (the plain bound has exact operands).
  generic     the same form (one fp32 FMA chain per output is inside it); bf16 outputs add 2^-8 |ref|.
  MFMA        2^-8 |ref| for the stored bf16 + (K Cin + 4) u24 S: exact bf16 products accumulated in fp32 in the matrix core's order.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _mimi_ref as R
from _util import report

pytestmark = pytest.mark.gpu

SENT = -512.0  # exact in bf16; no output here comes near it
U24, U23 = 2.0**-24, 2.0**-23
F32, BF16 = 0, 1
ACT_NONE, ACT_GELU_TANH, ACT_ELU = 0, 4, 5
GENERIC, FEW_ROWS, MFMA = 0, 1, 2
COUT1_F32, COUT1_BF16, COUT1_STAGED = 0, 1, 2
CARRY_SHIFT, CARRY_EDGE_FILL, CARRY_EDGE_FILL_ROWS, CARRY_SHIFT_ROWS, CARRY_RESET_ROW, CARRY_SET_ACTIVE = range(6)


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rup(a, b):
    return (a + b - 1) // b * b


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def dev(a, dtype=F32):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).to(tdt(dtype)).cuda()


def i32(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def host(t):
    return t.float().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def embed(vals, rows, ld, fill=np.nan):
    """vals [B][r][c] -> [B][rows][ld] float32 with `fill` outside."""
    B, r, c = vals.shape
    buf = np.full((B, rows, ld), fill, np.float32)
    buf[:, :r, :c] = vals
    return buf


def only_inside(buf, r, c, fill=SENT):
    """Everything of buf [B][rows][ld] outside [:, :r, :c] still holds the fill."""
    m = np.ones(buf.shape, bool)
    m[:, :r, :c] = False
    return bool(np.all(buf[m] == fill))


def values(rng, shape, dtype, elu=False):
    """Operands as the kernel reads them, float32.  For an ELU'd input: half positive, the negatives from [-4, -1/16] (where the device exp's
    error is far below the tie margin), and bf16 inputs moved off the ties of bf16(elu(x))."""
    if elu:
        v = np.where(rng.random(shape) < 0.5, np.abs(rng.standard_normal(shape)) + 0.01, -rng.uniform(1 / 16, 4, shape)).astype(np.float32)
    else:
        v = rng.standard_normal(shape).astype(np.float32)
    if dtype == BF16:
        v = R.bf16_round(v)
        if elu:
            v = R.avoid_elu_ties(v)
    return v


def ratio(got, ref, bound):
    assert np.isfinite(got).all(), "non-finite output (a NaN pad element leaked)"
    return float((np.abs(got.astype(np.float64) - ref) / (bound + 1e-300)).max())


# ------------------------------------------------------------------------------------------------ rvq_sum (bits)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Nf", [1, 3])
@pytest.mark.parametrize("qdim", [32, 300])
@pytest.mark.parametrize("nq", [1, 2, 4])
def test_rvq_sum(lib, nq, qdim, Nf, dtype):
    rng = np.random.default_rng(nq * 1000 + qdim + Nf)
    B, bins = 2, 5
    ld = rup(qdim, 64) if dtype == BF16 else qdim + 4  # bf16: the codec's 64-multiple pitch (64, 320), above qdim
    cb = rng.standard_normal((nq, bins, qdim)).astype(np.float32)
    codes = rng.integers(0, bins, (B, nq, Nf))
    codes[0, 0, 0], codes[1, nq - 1, Nf - 1] = -1, bins  # clamp to 0 and bins - 1
    q1 = torch.full((B, Nf, ld), SENT, dtype=tdt(dtype), device="cuda")
    q2 = torch.full((B, Nf, ld), SENT, dtype=tdt(dtype), device="cuda")
    cbd, cd = dev(cb), i32(codes)
    rc = lib.kk_op_mimi_rvq_sum(stream(), B, P(cd), P(cbd), nq, bins, qdim, Nf, ld, P(q1), P(q2), dtype)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g1, g2 = host(q1), host(q2)
    assert only_inside(g1, Nf, qdim) and only_inside(g2, Nf, qdim), "pad columns written"
    for b in range(B):
        first, rest = R.rvq_sum(codes[b], cb)
        if dtype == BF16:
            first, rest = R.bf16_round(first), R.bf16_round(rest)
        assert same_bits(g1[b, :, :qdim], first) and same_bits(g2[b, :, :qdim], rest), f"item {b}"
    if nq == 1:
        assert not g2[:, :, :qdim].any()
    report(f"mimi_kernels/rvq_sum nq{nq} q{qdim} Nf{Nf} dt{dtype}", bits_equal=True)


# ------------------------------------------------------------------------------------------------ upsample_dw (bits)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Lin", [1, 2, 5])
@pytest.mark.parametrize("Cc", [8, 300])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_upsample_dw(lib, s, Cc, Lin, dtype):
    rng = np.random.default_rng(s * 100 + Cc + Lin)
    B = 2
    ld = rup(Cc, 64) if dtype == BF16 else Cc + 4
    x = values(rng, (B, Lin, Cc), dtype)
    w = rng.standard_normal((2 * s, Cc)).astype(np.float32)
    # item pitch (Lin + 1) * ld as when reading a state buffer: the row before item 1 (row Lin of item 0) holds NaN, so t = 0 may not read it
    xd = dev(embed(x, Lin + 1, ld), dtype)
    out = torch.full((B, Lin * s, ld), SENT, dtype=tdt(dtype), device="cuda")
    wd = dev(w)
    rc = lib.kk_op_mimi_upsample(stream(), B, P(xd), (Lin + 1) * ld, P(wd), Cc, ld, Lin, s, P(out), dtype)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g = host(out)
    assert only_inside(g, Lin * s, Cc), "pad columns written"
    for b in range(B):
        ref = R.upsample_dw(x[b], w, s)
        if dtype == BF16:
            ref = R.bf16_round(ref)
        assert same_bits(g[b, :, :Cc], ref), f"item {b}"
    report(f"mimi_kernels/upsample s{s} C{Cc} L{Lin} dt{dtype}", bits_equal=True)


# ------------------------------------------------------------------------------------------------ rope
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("T", [1, 5])
def test_rope(lib, T, heads, dtype):
    rng = np.random.default_rng(T * 10 + heads)
    B, hd = 2, 64
    D = heads * hd
    ld = 3 * D + (64 if dtype == BF16 else 4)
    inv = (10000.0 ** (-np.arange(hd // 2, dtype=np.float64) / (hd // 2))).astype(np.float32)
    x = values(rng, (B, T, 3 * D), dtype)
    buf = embed(x, T, ld)
    qkv = dev(buf, dtype)
    before = qkv.clone()
    invd = dev(inv)
    rc = lib.kk_op_mimi_rope(stream(), B, T, D, ld, hd, P(invd), P(qkv), dtype)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g = host(qkv)
    assert same_bits(g[:, :, 2 * D :], host(before)[:, :, 2 * D :]), "the v third or a pad column changed"
    worst = 0.0
    for b in range(B):
        for t in range(T):
            ref, scale = R.rope(x[b, t], inv, t, D, hd)
            bound = 8 * U23 * scale[: 2 * D] + (2.0**-8 * np.abs(ref[: 2 * D]) if dtype == BF16 else 0.0)
            worst = max(worst, ratio(g[b, t, : 2 * D], ref[: 2 * D], bound))
    report(f"mimi_kernels/rope T{T} h{heads} dt{dtype}", ratio=worst)
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ SEANet's last conv (Cout = 1)
COUT1_FORMS = [
    # id, dtype, Cin, ld, expected form
    ("f32_C12", F32, 12, 16, COUT1_F32),
    ("staged_C8", BF16, 8, 16, COUT1_STAGED),
    ("staged_C64", BF16, 64, 72, COUT1_STAGED),
    ("vector_C72", BF16, 72, 80, COUT1_BF16),  # Cin > 64: conv_cout1_kernel<bf16_t>, 16-byte vector inner loop
    ("scalar_C12", BF16, 12, 16, COUT1_BF16),  # Cin % 8 != 0: its scalar inner loop
    ("scalar_C8_ld12", BF16, 8, 12, COUT1_BF16),  # ld % 8 != 0: scalar as well
]


@pytest.mark.parametrize("elu", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 7, 16])
@pytest.mark.parametrize("form", COUT1_FORMS, ids=[f[0] for f in COUT1_FORMS])
def test_conv_cout1(lib, form, K, elu):
    name, dtype, Cin, ld, want = form
    rng = np.random.default_rng(K * 100 + Cin + elu)
    B, ldw = 2, 64
    w = (rng.standard_normal((K, Cin)) * 0.5).astype(np.float32)
    wp = np.full((K, Cin, ldw), np.nan, np.float32)
    wp[:, :, 0] = w
    wd = dev(wp)
    bias = np.float32(0.37)
    bd = dev([bias])
    worst = 0.0
    # (L, pad, bias): every L causal with and without bias in turn; one non-causal pad at 257 and 600, where rows >= L are met past a block edge
    runs = [(L, K - 1, i % 2 == 0) for i, L in enumerate([1, 255, 256, 257, 600])] + [(257, K // 2, True), (600, 0, False), (256, K - 1, False)]
    for L, pad, has_b in runs:
        x = values(rng, (B, L, Cin), dtype, elu=bool(elu))
        guard = 16 * ld  # NaN rows before item 0 and behind the last item
        flat = np.full(guard + B * L * ld + guard, np.nan, np.float32)
        flat[guard : guard + B * L * ld] = embed(x, L, ld).reshape(-1)
        xd = dev(flat, dtype)
        xv = xd[guard : guard + B * L * ld]
        out = torch.full((B * L + 8,), SENT, device="cuda")
        fm = C.c_int(-9)
        rc = lib.kk_op_mimi_conv_cout1(stream(), B, P(xv), dtype, ld, L, Cin, K, pad, P(wd), ldw, P(bd) if has_b else None, elu, P(out), C.byref(fm))
        assert rc == 0, lib.kk_last_error()
        torch.cuda.synchronize()
        assert fm.value == want, f"{name}: form {fm.value}, expected {want}"
        g = host(out)
        assert np.all(g[B * L :] == SENT), "write past the output"
        for b in range(B):
            if not elu:
                op, extra = x[b].astype(np.float64), 0.0
            elif want == COUT1_STAGED:
                op, extra = R.bf16_round(R.elu(x[b]).astype(np.float32)).astype(np.float64), 0.0
            else:
                op, extra = R.elu(x[b]), 2.0**-21 * np.abs(w).sum()
            ref, ab = R.conv_cout1(op, w, bias if has_b else None, pad=pad)
            bound = (K * Cin + 2) * U24 * ab + extra
            worst = max(worst, ratio(g[b * L : (b + 1) * L], ref, bound))
    report(f"mimi_kernels/cout1 {name} K{K} elu{elu}", ratio=worst)
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ edge_pad (bits)
@pytest.mark.parametrize("L,Cc", [(1, 8), (4, 300), (7, 8)])
def test_edge_pad(lib, L, Cc):
    rng = np.random.default_rng(L + Cc)
    B, left = 2, 2
    Lp = left + L + 3
    x = rng.standard_normal((B, L, Cc)).astype(np.float32)
    xd = dev(x)
    out = torch.full((B * Lp * Cc + 8,), SENT, device="cuda")
    rc = lib.kk_op_mimi_edge_pad(stream(), B, P(xd), L, Cc, left, Lp, P(out))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g = host(out)
    assert np.all(g[B * Lp * Cc :] == SENT)
    for b in range(B):
        assert same_bits(g[: B * Lp * Cc].reshape(B, Lp, Cc)[b], R.edge_pad(x[b], left, Lp))
    report(f"mimi_kernels/edge_pad L{L} C{Cc}", bits_equal=True)


# ------------------------------------------------------------------------------------------------ rvq_argmin (bits)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("qdim", [32, 300])
@pytest.mark.parametrize("bins", [5, 64, 300, 2048])
def test_rvq_argmin(lib, bins, qdim, T):
    rng = np.random.default_rng(bins + qdim + T)
    B, nq, cbi = 2, 3, 1
    cb = rng.standard_normal((bins, qdim)).astype(np.float32)
    # identical code-book rows.  Small code books: two of them on different threads (the reduction's tie rule); from 300 bins on also 256
    # apart, on ONE thread (its own scan's rule), and 1024 apart at 2048
    j1 = 1
    twins = [3] if bins <= 64 else ([j1 + 256] if bins == 300 else [j1 + 256, j1 + 1024, 7])
    for j in twins:
        cb[j] = cb[j1]
    c2 = ((cb.astype(np.float64) ** 2).sum(-1) / 2).astype(np.float32)
    res = rng.standard_normal((B, T, qdim)).astype(np.float32)
    dots = (res.astype(np.float64) @ cb.T.astype(np.float64)).astype(np.float32)
    dots[0, 0, [j1] + twins] = np.float32(np.abs(dots[0, 0]).max() + c2.max() + 10.0)  # row (0, 0): the twins tie for the minimum
    dots[0, 0, 0] = np.nan
    v = c2 - dots[1, 0]
    dots[1, 0, int(np.argmin(v))] = np.nan  # row (1, 0): its best distance is NaN and is skipped
    dots[B - 1, T - 1, :] = np.nan  # the last row: every distance NaN (for T = 1 this replaces the row above)
    codes = torch.full((B, nq, T), -7, dtype=torch.int32, device="cuda")
    dd, c2d, cbd, rd = dev(dots), dev(c2), dev(cb), dev(res)
    rc = lib.kk_op_mimi_rvq_argmin(stream(), B, P(dd), P(c2d), P(cbd), bins, qdim, T, nq, cbi, P(rd), P(codes))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    gc, gr = codes.cpu().numpy(), host(rd)
    assert np.all(gc[:, [0, 2], :] == -7), "a code outside (b, cbi, t) was written"
    for b in range(B):
        rcodes, rres = R.rvq_argmin(dots[b], c2, cb, res[b])
        assert np.array_equal(gc[b, cbi], rcodes), (b, gc[b, cbi], rcodes)
        assert same_bits(gr[b], rres), f"item {b}: residual"
    assert gc[0, cbi, 0] == j1 and gc[B - 1, cbi, T - 1] == bins - 1
    report(f"mimi_kernels/rvq_argmin bins{bins} q{qdim} T{T}", bits_equal=True)


# ------------------------------------------------------------------------------------------------ carry kernels (bits)
def carry(lib, op, B, bufs=(), S=(), n=(), Cc=(), pitch=(), table=None, active=None, pos=None, F=1, pos_step=0, row=0, mask=0):
    nb = len(bufs)
    return lib.kk_op_mimi_carry(stream(), op, B, nb, (C.c_void_p * max(nb, 1))(*[b.data_ptr() for b in bufs]), (C.c_int * max(nb, 1))(*S),
                                (C.c_int * max(nb, 1))(*n), (C.c_int * max(nb, 1))(*Cc), (C.c_longlong * max(nb, 1))(*pitch), P(table), P(active),
                                P(pos), F, pos_step, row, mask)


@pytest.mark.parametrize("S,n,Cc", [(6, 1, 8), (2, 5, 8), (8, 3, 1024), (1, 1, 300)], ids=["overlap", "n_ge_S", "8192_exactly", "one_row"])
def test_state_shift(lib, S, n, Cc):
    rng = np.random.default_rng(S * 10 + n)
    B, rows = 2, S + n + 1  # the pitch of a stream's largest step: one row more than this step uses
    x = rng.standard_normal((B, rows, Cc)).astype(np.float32)
    buf = dev(x)
    rc = carry(lib, CARRY_SHIFT, B, [buf], [S], [n], [Cc], [rows * Cc])
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g = host(buf)
    for b in range(B):
        assert same_bits(g[b], R.state_shift(x[b], S, n)), f"item {b}"
    report(f"mimi_kernels/state_shift S{S} n{n} C{Cc}", bits_equal=True)


def test_state_shift_refused_above_8192(lib):
    S, n, Cc, B = 9, 1, 1024, 1
    buf = torch.full((B, S + n, Cc), SENT, device="cuda")
    assert carry(lib, CARRY_SHIFT, B, [buf], [S], [n], [Cc], [(S + n) * Cc]) != 0
    assert b"larger than the shift kernel takes" in lib.kk_last_error()
    torch.cuda.synchronize()
    assert np.all(host(buf) == SENT)


def test_state_edge_fill(lib):
    rng = np.random.default_rng(3)
    B, S, n, Cc = 2, 3, 2, 16
    x = rng.standard_normal((B, S + n + 1, Cc)).astype(np.float32)
    buf = dev(x)
    rc = carry(lib, CARRY_EDGE_FILL, B, [buf], [S], [n], [Cc], [(S + n + 1) * Cc])
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    for b in range(B):
        assert same_bits(host(buf)[b], R.state_edge_fill(x[b], S))
    report("mimi_kernels/state_edge_fill", bits_equal=True)


def test_row_mode_carry(lib):
    """Four rows, mask 0b1101 (bit b is row b: rows 0, 2, 3 active, row 1 inactive), positions [0, 0, 5, 0]: the 'edge' fill reaches rows 0 and 3 only; the masked carry moves the
    active rows of BOTH buffers of the table and advances each active row's position once; the reset touches one row."""
    rng = np.random.default_rng(9)
    B, Fr, step = 4, 2, 4
    specs = [(2, 2, 8), (3, 1, 4)]  # S, rows per code frame, C
    xs = [rng.standard_normal((B, S + Fr * npf + 1, Cc)).astype(np.float32) for S, npf, Cc in specs]
    bufs = [dev(x) for x in xs]
    pitches = [x.shape[1] * x.shape[2] for x in xs]
    Sv, nv, Cv = [s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs]
    active = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    pos0 = np.array([0, 0, 5, 0], np.int32)
    pos = i32(pos0)
    table = torch.zeros(len(specs) * 32, dtype=torch.uint8, device="cuda")
    mask = 0b1101
    act = [1, 0, 1, 1]
    assert carry(lib, CARRY_SET_ACTIVE, B, active=active, mask=mask) == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    assert active.cpu().tolist() == act
    # the per-row edge fill on buffer 0 (n = this step's rows)
    assert carry(lib, CARRY_EDGE_FILL_ROWS, B, [bufs[0]], [Sv[0]], [Fr * nv[0]], [Cv[0]], [pitches[0]], active=active, pos=pos) == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    exp0 = xs[0].copy()
    for b in (0, 3):
        exp0[b] = R.state_edge_fill(xs[0][b], Sv[0])
    assert same_bits(host(bufs[0]), exp0), "edge fill: an inactive row or a row past position 0 changed, or an active one did not"
    assert np.array_equal(pos.cpu().numpy(), pos0)
    # the masked carry over the table
    rc = carry(lib, CARRY_SHIFT_ROWS, B, bufs, Sv, nv, Cv, pitches, table=table, active=active, pos=pos, F=Fr, pos_step=step)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    exp = [exp0, xs[1].copy()]
    for i, (S, npf, _) in enumerate(specs):
        for b in range(B):
            if act[b]:
                exp[i][b] = R.state_shift(exp[i][b], S, Fr * npf)
        assert same_bits(host(bufs[i]), exp[i]), f"buffer {i}"
    pos1 = pos0 + step * np.array(act, np.int32)
    assert np.array_equal(pos.cpu().numpy(), pos1), "positions: once per active row, not once per buffer"
    # reset of row 2
    rc = carry(lib, CARRY_RESET_ROW, B, bufs, Sv, nv, Cv, pitches, table=table, active=active, pos=pos, F=Fr, row=2)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    for i, (S, _, _) in enumerate(specs):
        exp[i][2, :S] = 0
        assert same_bits(host(bufs[i]), exp[i]), f"reset: buffer {i}"
    pos1[2] = 0
    assert np.array_equal(pos.cpu().numpy(), pos1)
    report("mimi_kernels/row_mode_carry", bits_equal=True)


# ------------------------------------------------------------------------------------------------ kk_op_mimi_conv
def pack_generic(w_oki):
    """[O][K][I] -> [K][I][ldw] fp32, NaN in the unused columns (ldw = O rounded up to 64, + 4 so that there always are some)."""
    O_, K, I = w_oki.shape
    ldw = rup(O_, 64) + 4
    p = np.full((K, I, ldw), np.nan, np.float32)
    p[:, :, :O_] = np.transpose(w_oki, (1, 2, 0))
    return p, ldw


def pack_frag(lib, w_oki):
    """The bf16 pack [K][CoutP][CinP] re-laid in fragment order on the device (kk_op_pack_w_frag).  Input-channel padding is zero (the kernel
    masks x there and 0 * w must be 0); the rows of the unused output channels hold NaN."""
    O_, K, I = w_oki.shape
    CinP, CoutP = rup(I, 64), rup(O_, 128)
    p = np.zeros((K, CoutP, CinP), np.float32)
    p[:, O_:, :] = np.nan
    p[:, :O_, :I] = np.transpose(w_oki, (1, 0, 2))
    wd = torch.tensor(p).to(torch.bfloat16).cuda()
    wf = torch.empty_like(wd)
    rc = lib.kk_op_pack_w_frag(stream(), P(wd), P(wf), K, CoutP, CinP)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return wf, CinP, CoutP


def run_conv(lib, x, w, bias=None, *, xdt=F32, odt=F32, ldx=None, ldo=None, xrows_pitch=None, out_rows, pad=0, dil=1, transposed=False, stride=1,
             in_act=0, act=0, res=None, ldr=None, old=None, frag=False, elu_scratch=True, want=None):
    """kk_op_mimi_conv on x [B][x_rows][Cin] (values as the kernel reads them) -> (out [B][rows_pitch][ldo] as float32 host array, path).
    res / old [B][out_rows][Cout]: the residual (pitch ldr) and the previous output (accumulate)."""
    B, x_rows, Cin = x.shape
    O_, K, _ = w.shape
    ldx = ldx or Cin
    ldo = ldo or O_
    xp = xrows_pitch or x_rows
    op = out_rows + 1  # one sentinel row behind every item
    xd = dev(embed(x, xp, ldx), xdt)
    if old is not None:
        outd = dev(embed(old, op, ldo, fill=SENT), odt)
    else:
        outd = torch.full((B, op, ldo), SENT, dtype=tdt(odt), device="cuda")
    resd = dev(embed(res, out_rows + 2, ldr), odt) if res is not None else None
    wp, ldw = pack_generic(w)
    wd = dev(wp)
    wf, CinP, CoutP = (None, 0, 0)
    if frag:
        wf, CinP, CoutP = pack_frag(lib, w)
    nb = CoutP if frag else O_
    bd = None
    if bias is not None or frag:
        bv = np.full(nb, np.nan, np.float32)
        bv[:O_] = bias if bias is not None else 0.0
        bd = dev(bv)
    scratch = torch.full((B * xp * ldx,), np.nan, device="cuda") if (in_act == ACT_ELU and elu_scratch and xdt == F32) else None
    path = C.c_int(-9)
    rc = lib.kk_op_mimi_conv(stream(), B, P(xd), xp * ldx, ldx, x_rows, xdt, P(wd), ldw, P(wf), CinP, CoutP, P(bd), Cin, O_, K, pad, dil,
                             int(transposed), stride, in_act, act, P(resd), (out_rows + 2) * (ldr or 0), ldr or 0, int(old is not None), P(outd),
                             op * ldo, ldo, out_rows, odt, P(scratch), scratch.numel() if scratch is not None else 0, C.byref(path))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    if want is not None:
        assert path.value == want, f"dispatch took path {path.value}, the case is about path {want}"
    return host(outd), path.value


def conv_ref(x, w, bias, *, out_rows, pad=0, dil=1, transposed=False, stride=1, in_act=0, act=0, res=None, old=None, path=GENERIC, xdt=F32, odt=F32):
    """-> (ref [B][out_rows][Cout] float64, bound) for one call of run_conv, by the docstring's bounds."""
    B, _, Cin = x.shape
    O_, K, _ = w.shape
    w64 = (R.bf16_round(w) if path == MFMA else w).astype(np.float64)
    taps = -(-K // stride) if transposed else K
    refs, bounds = [], []
    for b in range(B):
        xb = x[b].astype(np.float64)
        extra = 0.0
        if in_act == ACT_ELU:
            if path == MFMA:
                xb = R.bf16_round(R.elu(xb).astype(np.float32)).astype(np.float64)
            else:
                xb = R.elu(xb)
        if transposed:
            both = lambda v: R.conv_transposed(v, w64, None, stride=stride, pad=pad, Lout=out_rows, absum=True)  # noqa: E731
        else:
            both = lambda v: R.conv(v, w64, None, pad=pad, dil=dil, stride=stride, Lout=out_rows, absum=True)  # noqa: E731
        o, ab = both(xb)
        if in_act == ACT_ELU and path != MFMA:
            extra = 2.0**-21 * both(np.ones_like(xb))[1]  # sum |w| over the taps that reach each output row (two per row when transposed)
        scale = ab.copy()
        if bias is not None:
            o = o + bias.astype(np.float64)[None, :]
            scale += np.abs(bias)[None, :]
        if act == ACT_GELU_TANH:
            o = R.gelu_tanh(o)
        if res is not None:
            o = o + res[b]
            scale += np.abs(res[b])
        if old is not None:
            o = o + old[b]
            scale += np.abs(old[b])
        if path == MFMA:
            bound = 2.0**-8 * np.abs(o) + (K * Cin + 4) * U24 * ab
        else:
            bound = (taps * Cin + 4) * U23 * scale + extra + (2.0**-8 * np.abs(o) if odt == BF16 else 0.0)
        refs.append(o)
        bounds.append(bound)
    return np.stack(refs), np.stack(bounds)


def check_conv(lib, name, x, w, bias, *, want, out_rows, first_row=0, **kw):
    """Run, compare rows [first_row, out_rows) with the reference, the rest of the buffer with the sentinel; report; -> the output."""
    refkw = {k: kw[k] for k in ("pad", "dil", "transposed", "stride", "in_act", "act", "res", "old", "xdt", "odt") if k in kw}
    g, path = run_conv(lib, x, w, bias, out_rows=out_rows, want=want, **kw)
    O_ = w.shape[0]
    ref, bound = conv_ref(x, w, bias, out_rows=out_rows, path=path, **refkw)
    assert np.all(g[:, out_rows:, :] == SENT) and np.all(g[:, :, O_:] == SENT), "write outside the output rows / channels"
    if first_row and kw.get("old") is None:
        assert np.all(g[:, :first_row, :] == SENT), "the rows the few-rows transposed form leaves alone were written"
    worst = ratio(g[:, first_row:out_rows, :O_], ref[:, first_row:], bound[:, first_row:])
    report(f"mimi_kernels/conv {name}", ratio=worst, path=path)
    assert worst <= 1.0, worst
    return g


def rnd_w(rng, O_, K, I):
    return (rng.standard_normal((O_, K, I)) * 0.5).astype(np.float32)


# (B, rows): M = B * rows in {1, 4, 5, 8, 9, 16, 17}: linear_rows_kernel<4>, <8> and <16> with full and ragged last blocks
LR_M = [(1, 1), (2, 2), (1, 5), (2, 4), (3, 3), (2, 8), (1, 17)]


@pytest.mark.parametrize("Brows", LR_M, ids=[f"M{b * r}" for b, r in LR_M])
@pytest.mark.parametrize("Cin,N", [(8, 32), (20, 40), (136, 48)])
def test_few_rows_linear(lib, Cin, N, Brows):
    """K' = Cin below 16 (8: most k-slices are empty), not a multiple of 16 * 8 (20, 136), N not a multiple of 16 (40).  Epilogue by case:
    Cin 8: bias + tanh-GELU (small K' keeps the bound tight enough to see the GELU's constants); Cin 20: bias + GELU + residual of another pitch;
    Cin 136: bias + residual + accumulate."""
    B, rows = Brows
    rng = np.random.default_rng(Cin * 100 + B * rows)
    x, w, bias = values(rng, (B, rows, Cin), F32), rnd_w(rng, N, 1, Cin), rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((B, rows, N)).astype(np.float32) if Cin != 8 else None
    old = rng.standard_normal((B, rows, N)).astype(np.float32) if Cin == 136 else None
    act = ACT_GELU_TANH if Cin != 136 else ACT_NONE
    check_conv(lib, f"few_rows linear C{Cin} N{N} M{B * rows}", x, w, bias, want=FEW_ROWS, out_rows=rows, act=act, res=res, ldr=N + 4, old=old, ldo=N + 4)


@pytest.mark.parametrize("elu", [0, 1])
@pytest.mark.parametrize("K", [3, 7])
def test_few_rows_causal_conv(lib, K, elu):
    """The flattened causal conv over rows + K - 1 contiguous rows; with the ELU pre-pass the input's item pitch differs from rows * ld."""
    rng = np.random.default_rng(K + elu)
    B, rows, Cin, N = 2, 2, 8, 32
    x, w, bias = values(rng, (B, rows + K - 1, Cin), F32, elu=bool(elu)), rnd_w(rng, N, K, Cin), rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((B, rows, N)).astype(np.float32)
    check_conv(lib, f"few_rows conv K{K} elu{elu}", x, w, bias, want=FEW_ROWS, out_rows=rows, in_act=ACT_ELU * elu, res=res, ldr=N,
               xrows_pitch=rows + K + 1)


@pytest.mark.parametrize("xrows", [2, 3])
@pytest.mark.parametrize("stride", [2, 4, 5])
def test_few_rows_transposed(lib, stride, xrows):
    """Polyphase transposed conv K = 2 stride over [previous | new] input rows: output rows [0, stride) keep the sentinel."""
    rng = np.random.default_rng(stride * 10 + xrows)
    B, Cin, N = 2, 16, 32
    x, w = values(rng, (B, xrows, Cin), F32, elu=True), rnd_w(rng, N, 2 * stride, Cin)
    bias = rng.standard_normal(N).astype(np.float32)
    check_conv(lib, f"few_rows transposed s{stride} rows{xrows}", x, w, bias, want=FEW_ROWS, out_rows=xrows * stride, first_row=stride,
               transposed=True, stride=stride, in_act=ACT_ELU, xrows_pitch=xrows + 1)


def test_few_rows_transposed_with_res_or_accumulate_goes_generic(lib):
    rng = np.random.default_rng(77)
    B, Cin, N, stride, xrows = 2, 16, 32, 2, 3
    x, w = values(rng, (B, xrows, Cin), F32), rnd_w(rng, N, 2 * stride, Cin)
    extra = rng.standard_normal((B, xrows * stride, N)).astype(np.float32)
    check_conv(lib, "transposed + res -> generic", x, w, None, want=GENERIC, out_rows=xrows * stride, transposed=True, stride=stride, res=extra, ldr=N)
    check_conv(lib, "transposed + accumulate -> generic", x, w, None, want=GENERIC, out_rows=xrows * stride, transposed=True, stride=stride, old=extra)
    # and without scratch an ELU'd few-rows shape is the generic kernel's
    check_conv(lib, "few-rows shape, ELU without scratch -> generic", values(rng, (B, xrows, Cin), F32, elu=True), rnd_w(rng, N, 1, Cin), None,
               want=GENERIC, out_rows=xrows, in_act=ACT_ELU, elu_scratch=False)


def test_few_rows_batch_invariance(lib):
    """An item's rows at B = 3 (M = 9: the <16> instantiation) equal the same item alone (M = 3: <4>) bit for bit."""
    rng = np.random.default_rng(5)
    B, rows, Cin, N = 3, 3, 136, 48
    x, w, bias = values(rng, (B, rows, Cin), F32), rnd_w(rng, N, 1, Cin), rng.standard_normal(N).astype(np.float32)
    g3, _ = run_conv(lib, x, w, bias, out_rows=rows, act=ACT_GELU_TANH, want=FEW_ROWS)
    for b in range(B):
        g1, _ = run_conv(lib, x[b : b + 1], w, bias, out_rows=rows, act=ACT_GELU_TANH, want=FEW_ROWS)
        assert same_bits(g3[b], g1[0]), f"item {b}"
    report("mimi_kernels/conv few_rows batch invariance", bits_equal=True)


@pytest.mark.parametrize("odt", [F32, BF16], ids=["f32out", "bf16out"])
def test_generic_elu_first_conv(lib, odt):
    """The ELU template of the generic tile at Cin = 1 (the encoder's first conv shape, K = 7, causal)."""
    rng = np.random.default_rng(11)
    B, L, N, K = 2, 70, 8, 7
    x, w, bias = values(rng, (B, L, 1), F32, elu=True), rnd_w(rng, N, K, 1), rng.standard_normal(N).astype(np.float32)
    check_conv(lib, f"generic ELU Cin1 K7 odt{odt}", x, w, bias, want=GENERIC, out_rows=L, pad=K - 1, in_act=ACT_ELU, odt=odt, ldo=N + 8, ldx=4)


@pytest.mark.parametrize("xdt,odt", [(F32, F32), (BF16, BF16)], ids=["f32", "bf16"])
@pytest.mark.parametrize("r", [4, 5])
def test_generic_strided_causal_conv(lib, r, xdt, odt):
    """The encoder's down-sampling: K = 2 r, stride r, left pad K - r, L not a multiple of r (the last window runs into zero rows)."""
    rng = np.random.default_rng(r)
    B, L, Cin, N = 2, 37, 12, 20
    x, w, bias = values(rng, (B, L, Cin), xdt, elu=True), rnd_w(rng, N, 2 * r, Cin), rng.standard_normal(N).astype(np.float32)
    check_conv(lib, f"generic strided r{r} dt{xdt}", x, w, bias, want=GENERIC, out_rows=-(-L // r), pad=r, stride=r, in_act=ACT_ELU, xdt=xdt, odt=odt,
               ldx=16, ldo=24)


@pytest.mark.parametrize("xdt,odt", [(F32, F32), (BF16, BF16), (F32, BF16)], ids=["f32", "bf16", "f32_to_bf16"])
def test_generic_transposed_many_rows(lib, xdt, odt):
    """K = 2 stride transposed at more than 128 input rows (past the few-rows kernel), Cout < 32."""
    rng = np.random.default_rng(13)
    B, L, Cin, N, s = 2, 140, 12, 24, 2
    x, w, bias = values(rng, (B, L, Cin), xdt, elu=True), rnd_w(rng, N, 2 * s, Cin), rng.standard_normal(N).astype(np.float32)
    check_conv(lib, f"generic transposed L{L} dt{xdt}{odt}", x, w, bias, want=GENERIC, out_rows=L * s, transposed=True, stride=s, in_act=ACT_ELU,
               xdt=xdt, odt=odt, ldx=Cin if xdt == F32 else 16, ldo=N if odt == F32 else 32)


MFMA_CASES = [
    # id, Cin, Cout, K, L (input rows), stride (0: plain conv), residual
    ("k1_16_16_L1", 16, 16, 1, 1, 0, False),
    ("k1_72_40_L5", 72, 40, 1, 5, 0, True),
    ("k1_128_64_L193", 128, 64, 1, 193, 0, False),
    ("k3_72_40_L193_res", 72, 40, 3, 193, 0, True),
    ("k3_16_64_L5", 16, 64, 3, 5, 0, False),
    ("t16s8_128_64_L5", 128, 64, 16, 5, 8, False),
    ("t12s6_72_40_L193", 72, 40, 12, 193, 6, False),
    ("t10s5_16_16_L1", 16, 16, 10, 1, 5, False),
    ("t8s4_128_40_L193", 128, 40, 8, 193, 4, False),
]


def mfma_conv(lib, name, x, w, bias, want=MFMA, **kw):
    Cin, O_ = x.shape[2], w.shape[0]
    return check_conv(lib, name, x, w, bias, want=want, xdt=BF16, odt=BF16, frag=True, ldx=kw.pop("ldx", rup(Cin, 64)), ldo=rup(O_, 64), **kw)


@pytest.mark.parametrize("case", MFMA_CASES, ids=[c[0] for c in MFMA_CASES])
def test_mfma_elu(lib, case):
    """in_act = ELU on the variant-4 staging (elu(x) rounded to bf16): K = 1, K = 3 causal, and the causal transposed conv K = 2 stride with
    Lout = Lin * stride at the decoder's four ratios; with the block's skip as residual."""
    name, Cin, N, K, L, s, with_res = case
    rng = np.random.default_rng(Cin + N + K + L)
    B = 2
    x, w, bias = values(rng, (B, L, Cin), BF16, elu=True), rnd_w(rng, N, K, Cin), rng.standard_normal(N).astype(np.float32)
    Lo = L * s if s else L
    res = R.bf16_round(rng.standard_normal((B, Lo, N)).astype(np.float32)) if with_res else None
    mfma_conv(lib, f"mfma {name}", x, w, bias, out_rows=Lo, pad=0 if s else K - 1, transposed=bool(s), stride=s or 1, in_act=ACT_ELU, res=res,
              ldr=rup(N, 64) + 64)


@pytest.mark.parametrize("L", [5, 193])
def test_mfma_accumulate(lib, L):
    """accumulate = 1 on the MFMA path (proj_rest into x0): K = 1, no bias."""
    rng = np.random.default_rng(L)
    B, Cin, N = 2, 72, 64
    x, w = values(rng, (B, L, Cin), BF16), rnd_w(rng, N, 1, Cin)
    old = R.bf16_round(rng.standard_normal((B, L, N)).astype(np.float32))
    mfma_conv(lib, f"mfma accumulate L{L}", x, w, None, out_rows=L, old=old)


def test_mfma_not_taken_falls_to_generic(lib):
    """With a fragment pack at hand, what the MFMA kernel does not take is the generic kernel's: Cout not a multiple of 8, an input pitch below
    CinP, a strided plain conv."""
    rng = np.random.default_rng(21)
    B, L = 2, 5
    x, w = values(rng, (B, L, 72), BF16, elu=True), rnd_w(rng, 20, 1, 72)
    mfma_conv(lib, "mfma refused: Cout 20", x, w, None, want=GENERIC, out_rows=L, in_act=ACT_ELU)
    w = rnd_w(rng, 40, 1, 72)
    mfma_conv(lib, "mfma refused: ldx 80 < CinP 128", x, w, None, want=GENERIC, out_rows=L, in_act=ACT_ELU, ldx=80)
    w = rnd_w(rng, 40, 4, 72)
    mfma_conv(lib, "mfma refused: stride 2", x, w, None, want=GENERIC, out_rows=3, pad=2, stride=2, in_act=ACT_ELU)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_outputs_untouched(lib):
    """Every documented refusal returns non-zero with a message, before any launch: the sentinel outputs stay."""
    B, L, Cc = 1, 4, 32
    x = torch.zeros((B, L, Cc), device="cuda")
    xb = torch.zeros((B, L, 64), dtype=torch.bfloat16, device="cuda")
    out = torch.full((B, L, 64), SENT, device="cuda")
    outb = torch.full((B, L, 64), SENT, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((1, Cc, 64), device="cuda")
    wf = torch.zeros((1, 128, 64), dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(128, device="cuda")
    ids = torch.zeros((B, 1, L), dtype=torch.int32, device="cuda")
    codes = torch.full((B, 1, L), -7, dtype=torch.int32, device="cuda")
    path = C.c_int(0)

    def conv(**kw):
        a = dict(B=B, x=x, xbs=L * Cc, ldx=Cc, x_rows=L, xdt=F32, w=w, ldw=64, wf=None, CinP=0, CoutP=0, bias=None, Cin=Cc, Cout=Cc, K=1, pad=0, dil=1, tr=0,
                 stride=1, in_act=0, act=0, res=None, rbs=0, ldr=0, acc=0, out=out, obs=L * 64, ldo=64, out_rows=L, odt=F32, elu=None, elu_floats=0)
        a.update(kw)
        return lib.kk_op_mimi_conv(stream(), a["B"], P(a["x"]), a["xbs"], a["ldx"], a["x_rows"], a["xdt"], P(a["w"]), a["ldw"], P(a["wf"]), a["CinP"],
                                   a["CoutP"], P(a["bias"]), a["Cin"], a["Cout"], a["K"], a["pad"], a["dil"], a["tr"], a["stride"], a["in_act"], a["act"],
                                   P(a["res"]), a["rbs"], a["ldr"], a["acc"], P(a["out"]), a["obs"], a["ldo"], a["out_rows"], a["odt"], P(a["elu"]),
                                   a["elu_floats"], C.byref(path))

    class Raw:  # a device address that is no tensor's start (mis-aligned pointers)
        def __init__(self, addr):
            self.addr = addr

        def data_ptr(self):
            return self.addr

    frag = dict(wf=wf, CinP=64, CoutP=128, bias=bias)  # a valid fragment pack for Cin = Cout = 32
    frag_bf16 = dict(frag, x=xb, xdt=BF16, ldx=64, xbs=L * 64, out=outb, odt=BF16)
    bad_conv = [
        dict(B=0), dict(x=None), dict(xdt=2), dict(Cin=0), dict(pad=-1), dict(dil=0), dict(tr=1, dil=2), dict(stride=0), dict(in_act=1), dict(act=2),
        dict(ldw=62), dict(ldw=32), dict(ldx=Cc - 1), dict(ldo=Cc - 1), dict(xbs=L * Cc - 1), dict(obs=L * 64 - 1), dict(res=out, ldr=64, rbs=1),
        dict(acc=2), dict(elu=out, elu_floats=0),
        dict(in_act=ACT_ELU, elu=out, elu_floats=B * L * Cc - 1),  # few-rows shape, scratch too small
        dict(frag, CinP=32), dict(frag, CoutP=64),  # not multiples of 64 / 128
        dict(frag, CinP=0), dict(frag, CoutP=0),  # below Cin / Cout
        dict(frag, bias=None),
        dict(frag, wf=Raw(wf.data_ptr() + 2)),  # mis-aligned fragment pack
        dict(frag_bf16, ldx=36, xbs=L * 36),  # bf16 pitch not a multiple of 8
        dict(frag_bf16, res=outb, ldr=36, rbs=L * 36),  # bf16 residual pitch not a multiple of 8
        dict(frag_bf16, res=Raw(outb.data_ptr() + 2), ldr=64, rbs=L * 64),  # mis-aligned bf16 residual
    ]
    for kw in bad_conv:
        path.value = 0
        assert conv(**kw) != 0, kw
        assert lib.kk_last_error() and path.value == -1, kw
    z = torch.zeros(4096, device="cuda")
    fm = C.c_int(0)
    bad = [
        lambda: lib.kk_op_mimi_rvq_sum(stream(), B, P(ids), P(z), 1, 5, Cc, L, Cc - 1, P(out), P(out), F32),
        lambda: lib.kk_op_mimi_rvq_sum(stream(), B, P(ids), P(z), 0, 5, Cc, L, 64, P(out), P(out), F32),
        lambda: lib.kk_op_mimi_rvq_sum(stream(), B, None, P(z), 1, 5, Cc, L, 64, P(out), P(out), F32),
        lambda: lib.kk_op_mimi_rvq_sum(stream(), B, P(ids), P(z), 1, 5, Cc, L, 64, P(out), P(out), 2),  # dtype
        lambda: lib.kk_op_mimi_upsample(stream(), B, P(x), L * Cc, P(z), Cc, Cc, L, 1, P(out), 2),  # dtype
        lambda: lib.kk_op_mimi_rope(stream(), B, L, 64, 192, 64, P(z), P(out), 2),  # dtype
        lambda: lib.kk_op_mimi_upsample(stream(), B, P(x), L * Cc - 1, P(z), Cc, Cc, L, 1, P(out), F32),
        lambda: lib.kk_op_mimi_upsample(stream(), B, P(x), L * Cc, P(z), Cc, Cc, L, 0, P(out), F32),
        lambda: lib.kk_op_mimi_upsample(stream(), B, P(out), L * 64, P(z), Cc, 64, L, 1, P(out), F32),
        lambda: lib.kk_op_mimi_rope(stream(), B, L, 64, 191, 64, P(z), P(out), F32),
        lambda: lib.kk_op_mimi_rope(stream(), B, L, 96, 288, 64, P(z), P(out), F32),
        lambda: lib.kk_op_mimi_rope(stream(), B, L, 64, 192, 63, P(z), P(out), F32),
        lambda: lib.kk_op_mimi_conv_cout1(stream(), B, P(x), F32, Cc, L, Cc, 257, 0, P(z), 1, None, 0, P(out), C.byref(fm)),
        lambda: lib.kk_op_mimi_conv_cout1(stream(), B, P(x), F32, Cc - 1, L, Cc, 1, 0, P(z), 1, None, 0, P(out), C.byref(fm)),
        lambda: lib.kk_op_mimi_conv_cout1(stream(), B, P(x), F32, Cc, L, Cc, 1, 0, P(z), 1, None, 2, P(out), C.byref(fm)),
        lambda: lib.kk_op_mimi_conv_cout1(stream(), B, C.c_void_p(xb.data_ptr() + 2), BF16, 64, 2, 8, 1, 0, P(z), 1, None, 0, P(out), C.byref(fm)),
        lambda: lib.kk_op_mimi_edge_pad(stream(), B, P(x), L, Cc, -1, L, P(out)),
        lambda: lib.kk_op_mimi_edge_pad(stream(), B, P(x), 0, Cc, 0, L, P(out)),
        lambda: lib.kk_op_mimi_rvq_argmin(stream(), B, P(z), P(z), P(z), 5, Cc, L, 1, 1, P(out), P(codes)),
        lambda: lib.kk_op_mimi_rvq_argmin(stream(), B, P(z), P(z), P(z), 0, Cc, L, 1, 0, P(out), P(codes)),
        lambda: carry(lib, 6, B),
        lambda: carry(lib, CARRY_SET_ACTIVE, 65, active=codes, mask=1),
        lambda: carry(lib, CARRY_SHIFT, B, [out], [0], [1], [8], [64]),
        lambda: carry(lib, CARRY_SHIFT, B, [out], [2], [2], [8], [31]),  # pitch below (S + n) * C
        lambda: carry(lib, CARRY_SHIFT, B, [out], [2], [2], [8], [33]),  # pitch not a whole number of rows
        lambda: carry(lib, CARRY_SHIFT, B, [out], [2], [0], [8], [64]),  # n < 1
        lambda: carry(lib, CARRY_SHIFT_ROWS, B, [out], [1], [1], [8], [64], table=z, active=codes, pos=codes, F=0),
        lambda: carry(lib, CARRY_RESET_ROW, B, [out], [1], [1], [8], [64], table=z, active=codes, pos=codes, F=0, row=0),
        lambda: carry(lib, CARRY_SHIFT, B, [out, out], [1, 1], [1, 1], [8, 8], [64, 64]),
        lambda: carry(lib, CARRY_EDGE_FILL_ROWS, B, [out], [1], [1], [8], [64]),
        lambda: carry(lib, CARRY_SHIFT_ROWS, B, [out], [1], [1], [8], [64], active=codes, pos=codes),
        lambda: carry(lib, CARRY_SHIFT_ROWS, B, [out], [9], [1], [1024], [16384], table=z, active=codes, pos=codes),
        lambda: carry(lib, CARRY_RESET_ROW, B, [out], [1], [1], [8], [64], table=z, active=codes, pos=codes, row=1),
    ]
    for i, f in enumerate(bad):
        assert f() != 0, f"refusal {i} was accepted"
        assert lib.kk_last_error(), i
    torch.cuda.synchronize()
    assert np.all(host(out) == SENT) and np.all(host(outb) == SENT) and np.all(codes.cpu().numpy() == -7)
