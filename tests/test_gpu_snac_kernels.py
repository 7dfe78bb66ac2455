"""GPU parity tests of mlx-audio_amd/csrc/kk_snac.hip kernel by kernel (through kk_op_snac_*, which call the launch functions the codec calls),
against the float64 references of tests/_snac_ref.py on the operands the kernel reads (bf16 RNE where it reads bf16).
tests/test_snac_ref_cpu.py pins those references.

Every input carries NaN in its pad columns and in rows outside the valid range; every output starts as a sentinel, so a leak or a stray write
shows.  Each case reports its worst error as a fraction of its bound (report()).

Bits (the build has -ffp-contract=off; numpy float32 reproduces the kernels' operations): from_codes, the straight-through line of the search,
and every batch-invariance check.

Bounds (u = 2^-24 is the unit round-off of fp32; S = sum |x w| (+ |bias|, |res|) over the taps of an output):
  snake       e_sn(x) = 2u (ra (2 |alpha x| + 8) + |x| + ra), ra = 1 / alpha: the rounded product alpha x, sinf within 2 ulp of a value <= 1, the
              square, the reciprocal, the product and the sum, with a factor 2 of slack.  |d snake / dx| = |1 + sin(2 alpha x)| <= 2.
  depth-wise  (K + 2) u S + sum_k |w_k| e_sn(x_k) for the sum; an output Snake doubles that and adds e_sn(y); a bf16 output adds 2^-8 |ref|.
  last conv   (K Cin + 4) u S + sum |w| e_sn(x) (one FMA chain per 16 channels, met in a fixed order); tanh has slope <= 1 and adds 4 * 2^-23.
  1x1 conv    generic: (C + 4) * 2^-23 S; matrix core: 2^-8 |ref| + (C + 4) u S (exact bf16 products accumulated in fp32), as in
              test_gpu_mimi_kernels.py.
  search      distances of unit vectors: (3 cd + 20) u each (three cd-term FMA chains on operands of relative error 3u); the chosen index's
              reference distance is within twice that of the minimum, and it is the FIRST of the rows identical to it.
The residual unit is two launches with a tensor between them; in bf16 that tensor is rounded, so the second launch is compared on the tensor
the first one wrote (read back), each launch on the operands it reads -- no tie of an intermediate rounding can hide in a bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import _snac_ref as R
from _util import report

pytestmark = pytest.mark.gpu

SENT = -512.0  # exact in bf16; no output here comes near it
U24, U23 = 2.0**-24, 2.0**-23
F32, BF16 = 0, 1
GENERIC, MFMA = 0, 1


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


def host(t):
    return t.float().cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def embed(vals, rows, ld, fill=np.nan):
    B, r, c = vals.shape
    buf = np.full((B, rows, ld), fill, np.float32)
    buf[:, :r, :c] = vals
    return buf


def only_inside(buf, r, c, fill=SENT):
    m = np.ones(buf.shape, bool)
    m[:, :r, :c] = False
    return bool(np.all(buf[m] == fill))


def values(rng, shape, dtype):
    v = rng.standard_normal(shape).astype(np.float32)
    return R.bf16_round(v) if dtype == BF16 else v


def ratio(got, ref, bound):
    assert np.isfinite(got).all(), "non-finite output (a NaN pad element leaked)"
    return float((np.abs(got.astype(np.float64) - ref) / (bound + 1e-300)).max())


def e_snake(x, alpha):
    ra = 1.0 / alpha
    return 2 * U24 * (ra * (2 * np.abs(alpha * x) + 8) + np.abs(x) + ra)


def ld_of(C_, dtype):
    return rup(C_, 64) if dtype == BF16 else C_ + 4  # bf16: the codec's 64-multiple pitch; fp32: a pitch above C so that pad columns exist


# ------------------------------------------------------------------------------------------------ depth-wise conv
def run_dw(lib, x, w, b, dil, a_in, a_out, dtype, B=None):
    B_, L, C_ = x.shape
    ldx, ldo = ld_of(C_, dtype) + (64 if dtype == BF16 else 0), ld_of(C_, dtype)
    xd = dev(embed(x, L + 2, ldx), dtype)
    od = torch.full((B_, L + 1, ldo), SENT, dtype=tdt(dtype), device="cuda")
    wd, bd = dev(w.reshape(C_, 7)), dev(b)
    ai, ao = (dev(a_in) if a_in is not None else None), (dev(a_out) if a_out is not None else None)
    rc = lib.kk_op_snac_dw_conv(stream(), B_, P(xd), (L + 2) * ldx, ldx, dtype, L, C_, dil, P(wd), P(bd), P(ai), P(ao), P(od), (L + 1) * ldo, ldo)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g = host(od)
    assert only_inside(g, L, C_), "a pad column or a row past L was written"
    return g[:, :L, :C_]


def dw_bound(x, w, b, dil, a_in, a_out, dtype):
    """(reference, bound) of the depth-wise kernel on float32 operands x [B][L][C]."""
    ref, S, pre = R.dw_conv(x, w, b, dil=dil, alpha_in=a_in, alpha_out=a_out, absum=True)
    bound = 9 * U24 * S
    if a_in is not None:
        bound = bound + R.dw_conv(e_snake(x.astype(np.float64), a_in.astype(np.float64)), np.abs(w), None, dil=dil)
    if a_out is not None:
        bound = 2 * bound + e_snake(pre, a_out.astype(np.float64))
    if dtype == BF16:
        bound = bound + 2.0**-8 * np.abs(ref)
    return ref, bound


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("C_", [4, 48, 300])
def test_dw_conv(lib, C_, dil, dtype):
    rng = np.random.default_rng(C_ * 100 + dil * 10 + dtype)
    w = (rng.standard_normal((C_, 7, 1)) / np.sqrt(7)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C_)).astype(np.float32)
    a1, a2 = rng.uniform(0.5, 2, C_).astype(np.float32), rng.uniform(0.5, 2, C_).astype(np.float32)
    worst = 0.0
    for L in (1, 5, 30, 70, 200):  # 1, 5, 30: shorter than the dil-9 halo of 27 on one or both sides; 200: two row tiles
        x = values(rng, (2, L, C_), dtype)
        for a_in in (None, a1):
            for a_out in (None, a2):
                got = run_dw(lib, x, w, b, dil, a_in, a_out, dtype)
                ref, bound = dw_bound(x, w, b, dil, a_in, a_out, dtype)
                r = ratio(got, ref, bound)
                assert r <= 1.0, (L, a_in is not None, a_out is not None, r)
                worst = max(worst, r)
                one = run_dw(lib, x[1:], w, b, dil, a_in, a_out, dtype)
                assert same_bits(one[0], got[1]), "item 1 differs from its own B = 1 launch"
    report(f"snac_kernels/dw_conv/C{C_}_dil{dil}_{'bf16' if dtype else 'f32'}", worst_over_bound=worst)


def test_dw_conv_refusals(lib):
    x = torch.zeros(1, 4, 8, device="cuda")
    o = torch.zeros(1, 4, 8, device="cuda")
    w, b = torch.zeros(8, 7, device="cuda"), torch.zeros(8, device="cuda")
    ok = lambda **k: lib.kk_op_snac_dw_conv(stream(), k.get("B", 1), P(k.get("x", x)), 32, k.get("ldx", 8), k.get("dtype", 0), 4, 8, k.get("dil", 1), P(w),
                                            P(k.get("b", b)), None, None, P(k.get("o", o)), 32, 8)
    assert ok() == 0
    for bad in (dict(B=0), dict(dil=0), dict(dil=10), dict(ldx=7), dict(dtype=2), dict(o=x)):
        assert ok(**bad) != 0 and lib.kk_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ from_codes (bits)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("strides", [[4, 2, 1], [2, 1]], ids=["421", "21"])
def test_from_codes(lib, strides, T, dtype):
    rng = np.random.default_rng(T * 10 + len(strides))
    B, bins, D = 2, 37, 300
    ldo = ld_of(D, dtype)
    tables = [rng.standard_normal((bins, D)).astype(np.float32) for _ in strides]
    bias = rng.standard_normal(D).astype(np.float32)
    codes = [rng.integers(0, bins, (B, T // s)) for s in strides]
    codes[0][0, 0], codes[-1][1, -1] = -3, bins + 5  # clamped to 0 and bins - 1
    cd = [torch.tensor(c.astype(np.int32)).cuda() for c in codes]
    td = [dev(t) for t in tables]
    od = torch.full((B, T, ldo), SENT, dtype=tdt(dtype), device="cuda")
    n, bd = len(strides), dev(bias)
    rc = lib.kk_op_snac_from_codes(stream(), B, T, D, n, (C.c_void_p * n)(*[c.data_ptr() for c in cd]), (C.c_int32 * n)(*strides),
                                   (C.c_void_p * n)(*[t.data_ptr() for t in td]), bins, P(bd), P(od), ldo, dtype)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g = host(od)
    assert only_inside(g, T, D)
    acc = None
    for c, s, t in zip(codes, strides, tables):
        v = t[np.repeat(np.clip(c, 0, bins - 1), s, axis=1)]
        acc = v if acc is None else (acc + v).astype(np.float32)  # ascending order in fp32
    exp = (acc + bias).astype(np.float32)
    if dtype == BF16:
        exp = R.bf16_round(exp)
    assert same_bits(g[:, :T, :D], exp)
    report(f"snac_kernels/from_codes/{len(strides)}q_T{T}_{'bf16' if dtype else 'f32'}", bits_equal=True)


# ------------------------------------------------------------------------------------------------ code-book search
@pytest.mark.parametrize("bins", [5, 37, 4096])
def test_vq_search(lib, bins):
    rng = np.random.default_rng(bins)
    B, T, cd, ldz, ldq = 2, 6, 8, 12, 10
    cb = rng.standard_normal((bins, cd)).astype(np.float32)
    dup_lo, dup_hi = 1, bins - 2
    cb[dup_hi] = cb[dup_lo]  # an exact tie wherever this row is the nearest: the first index wins
    cn64 = R.normalize(cb.astype(np.float64))
    cbn = cn64.astype(np.float32)
    c2 = (cbn.astype(np.float64) ** 2).sum(-1).astype(np.float32)
    ze = rng.standard_normal((B, T, cd)).astype(np.float32)
    ze[0, 1] = 2.5 * cb[dup_hi]  # lands on the duplicated row
    ze[1, 4] = cb[dup_lo] + np.float32(1e-3) * rng.standard_normal(cd).astype(np.float32)
    ze[1, 2] = 0.0  # the eps of normalize: e = 0, every distance is c2[j]
    zd = dev(embed(ze, T, ldz))
    codes = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    zq = torch.full((B, T, ldq), SENT, device="cuda")
    cbd, cnd, c2d = dev(cb), dev(cbn), dev(c2)  # (named: a temporary's memory would be handed to the next allocation)
    rc = lib.kk_op_snac_vq_search(stream(), B, T, P(zd), ldz, cd, P(cbd), P(cnd), P(c2d), bins, P(codes), P(zq), ldq)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    got, q = codes.cpu().numpy(), host(zq)
    assert only_inside(q, T, cd) and got.min() >= 0 and got.max() < bins
    e = R.normalize(ze.astype(np.float64))
    dist = (e**2).sum(-1, keepdims=True) - 2 * e @ cbn.astype(np.float64).T + c2.astype(np.float64)  # on the operands the kernel reads
    tol = 2 * (3 * cd + 20) * U24
    worst = 0.0
    for b in range(B):
        for t in range(T):
            g = int(got[b, t])
            gap = float(dist[b, t, g] - dist[b, t].min())
            worst = max(worst, gap / tol)
            assert gap <= tol, (b, t, g, gap)
            same = [j for j in range(bins) if np.array_equal(cbn[j], cbn[g]) and c2[j] == c2[g]]
            assert g == same[0], "a later one of identical rows was chosen"
            assert same_bits(q[b, t, :cd], ze[b, t] + (cb[g] - ze[b, t]))  # vq.py:37 as written, in fp32
    assert got[0, 1] == dup_lo and got[1, 4] == dup_lo
    assert got[1, 2] == int(np.argmin(c2))  # first index of the smallest |c|^2
    report(f"snac_kernels/vq_search/bins{bins}", worst_over_bound=worst)


# ------------------------------------------------------------------------------------------------ residual unit
def pack_generic(w_oki):
    O_, K, I = w_oki.shape
    ldw = rup(O_, 64) + 4
    p = np.full((K, I, ldw), np.nan, np.float32)
    p[:, :, :O_] = np.transpose(w_oki, (1, 2, 0))
    return p, ldw


def pack_frag(lib, w_oki):
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


def run_unit(lib, x, u, dil, dtype, frag):
    """-> (out [B][L][C], tmp [B][L][C], path)."""
    B, L, C_ = x.shape
    ld = ld_of(C_, dtype)
    xd = dev(embed(x, L, ld), dtype)
    tmp = torch.full((B, L, ld), SENT, dtype=tdt(dtype), device="cuda")
    od = torch.full((B, L, ld), SENT, dtype=tdt(dtype), device="cuda")
    pk, ldw = pack_generic(u["pw"])
    wf, CinP, CoutP, bias = None, 0, 0, u["pb"]
    if frag:
        wf, CinP, CoutP = pack_frag(lib, u["pw"])
        bias = np.zeros(CoutP, np.float32)
        bias[:C_] = u["pb"]
    path = C.c_int(-9)
    keep = [dev(u["dw"].reshape(C_, 7)), dev(u["db"]), dev(u["a1"]), dev(u["a2"]), dev(pk), dev(bias)]
    rc = lib.kk_op_snac_residual_unit(stream(), B, P(xd), ld, dtype, L, C_, dil, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]), ldw,
                                      P(wf), CinP, CoutP, P(keep[5]), P(tmp), P(od), ld, C.byref(path))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    g, t = host(od), host(tmp)
    assert only_inside(g, L, C_) and only_inside(t, L, C_), "a pad column was written"
    return g[:, :, :C_], t[:, :, :C_], path.value


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dil", [1, 9])
@pytest.mark.parametrize("C_", [48, 64, 128])
def test_residual_unit(lib, C_, dil, dtype):
    rng = np.random.default_rng(C_ + dil + dtype)
    u = dict(dw=(rng.standard_normal((C_, 7, 1)) / np.sqrt(7)).astype(np.float32), db=(0.1 * rng.standard_normal(C_)).astype(np.float32),
             a1=rng.uniform(0.5, 2, C_).astype(np.float32), a2=rng.uniform(0.5, 2, C_).astype(np.float32),
             pw=(rng.standard_normal((C_, 1, C_)) / np.sqrt(C_)).astype(np.float32), pb=(0.1 * rng.standard_normal(C_)).astype(np.float32))
    frag = dtype == BF16
    wq = R.bf16_round(u["pw"]) if frag else u["pw"]  # the matrix-core pack holds bf16 weights (every C here is eligible: C % 8 == 0, C >= 16)
    worst = 0.0
    for L in (5, 64, 150):  # inside one tile; 64; 150: a dil-9 halo across the edge of the depth-wise kernel's 128-row tile
        x = values(rng, (2, L, C_), dtype)
        got, tmp, path = run_unit(lib, x, u, dil, dtype, frag)
        assert path == (MFMA if frag else GENERIC)
        # launch 1: the depth-wise conv with both Snakes
        ref1, b1 = dw_bound(x, u["dw"], u["db"], dil, u["a1"], u["a2"], dtype)
        r1 = ratio(tmp, ref1, b1)
        # launch 2: the 1x1 conv + residual on the tensor launch 1 wrote
        ref2, S2 = R.conv(tmp, wq, u["pb"], absum=True)
        ref2, S2 = ref2 + x, S2 + np.abs(x)
        b2 = 2.0**-8 * np.abs(ref2) + (C_ + 4) * U24 * S2 if path == MFMA else (C_ + 4) * U23 * S2 + (2.0**-8 * np.abs(ref2) if dtype == BF16 else 0)
        r2 = ratio(got, ref2, b2)
        assert r1 <= 1.0 and r2 <= 1.0, (L, r1, r2)
        worst = max(worst, r1, r2)
        one, _, _ = run_unit(lib, x[1:], u, dil, dtype, frag)
        assert same_bits(one[0], got[1]), "item 1 differs from its own B = 1 launch"
    report(f"snac_kernels/residual_unit/C{C_}_dil{dil}_{'bf16' if dtype else 'f32'}", worst_over_bound=worst, path=path)


# ------------------------------------------------------------------------------------------------ last conv
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cin", [8, 64, 100])
def test_conv_cout1(lib, Cin, dtype):
    rng = np.random.default_rng(Cin + dtype)
    K, pad, ldw = 7, 3, 64
    w = (rng.standard_normal((1, K, Cin)) / np.sqrt(K * Cin)).astype(np.float32)
    bias = np.array([0.1], np.float32)
    alpha = rng.uniform(0.5, 2, Cin).astype(np.float32)
    wp = np.full((K, Cin, ldw), np.nan, np.float32)
    wp[:, :, 0] = w[0]
    worst = 0.0
    for L in (1, 70, 130):
        x = values(rng, (2, L, Cin), dtype)
        ld = ld_of(Cin, dtype)
        for a in (None, alpha):
            for th in (0, 1):
                def run(xx):
                    xd = dev(embed(xx, L, ld), dtype)
                    od = torch.full((xx.shape[0], L + 3), SENT, device="cuda")
                    wd, bd, ad = dev(wp), dev(bias), (dev(a) if a is not None else None)  # (named: kept alive over the launch)
                    rc = lib.kk_op_snac_conv_cout1(stream(), xx.shape[0], P(xd), dtype, ld, L, Cin, K, pad, P(wd), ldw, P(bd), P(ad), th, P(od))
                    assert rc == 0, lib.kk_last_error()
                    torch.cuda.synchronize()
                    return host(od)

                g = run(x)
                flat = g.reshape(-1)
                assert np.all(flat[2 * L :] == SENT), "written past B * L samples"
                got = flat[: 2 * L].reshape(2, L)
                ref, S, pre = R.conv_cout1(x, w, bias, pad=pad, alpha=a, tanh=bool(th), absum=True)
                bound = (K * Cin + 4) * U24 * S
                if a is not None:
                    bound = bound + R.conv(e_snake(x.astype(np.float64), a.astype(np.float64)), np.abs(w), None, pad=pad)[..., 0]
                if th:
                    bound = bound + 4 * U23
                r = ratio(got, ref, bound)
                assert r <= 1.0, (L, a is not None, th, r)
                worst = max(worst, r)
                assert same_bits(run(x[1:]).reshape(-1)[:L], got[1]), "item 1 differs from its own B = 1 launch"
    report(f"snac_kernels/conv_cout1/C{Cin}_{'bf16' if dtype else 'f32'}", worst_over_bound=worst)
