"""GPU parity tests of mlx-audio_amd/csrc/kk_norm.hip on its own, bf16 half included: every kernel of the file against the float64
references of tests/_norm_ref.py ON THE SAME OPERANDS (the bf16-rounded inputs, upcast), through kk_op_adain, kk_op_layernorm and
kk_op_norm_finalize.

Inputs are N(3, 2^2) rounded to bf16, zero past an item's length, NaN in every input pad column [C, ld); outputs are pre-filled
with a sentinel, so a pad channel that leaks, a row dropped at a chunk / 4-row / 32-row edge or a write outside the documented
region shows.  Bounds (each test reports its worst error as a ratio of its bound):

  statistics   |mean - ref| <= 1e-5 (|mean| + 1 / rstd), rstd to 1e-4 relative: a CPU emulation with fp32 sums in a worse order than
               the kernels' (one fp32 accumulator over all rows, shifted by row 0) measured 1.7e-7 / 1.4e-5 at these shapes; one row
               dropped out of 513 moves a mean by ~4e-3 of its std
  bf16 output  |got - ref| <= 2^-8 |ref| + 2e-5 max|ref|: one bf16 rounding (8 significant bits) + the conv tests' bar for
               "fp32, summation order only"
  fp32 output  rel_max < 1e-5 (the bar of test_layernorm_and_adaln)
  Snake fast   the bf16 bound + 4 x the largest fp32 fast-versus-exact difference measured in the test at the same shape
  finalize     1e-6 relative: the kernels work in double on the same fp32 partials, only the final casts differ
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _norm_ref as R
from _util import err_stats, report

pytestmark = pytest.mark.gpu

SENT = -512.0  # exact in bf16; the outputs here stay within a few tens
LENS_APPLY = [70, 64, 33, 32, 31, 1, 0]
ROWS_APPLY = 75  # Lout_rows 75 / 150 (pool): neither is a multiple of the apply kernels' 32-row blocks


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def i32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).cuda()


def make_x(rng, B, L, Cc, ld, lens, bf16=True):
    """-> (host tensor [B][L][ld] in the kernel's dtype, the same values as float64).  NaN in [Cc, ld), zero rows past lens[b]."""
    x = (rng.standard_normal((B, L, ld)) * 2 + 3).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    x[:, :, Cc:] = np.nan
    t = torch.tensor(x)
    if bf16:
        t = t.to(torch.bfloat16)
    return t, t.double().numpy()


def place(t, offset=0, fill=None):
    """A device buffer holding host tensor `t` (or `fill`, in t's shape and dtype) `offset` ELEMENTS past an aligned base."""
    flat = torch.full((t.numel() + 8,), 0.0 if fill is None else fill, dtype=t.dtype, device="cuda")
    view = flat[offset : offset + t.numel()].view(t.shape)
    if fill is None:
        view.copy_(t)
    assert view.data_ptr() % 16 == (offset * t.element_size()) % 16
    return view


def bf16_ratio(got, ref, extra=0.0):
    """Worst |got - ref| as a ratio of the bf16-output bound (+ extra) over one item's valid region."""
    if ref.size == 0:
        return 0.0
    bound = 2.0**-8 * np.abs(ref) + 2e-5 * np.abs(ref).max() + extra
    return float((np.abs(got - ref) / bound).max())


def run_adain(lib, xt, lens, Cc, gb, *, act=R.ACT_NONE, slope=0.2, alpha=None, pool=False, pw=None, pb=None, ldo, Cpad, bf16=True, fast=0,
              x_off=0, out_off=0):
    """kk_op_adain on host tensor xt [B][L][ldx] -> (out [B][Lout_rows][ldo] as a host tensor, mean [B][Cc], rstd [B][Cc]) with the
    statistics read back from `scratch` at the offsets include/kokoro_hip.h documents."""
    from mlx_audio_amd import _lib

    B, L, ldx = xt.shape
    Lout = 2 * L if pool else L
    xd = place(xt, x_off)
    out = place(torch.empty((B, Lout, ldo), dtype=xt.dtype), out_off, fill=SENT)
    nchunk = (L + 511) // 512
    scratch = torch.full((B * nchunk * 2 * Cc + 2 * B * Cc,), float("nan"), device="cuda")
    gbd, lend = f32(gb), i32(lens)
    ald = f32(alpha) if alpha is not None else None
    pwd, pbd = (f32(pw), f32(pb)) if pool else (None, None)
    rc = lib.kk_op_adain(stream(), B, P(xd), ldx, L, P(lend), Cc, P(gbd), gb.shape[1], act, slope, P(ald), int(pool), P(pwd), P(pbd), P(out), ldo,
                         Cpad, Lout, P(scratch), scratch.numel(), _lib.KK_BF16 if bf16 else _lib.KK_F32, fast)
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    st = scratch.cpu().numpy().astype(np.float64)
    o = B * nchunk * 2 * Cc
    return out.cpu(), st[o : o + B * Cc].reshape(B, Cc), st[o + B * Cc : o + 2 * B * Cc].reshape(B, Cc)


def stats_ratios(mean, rstd, x64, lens, Cc):
    """Worst statistics errors of a batch as ratios of their bounds; an empty item must give exactly 0 / 0."""
    rm = rr = 0.0
    for b, n in enumerate(lens):
        m_ref, r_ref = R.instnorm_stats(x64[b, :, :Cc], n)
        if n == 0:
            assert not mean[b].any() and not rstd[b].any(), f"item {b}: statistics of an empty item are not 0 / 0"
            continue
        assert np.isfinite(mean[b]).all() and np.isfinite(rstd[b]).all(), f"item {b} (len {n}): non-finite statistics"
        rm = max(rm, float((np.abs(mean[b] - m_ref) / (1e-5 * (np.abs(m_ref) + 1.0 / r_ref))).max()))
        rr = max(rr, float((np.abs(rstd[b] - r_ref) / (1e-4 * r_ref)).max()))
    return rm, rr


def check_apply_layout(out64, lens, Cc, Cpad, pool):
    """What both apply kernels promise around the valid region: zeros in [Cc, Cpad) and past the valid rows, the sentinel from Cpad on."""
    assert not np.isnan(out64).any(), "NaN in the output (a pad channel of the input leaked)"
    assert np.all(out64[:, :, Cc:Cpad] == 0), "pad channels [C, Cpad) are not exactly 0"
    assert np.all(out64[:, :, Cpad:] == SENT), "columns [Cpad, ldo) were written"
    for b, n in enumerate(lens):
        assert np.all(out64[b, (2 * n if pool else n) :, :Cpad] == 0), f"item {b}: rows past the valid length are not 0"


def apply_ratio(out64, x64, lens, Cc, gb, extra=0.0, **kw):
    worst = 0.0
    for b, n in enumerate(lens):
        ref = R.adain(x64[b, :, :Cc], n, gb[b], **kw)
        worst = max(worst, bf16_ratio(out64[b, : ref.shape[0], :Cc], ref, extra))
    return worst


# ------------------------------------------------------------------------------------------------ statistics (bf16)
LENS_V = [1030, 1025, 1024, 513, 512, 511, 1, 0]
LENS_P = [517, 514, 515, 512, 1, 0]
STATS_CASES = [
    # id, C, ldx, L_rows, lens, element offset of x
    ("bf16v_C64", 64, 64, 1030, LENS_V, 0),  # 32 rows in flight
    ("bf16v_C128", 128, 128, 1030, LENS_V, 0),  # 16
    ("bf16v_C1024", 1024, 1024, 1030, [1030, 513, 1, 0], 0),  # 2
    ("bf16p_C514_ld576", 514, 576, 517, LENS_P, 0),
    ("bf16p_C1090_ld1152", 1090, 1152, 517, LENS_P, 0),
    ("bf16p_C72_ld72", 72, 72, 517, LENS_P, 0),
    ("bf16p_C100_ld104", 100, 104, 517, LENS_P, 0),
    ("scalar_C50_ld50", 50, 50, 517, LENS_P, 0),
    ("scalar_C40_ld40", 40, 40, 517, LENS_P, 0),
    ("C64_ld72", 64, 72, 517, LENS_P, 0),  # kk_launch_instnorm_stats gives C = 64 to the bf16v kernel at any pitch % 8 == 0: bf16v with pitch > C
    ("scalar_C128_misaligned", 128, 128, 517, LENS_P, 1),  # vec-shaped, base one element off 16 bytes
]


@pytest.mark.parametrize("case", STATS_CASES, ids=[c[0] for c in STATS_CASES])
def test_instnorm_stats_bf16(lib, case):
    name, Cc, ldx, L, lens, x_off = case
    rng = np.random.default_rng(Cc * 7 + ldx)
    B = len(lens)
    xt, x64 = make_x(rng, B, L, Cc, ldx, lens)
    gb = (rng.standard_normal((B, 2 * Cc)) * 0.5).astype(np.float32)
    ldo = ldx if x_off == 0 else ldx + 8
    out, mean, rstd = run_adain(lib, xt, lens, Cc, gb, ldo=ldo, Cpad=Cc, x_off=x_off)
    rm, rr = stats_ratios(mean, rstd, x64, lens, Cc)
    out64 = out.double().numpy()
    check_apply_layout(out64, lens, Cc, Cc, False)
    ro = apply_ratio(out64, x64, lens, Cc, gb)
    report(f"norm/stats/{name}", mean_ratio=rm, rstd_ratio=rr, out_ratio=ro)
    assert rm <= 1.0 and rr <= 1.0 and ro <= 1.0


# ------------------------------------------------------------------------------------------------ AdaIN apply (bf16)
APPLY_SHAPES = [(8, 8, 8, 8), (512, 512, 512, 512), (514, 576, 576, 576), (1090, 1152, 1152, 1152), (50, 64, 64, 72)]  # C, Cpad, ldx, ldo


def apply_inputs(Cc, ldx, seed):
    rng = np.random.default_rng(seed)
    B = len(LENS_APPLY)
    xt, x64 = make_x(rng, B, ROWS_APPLY, Cc, ldx, LENS_APPLY)
    gb = (rng.standard_normal((B, 2 * Cc)) * 0.5).astype(np.float32)
    alpha = rng.uniform(0.5, 1.5, Cc).astype(np.float32)
    pw, pb = rng.standard_normal((Cc, 3)).astype(np.float32), rng.standard_normal(Cc).astype(np.float32)
    return xt, x64, gb, alpha, pw, pb


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_LRELU], ids=["none", "lrelu"])
@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=["C%d_Cp%d_ldx%d_ldo%d" % s for s in APPLY_SHAPES])
def test_adain_apply_bf16v_and_its_scalar_twin(lib, shape, act, pool):
    """adain_act_bf16v_kernel against the reference, and against adain_act_kernel<bf16_t> on the same statistics: `out` one element
    off 16 bytes forces the scalar apply while x, and with it the statistics pass, stays as it was.  The vector kernel's comment says
    its arithmetic is the scalar kernel's in the same order, so the two must agree bit for bit."""
    Cc, Cpad, ldx, ldo = shape
    xt, x64, gb, alpha, pw, pb = apply_inputs(Cc, ldx, Cc)
    kw = dict(act=act, slope=0.2, pool_w=pw if pool else None, pool_b=pb if pool else None)
    run = dict(act=act, slope=0.2, pool=pool, pw=pw, pb=pb, ldo=ldo, Cpad=Cpad)
    out_v, mean_v, rstd_v = run_adain(lib, xt, LENS_APPLY, Cc, gb, **run)
    out_s, mean_s, rstd_s = run_adain(lib, xt, LENS_APPLY, Cc, gb, out_off=1, **run)
    assert np.array_equal(mean_v, mean_s) and np.array_equal(rstd_v, rstd_s)
    worst = {}
    for tag, out in (("vector", out_v), ("scalar", out_s)):
        o64 = out.double().numpy()
        check_apply_layout(o64, LENS_APPLY, Cc, Cpad, pool)
        worst[tag] = apply_ratio(o64, x64, LENS_APPLY, Cc, gb, **kw)
    rm, rr = stats_ratios(mean_v, rstd_v, x64, LENS_APPLY, Cc)
    differ = int((out_v.view(torch.int16) != out_s.view(torch.int16)).sum())
    report(f"norm/adain_bf16v/C{Cc}/act{act}/pool{int(pool)}", vector_ratio=worst["vector"], scalar_ratio=worst["scalar"], mean_ratio=rm,
           rstd_ratio=rr, vector_scalar_bits_differ=differ)
    assert worst["vector"] <= 1.0 and worst["scalar"] <= 1.0 and rm <= 1.0 and rr <= 1.0
    assert differ == 0, f"{differ} elements of the vector apply differ in bits from the scalar apply"


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
def test_adain_apply_scalar_bf16_snake(lib, pool):
    """adain_act_kernel<bf16_t> with Snake, exact sine (fast = 0) and hardware sine (fast = 1).  The hardware sine's error is not derivable
    here: the fast bound adds 4 x the largest fp32 fast-versus-exact difference of this very shape, measured through the fp32 kernel."""
    Cc, Cpad, ldx, ldo = 50, 64, 64, 72
    xt, x64, gb, alpha, pw, pb = apply_inputs(Cc, ldx, 1000 + int(pool))
    kw = dict(act=R.ACT_SNAKE, alpha=alpha, pool_w=pw if pool else None, pool_b=pb if pool else None)
    run = dict(act=R.ACT_SNAKE, alpha=alpha, pool=pool, pw=pw, pb=pb, ldo=ldo, Cpad=Cpad)
    f0, _, _ = run_adain(lib, xt.float(), LENS_APPLY, Cc, gb, bf16=False, fast=0, **run)
    f1, _, _ = run_adain(lib, xt.float(), LENS_APPLY, Cc, gb, bf16=False, fast=1, **run)
    f0, f1 = f0.double().numpy(), f1.double().numpy()
    check_apply_layout(f0, LENS_APPLY, Cc, Cpad, pool)
    check_apply_layout(f1, LENS_APPLY, Cc, Cpad, pool)
    fast_diff = float(np.abs(f1 - f0)[:, :, :Cc].max())
    ratios = {}
    for fast in (0, 1):
        out, mean, rstd = run_adain(lib, xt, LENS_APPLY, Cc, gb, fast=fast, **run)
        o64 = out.double().numpy()
        check_apply_layout(o64, LENS_APPLY, Cc, Cpad, pool)
        ratios[fast] = apply_ratio(o64, x64, LENS_APPLY, Cc, gb, extra=4.0 * fast_diff * fast, **kw)
    rm, rr = stats_ratios(mean, rstd, x64, LENS_APPLY, Cc)
    report(f"norm/adain_scalar_bf16_snake/pool{int(pool)}", exact_ratio=ratios[0], fast_ratio=ratios[1], fp32_fast_minus_exact_max_abs=fast_diff,
           mean_ratio=rm, rstd_ratio=rr)
    assert ratios[0] <= 1.0 and ratios[1] <= 1.0 and rm <= 1.0 and rr <= 1.0


# ------------------------------------------------------------------------------------------------ LayerNorm (fp32 and bf16)
LN_LENS = [39, 38, 5, 1, 0]
LN_ROWS = 39


def run_layernorm(lib, xd, rd, lens, Cc, *, w=None, b=None, gb=None, act, bf16, ldo, out=None):
    from mlx_audio_amd import _lib

    B, L, ldx = xd.shape
    if out is None:
        out = torch.full((B, L, ldo), SENT, dtype=xd.dtype, device="cuda")
    wd, bd = (f32(w), f32(b)) if w is not None else (None, None)
    gd = f32(gb) if gb is not None else None
    lend = i32(lens)
    rc = lib.kk_op_layernorm(stream(), B, P(xd), ldx, P(rd), rd.shape[2] if rd is not None else 0, L, P(lend), Cc, P(wd), P(bd), P(gd),
                             gb.shape[1] if gb is not None else 0, 1e-5, act, 0.1, P(out), ldo, _lib.KK_BF16 if bf16 else _lib.KK_F32)
    torch.cuda.synchronize()
    return rc, out.cpu().double().numpy()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cc", [8, 64, 100, 514, 2048])
def test_layernorm_ragged_pitched(lib, Cc, bf16):
    """layernorm_kernel<float> / <bf16_t>: both affine forms, with and without a residual of another pitch, NONE / LRELU, ragged rows,
    row and output pitches above C."""
    rng = np.random.default_rng(Cc)
    B = len(LN_LENS)
    ldx, ldo, ldr = Cc + 8, Cc + 16, Cc + 24
    xt, x64 = make_x(rng, B, LN_ROWS, Cc, ldx, LN_LENS, bf16)
    rt, r64 = make_x(rng, B, LN_ROWS, Cc, ldr, LN_LENS, bf16)
    w, bias = rng.standard_normal(Cc).astype(np.float32), rng.standard_normal(Cc).astype(np.float32)
    gb = (rng.standard_normal((B, 2 * Cc + 4)) * 0.5).astype(np.float32)
    xd, rd = xt.cuda(), rt.cuda()
    worst = 0.0
    for form in ("wb", "gb"):
        for res in (False, True):
            for act in (R.ACT_NONE, R.ACT_LRELU):
                rc, got = run_layernorm(lib, xd, rd if res else None, LN_LENS, Cc, w=w if form == "wb" else None, b=bias if form == "wb" else None,
                                        gb=gb if form == "gb" else None, act=act, bf16=bf16, ldo=ldo)
                assert rc == 0, lib.kk_last_error()
                what = f"C{Cc}/{form}/res{int(res)}/act{act}"
                assert not np.isnan(got).any(), what
                assert np.all(got[:, :, Cc:] == SENT), f"{what}: output pad columns were written"
                for bi, n in enumerate(LN_LENS):
                    assert np.all(got[bi, n:, :Cc] == 0), f"{what}: item {bi} rows past its length are not 0"
                    if n == 0:
                        continue
                    ref = R.layernorm(x64[bi], r64[bi] if res else None, n, Cc, w=w if form == "wb" else None, b=bias if form == "wb" else None,
                                      gb=gb[bi] if form == "gb" else None, eps=1e-5, act=act, slope=0.1)
                    ratio = bf16_ratio(got[bi, :n, :Cc], ref) if bf16 else err_stats(got[bi, :n, :Cc], ref)["rel_max"] / 1e-5
                    assert ratio < 1.0, f"{what}: item {bi} at {ratio:.3f} of its bound"
                    worst = max(worst, ratio)
    report(f"norm/layernorm/{'bf16' if bf16 else 'fp32'}/C{Cc}", worst_ratio=worst)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_layernorm_refuses_more_than_2048_channels(lib, bf16):
    Cc = 2049
    xt, _ = make_x(np.random.default_rng(0), 1, 3, Cc, Cc, [3], bf16)
    rc, got = run_layernorm(lib, xt.cuda(), None, [3], Cc, w=np.ones(Cc), b=np.zeros(Cc), act=R.ACT_NONE, bf16=bf16, ldo=Cc)
    assert rc != 0 and b"2048" in lib.kk_last_error()
    assert np.all(got == SENT)


# ------------------------------------------------------------------------------------------------ finalize / fold / add_row
TILE = 128


def tile_partials(rng, ntiles, Cc, lens):
    """Synthetic conv-epilogue partials: float64 column sums / sums of squares of random data per 128-row tile, cast to fp32.
    Column 0 is constant 0.5 (variance 0; its sums are exact in fp32), column 1 has mean / std = 30, column 2 is constant 0.3 (its fp32
    sums are rounded, so SS / L - mean^2 lands on either side of 0 and the clamp decides); tiles past an item's length hold zeros."""
    part = np.zeros((len(lens), ntiles, 2, Cc), np.float32)
    for b, n in enumerate(lens):
        x = rng.standard_normal((ntiles * TILE, Cc)) * 2 + 3
        x[:, 0] = 0.5
        x[:, 1] = rng.standard_normal(ntiles * TILE) + 30.0
        x[:, 2] = 0.3
        x[n:] = 0
        t = x.reshape(ntiles, TILE, Cc)
        part[b, :, 0], part[b, :, 1] = t.sum(1), (t * t).sum(1)
    return part


def finalize_ratios(got, part, lens, gb, Cc):
    """Worst mean / rstd / pa / pb errors (as ratios of the 1e-6 bounds) of a finalize against the float64 reference on the same partials."""
    mean, rstd, pa, pb = got
    worst = dict(mean=0.0, rstd=0.0, pa=0.0, pb=0.0)
    for b, n in enumerate(lens):
        m, r, a, s = R.finalize_tiles(part[b], n, 1e-5, gb[b])
        if n == 0:
            assert not mean[b].any() and not rstd[b].any() and not pa[b, :Cc].any() and np.array_equal(pb[b, :Cc], gb[b, Cc : 2 * Cc].astype(np.float64))
            continue
        worst["mean"] = max(worst["mean"], float((np.abs(mean[b] - m) / (1e-6 * (np.abs(m) + 1.0 / r))).max()))
        worst["rstd"] = max(worst["rstd"], float((np.abs(rstd[b] - r) / (1e-6 * r)).max()))
        worst["pa"] = max(worst["pa"], float((np.abs(pa[b, :Cc] - a) / (1e-6 * np.abs(a))).max()))
        worst["pb"] = max(worst["pb"], float((np.abs(pb[b, :Cc] - s) / (1e-6 * (np.abs(gb[b, Cc : 2 * Cc]) + np.abs(m * a)))).max()))
    return worst


def check_fold_layout(pa, pb, Cc, Cp):
    for p in (pa, pb):
        assert np.all(p[:, Cc:Cp] == 0), "pa / pb are not exactly 0 in the pad channels [C, Cp)"
        assert np.all(p[:, Cp:] == SENT), "pa / pb were written from Cp on"


def run_finalize(lib, B, Cc, lens, L_rows, part, ntiles, gb, pstride, Cp, *, mean_in=None, rstd_in=None, want_stats=True, want_fold=True, add_row=None,
                 add_row_bs=0):
    """kk_op_norm_finalize -> rc, (mean, rstd, pa, pb) as float64 host arrays (None where not asked for), the partials after the call."""
    pd = f32(part) if part is not None else None
    gd = f32(gb) if gb is not None else None
    if mean_in is not None:
        md, rd = f32(mean_in), f32(rstd_in)
    else:
        md, rd = (torch.full((B, Cc), SENT, device="cuda"), torch.full((B, Cc), SENT, device="cuda")) if want_stats else (None, None)
    pad, pbd = (torch.full((B, pstride), SENT, device="cuda"), torch.full((B, pstride), SENT, device="cuda")) if want_fold else (None, None)
    lend = i32(lens) if lens is not None else None
    rc = lib.kk_op_norm_finalize(stream(), B, Cc, P(lend), L_rows, P(pd), ntiles, P(add_row), add_row_bs, P(gd),
                                 gb.shape[1] if gb is not None else 0, P(md), P(rd), P(pad), P(pbd), pstride, Cp)
    torch.cuda.synchronize()
    host = [t.cpu().numpy().astype(np.float64) if t is not None else None for t in (md, rd, pad, pbd)]
    return rc, host, (pd.cpu().numpy() if pd is not None else None)


@pytest.mark.parametrize("CCp", [(40, 64), (128, 128), (200, 256)], ids=["C40_Cp64", "C128_Cp128", "C200_Cp256"])
@pytest.mark.parametrize("ntiles", [1, 31, 32, 33, 70])
def test_norm_finalize_and_fold(lib, ntiles, CCp):
    """norm_finalize_tiles_kernel (32 tile lanes: one, one short of, exactly, one past and more than two rounds of them) and the
    fused == 2 fold of stats_final_kernel<float>."""
    Cc, Cp = CCp
    rng = np.random.default_rng(ntiles * 1000 + Cc)
    rows = ntiles * TILE
    lens = [rows, rows - 51, TILE * (ntiles // 2) + 3, 0]
    B, pstride = len(lens), Cp + 8
    part = tile_partials(rng, ntiles, Cc, lens)
    gb = (rng.standard_normal((B, 2 * Cc + 4)) * 0.5).astype(np.float32)
    rc, got, part_after = run_finalize(lib, B, Cc, lens, rows, part, ntiles, gb, pstride, Cp)
    assert rc == 0, lib.kk_last_error()
    assert np.array_equal(part_after, part)
    check_fold_layout(got[2], got[3], Cc, Cp)
    worst = finalize_ratios(got, part, lens, gb, Cc)
    assert np.all(got[0][: B - 1, 0] == 0.5) and 25.0 < got[0][0, 1] * got[1][0, 1] < 36.0  # the planted columns are what they were planted as
    # the production call asks for pa / pb alone; the kernel is deterministic, so the bits repeat
    rc, only, _ = run_finalize(lib, B, Cc, lens, rows, part, ntiles, gb, pstride, Cp, want_stats=False)
    assert rc == 0 and np.array_equal(only[2], got[2]) and np.array_equal(only[3], got[3])
    # statistics alone: no pa / pb, nothing folded
    rc, stats, _ = run_finalize(lib, B, Cc, lens, rows, part, ntiles, None, pstride, Cp, want_fold=False)
    assert rc == 0 and np.array_equal(stats[0], got[0]) and np.array_equal(stats[1], got[1])
    # fold form: the same pa / pb from the mean / rstd just computed
    rc, fold, _ = run_finalize(lib, B, Cc, lens, rows, None, 0, gb, pstride, Cp, mean_in=got[0], rstd_in=got[1])
    assert rc == 0, lib.kk_last_error()
    assert np.array_equal(fold[0], got[0]) and np.array_equal(fold[1], got[1])  # inputs of this form: left alone
    check_fold_layout(fold[2], fold[3], Cc, Cp)
    wf = dict(pa=0.0, pb=0.0)
    for b in range(B):
        a, s = R.fold(got[0][b], got[1][b], gb[b])
        scale_a, scale_b = 1e-6 * np.abs(a), 1e-6 * (np.abs(gb[b, Cc : 2 * Cc]) + np.abs(got[0][b] * a))
        if lens[b] == 0:
            assert not fold[2][b, :Cc].any() and np.array_equal(fold[3][b, :Cc], gb[b, Cc : 2 * Cc].astype(np.float64))
            continue
        wf["pa"] = max(wf["pa"], float((np.abs(fold[2][b, :Cc] - a) / scale_a).max()))
        wf["pb"] = max(wf["pb"], float((np.abs(fold[3][b, :Cc] - s) / scale_b).max()))
    report(f"norm/finalize/tiles{ntiles}/C{Cc}", fold_pa_ratio=wf["pa"], fold_pb_ratio=wf["pb"],
           fold_bits_equal_finalize=bool(np.array_equal(fold[2], got[2]) and np.array_equal(fold[3], got[3])), **{k + "_ratio": v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0 and max(wf.values()) <= 1.0


@pytest.mark.parametrize("Cc", [40, 300])
def test_norm_finalize_add_row(lib, Cc):
    """stat_add_row_kernel in front of the finalize: tile 0 gains row 0 of each item and its square (fp32: the gained values to one
    fp32 ulp of the float64 sum), every other tile keeps its bits, and the statistics are those of the updated partials.
    len == NULL: every item has L_rows rows."""
    rng = np.random.default_rng(Cc)
    ntiles, B, ldx, xrows = 3, 3, Cc + 8, 5
    rows = ntiles * TILE
    part = tile_partials(rng, ntiles, Cc, [rows] * B)
    xt, x64 = make_x(rng, B, xrows, Cc, ldx, [xrows] * B)
    gb = (rng.standard_normal((B, 2 * Cc)) * 0.5).astype(np.float32)
    Cp = (Cc + 63) // 64 * 64
    rc, got, after = run_finalize(lib, B, Cc, None, rows + 1, part, ntiles, gb, Cp, Cp, add_row=xt.cuda(), add_row_bs=xrows * ldx)
    assert rc == 0, lib.kk_last_error()
    assert np.array_equal(after[:, 1:], part[:, 1:]), "add_row touched a tile other than tile 0"
    row0 = x64[:, 0, :Cc]
    want = np.stack([part[:, 0, 0].astype(np.float64) + row0, part[:, 0, 1].astype(np.float64) + row0 * row0], 1)
    ulp = float((np.abs(after[:, 0].astype(np.float64) - want) / (2.0**-23 * np.abs(want))).max())
    assert ulp <= 1.0
    check_fold_layout(got[2], got[3], Cc, Cp)
    worst = finalize_ratios(got, after, [rows + 1] * B, gb, Cc)
    report(f"norm/finalize_add_row/C{Cc}", tile0_fp32_ulps=ulp, **{k + "_ratio": v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


def test_norm_finalize_refuses_bad_arguments(lib):
    """Each refusal comes back non-zero with a message and before any launch: every output keeps its sentinel."""
    B, Cc, Cp, pstride, ntiles = 2, 40, 64, 72, 2
    rng = np.random.default_rng(5)
    lens = [200, 100]
    part = tile_partials(rng, ntiles, Cc, lens)
    gb = (rng.standard_normal((B, 2 * Cc)) * 0.5).astype(np.float32)
    ok = dict(B=B, Cc=Cc, lens=lens, L_rows=256, part=part, ntiles=ntiles, gb=gb, pstride=pstride, Cp=Cp)
    mean = rng.standard_normal((B, Cc)).astype(np.float32)
    bad = {
        "B == 0": dict(ok, B=0),
        "C == 0": dict(ok, Cc=0),
        "ntiles == 0": dict(ok, ntiles=0),
        "pa without gamma_beta": dict(ok, gb=None),
        "Cp < C": dict(ok, Cp=Cc - 8),
        "pstride < Cp": dict(ok, pstride=Cp - 8),
    }
    for what, kw in bad.items():
        rc, got, after = run_finalize(lib, **kw)
        assert rc != 0 and b"kk_op_norm_finalize" in lib.kk_last_error(), what
        assert all(np.all(t == SENT) for t in got), what
        assert np.array_equal(after, part), what
    # fold form (partial == NULL) without mean / without rstd: ctypes hands NULL for None, so build the calls by hand
    pa, pb = torch.full((B, pstride), SENT, device="cuda"), torch.full((B, pstride), SENT, device="cuda")
    md, gd, ld = f32(mean), f32(gb), i32(lens)
    for what, (m, r) in {"fold without mean": (None, md), "fold without rstd": (md, None)}.items():
        rc = lib.kk_op_norm_finalize(stream(), B, Cc, P(ld), 256, None, 0, None, 0, P(gd), 2 * Cc, P(m), P(r), P(pa), P(pb), pstride, Cp)
        torch.cuda.synchronize()
        assert rc != 0 and b"fold form" in lib.kk_last_error(), what
        assert bool((pa == SENT).all()) and bool((pb == SENT).all()), what
    rc, got, _ = run_finalize(lib, **ok)
    assert rc == 0, lib.kk_last_error()  # and the well-formed call next to them goes through
