"""GPU parity tests of the generic tap-loop kernel (csrc/kk_conv.hip, conv_generic_kernel: every conv, transposed conv and Linear of the fp32
models and every bf16 conv the matrix-core kernels refuse) through kk_op_conv1d, against tests/_conv_ref.py (float64, pinned by
tests/test_conv_ref_cpu.py).  The conventions are those of tests/test_gpu_kokoro_kernels.py.

Layout of a case.  x sits in a [B][Lin][Cin + pad] buffer, the residual in [B][rows][Cout + pad], the output in [B * rows + 2][Cout + pad] (two
guard rows behind the last item); the pads are 8 (aligned), 3 and 1 (odd), rotated over the three buffers by the case's crc32 seed.  NaN fills the
pad channels of x and res, the rows of x from lin[b] on, the rows of res and of the accumulate operand from lout[b] on, and one element behind the
bias.  The output starts as the sentinel -512 (exact in bf16) outside [rows][Cout].  Checked per case: nothing outside [row < rows][co < Cout] was
written (so the guard rows too: the rows phase + stride q >= Lo_rows of a transposed launch whose Lo_rows is no multiple of the stride), rows
[lout[b], rows) are exactly zero, every value is finite, and |got - ref| <= bound on the live rows; report() logs worst error / bound.
B = 3 with lengths {full, a third, 0} unless a test says otherwise.

What kk_op_conv1d cannot reach, and where it is checked instead:
  * the ELU input form (KKConvArgs.in_act; the entry leaves it 0).  tests/test_gpu_mimi_kernels.py compares it element-wise through kk_op_mimi_conv
    with the dispatch pinned to this kernel: test_generic_elu_first_conv (Cin 1, K 7), the strided encoder convs and the transposed convs
    (f32 and bf16), so it is left out here.
  * Q < Lo_rows (a launch that covers fewer rows than the buffer has).  The entry derives Q from Lout_rows (Q = Lout_rows, or
    ceil(Lout_rows / stride) per phase), as every other single-op entry does; only the model's own launches pass a smaller Q.  The reachable half
    of that guard, Q stride > Lo_rows, is in the transposed cases with output padding.
  KK_ACT_GELU_TANH is reachable (act = 4) and is in the epilogue group.

Bits.  Without a nonlinear term the float32 operation order is the kernel's: acc = fmaf(x[r][c], w[t][c][co], acc) over t = 0 .. Kw - 1, c = 0 .. Cin - 1
(the zero fill up to the next multiple of 16 adds exact zeros), then + bias, + res, * scale, each one rounding (the build has -ffp-contract=off).
With operands on the bf16 grid a product has 16 bits and product + acc is exact in float64 (asserted with TwoSum), so float64 followed by one
rounding to float32 IS fmaf.  test_bits_* compare bits for a Linear (Kw 1, Cin 13), a Kw 3 / Cin 17 conv, and the tap-free phases of a
Kw < stride transposed conv (bias, residual and scale only).

Bounds (u = 2^-24; nothing here is measured).  n = ntaps * ceil(Cin / 16) * 16 FMAs in one chain per output element, ntaps = Kw, or
ceil(Kw / stride) for a transposed conv; S = sum |w f(x)| from the reference.
  pre-activation  e = (n + 2) u S + u |bias|: the chain, the input transform's product (in_slope), the bias add.
  lrelu           e <- max(1, |slope|) e + u |v|                            (Lipschitz constant; the product)
  gelu            e <- 1.13 e + |v| / 2 (6u + u |v|) + 2u |g|: max g' = 1.129; erff within 2 ulp of a value <= 1 (4u), its argument v / sqrt 2
                  rounded (erf' <= 1.13: 0.8 u |v|, taken as u |v|), 1 + erf rounded (2u); the two products.
  gelu_tanh       e <- 1.13 e + |v| / 2 (9u) + 2u |g|: max g' = 1.129; the argument a = 0.79788 (v + 0.044715 v^3) carries 6u |a| through five
                  roundings of like-signed terms and a tanh'(a) <= 0.448 (3u); tanhf within 2 ulp (4u); 1 + tanh rounded (2u).
  res, accumulate e <- e + u |v| each;  scale != 1: e <- |scale| e + u |v|.
  bf16 output     + 2^-8 |ref|.  bf16 inputs (x, res, the accumulate operand) are handed to the reference already rounded and add nothing.
  bound = 2 e (a factor 2 of slack, as in test_gpu_kokoro_kernels.py); assert worst <= 1.0."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

import _conv_ref as R
from _util import report

pytestmark = pytest.mark.gpu

SENT = -512.0
U24 = 2.0**-24
F32, BF16 = 0, 1
GUARD = 2
PAIRS = [pytest.param((F32, F32), id="f32_f32"), pytest.param((BF16, BF16), id="bf16_bf16"), pytest.param((BF16, F32), id="bf16_f32"),
         pytest.param((F32, BF16), id="f32_bf16")]
ACTS = {"none": R.ACT_NONE, "lrelu": R.ACT_LRELU, "gelu": R.ACT_GELU, "gelu_tanh": R.ACT_GELU_TANH}


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


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def dev(a, dtype=F32):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).to(tdt(dtype)).cuda()


def idev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def cast(a, dtype):
    return R.bf16_round(a) if dtype == BF16 else np.asarray(a, np.float32)


def embed(vals, ld, lens=None, fill=np.nan):
    """vals [B][r][c] inside a [B][r][ld] buffer of `fill`, rows from lens[b] on filled too."""
    B, r, c = vals.shape
    buf = np.full((B, r, ld), fill, np.float32)
    buf[:, :, :c] = vals
    for b, n in enumerate(lens if lens is not None else []):
        buf[b, n:, :c] = fill
    return buf


def lens3(n):
    return [n, max(1, n // 3), 0]


def conv_rows(n, Kw, s, p, d):
    return max(0, (n + 2 * p - d * (Kw - 1) - 1) // s + 1) if n else 0


def convT_rows(n, Kw, s, p, opad=0):
    return max(0, (n - 1) * s - 2 * p + Kw + opad) if n else 0


def case_data(key, B, Lin, Cin, Cout, Kw, rows, idt, odt, *, w_scale=None, res=False, old=False, bias=True):
    """Operands as the kernel reads them (float32 arrays on the grid of their device type)."""
    rng = np.random.default_rng(seed_of(*key))
    d = {"x": cast(rng.standard_normal((B, Lin, Cin)), idt),
         "w": (rng.standard_normal((Cout, Kw, Cin)) * (w_scale or 1.0 / math.sqrt(Kw * Cin))).astype(np.float32),
         "bias": rng.standard_normal(Cout).astype(np.float32) if bias else None,
         "res": cast(rng.standard_normal((B, rows, Cout)), odt) if res else None,
         "old": cast(rng.standard_normal((B, rows, Cout)), odt) if old else None}
    return d


def launch(lib, key, d, *, idt, odt, rows, transposed=False, stride=1, pad=0, dil=1, in_shift=0, in_slope=1.0, act=R.ACT_NONE, act_slope=0.0,
           scale=1.0, lin=None, lout=None):
    """One kk_op_conv1d call on the NaN / sentinel layout of the module docstring -> the whole output buffer [B * rows + GUARD][ldo] (float32)."""
    x, w, bias, res, old = d["x"], d["w"], d["bias"], d["res"], d["old"]
    B, Lin, Cin = x.shape
    Cout, Kw, _ = w.shape
    pads = np.roll([8, 3, 1], seed_of(*key) % 3)
    ldx, ldo, ldr = Cin + int(pads[0]), Cout + int(pads[1]), Cout + int(pads[2])
    xd = dev(embed(x, ldx, lin), idt)
    wp, ldw = R.pack_w(w)
    wd = dev(wp)
    bd = dev(np.concatenate([bias, [np.nan]])) if bias is not None else None
    rd = dev(embed(res, ldr, lout if lout is not None else [rows] * B), odt) if res is not None else None
    ob = np.full((B * rows + GUARD, ldo), SENT, np.float32)
    if old is not None:
        ob[: B * rows] = embed(old, ldo, lout if lout is not None else [rows] * B, fill=np.nan).reshape(B * rows, ldo)
        ob[:, Cout:] = SENT
    od = dev(ob, odt)
    lind = idev(lin) if lin is not None else None
    loutd = idev(lout) if lout is not None else None
    rc = lib.kk_op_conv1d(stream(), B, P(xd), ldx, Lin, P(lind), P(wd), ldw, P(bd), Cin, Cout, Kw, int(transposed), stride, pad, dil, in_shift,
                          float(in_slope), act, float(act_slope), P(rd), ldr, float(scale), int(old is not None), P(od), ldo, rows, P(loutd), idt, odt)
    assert rc == 0, lib.kk_last_error()
    return host(od)


def reference(d, *, rows, transposed=False, stride=1, pad=0, dil=1, in_shift=0, in_slope=1.0, act=R.ACT_NONE, act_slope=0.0, scale=1.0, lin=None,
              lout=None, odt=F32):
    """-> (ref, bound) [B][rows][Cout] by the module docstring."""
    f32 = lambda v: float(np.float32(v))  # noqa: E731  (the kernel's arguments are floats)
    kw = dict(in_slope=f32(in_slope), act=act, act_slope=f32(act_slope), res=d["res"], scale=f32(scale), accumulate_into=d["old"], lin=lin, lout=lout,
              rows=rows, parts=True)
    Cout, Kw, Cin = d["w"].shape
    if transposed:
        ref, S, pre = R.conv_transpose1d(d["x"], d["w"], d["bias"], stride=stride, pad=pad, **kw)
        ntaps = -(-Kw // stride)
    else:
        ref, S, pre = R.conv1d(d["x"], d["w"], d["bias"], stride=stride, pad=pad, dil=dil, in_shift=in_shift, **kw)
        ntaps = Kw
    n = ntaps * (-(-Cin // 16) * 16)
    e = (n + 2) * U24 * S + (U24 * np.abs(d["bias"])[None, None, :] if d["bias"] is not None else 0.0)
    v = R.activation(pre, act, f32(act_slope))
    if act == R.ACT_LRELU:
        e = max(1.0, abs(f32(act_slope))) * e + U24 * np.abs(v)
    elif act == R.ACT_GELU:
        e = 1.13 * e + 0.5 * np.abs(pre) * (6 * U24 + U24 * np.abs(pre)) + 2 * U24 * np.abs(v)
    elif act == R.ACT_GELU_TANH:
        e = 1.13 * e + 0.5 * np.abs(pre) * 9 * U24 + 2 * U24 * np.abs(v)
    if d["res"] is not None:
        v = v + d["res"]
        e = e + U24 * np.abs(v)
    if f32(scale) != 1.0:
        v = v * f32(scale)
        e = abs(f32(scale)) * e + U24 * np.abs(v)
    if d["old"] is not None:
        v = v + d["old"]
        e = e + U24 * np.abs(v)
    if odt == BF16:
        e = e + 2.0**-8 * np.abs(v)
    return ref, 2.0 * e


def layout_ok(got, B, rows, Cout, lout):
    """-> the [B][rows][Cout] block, after the checks on everything around it and on the rows past each item's length."""
    assert np.all(got[:, Cout:] == SENT), "a pad column of the output was written"
    assert np.all(got[B * rows :] == SENT), "a row behind the last item was written"
    blk = got[: B * rows, :Cout].reshape(B, rows, Cout)
    assert np.isfinite(blk).all(), "non-finite output (a NaN pad element leaked, or a row was left unwritten over NaN)"
    for b, n in enumerate(lout if lout is not None else []):
        assert np.all(blk[b, n:] == 0.0), f"item {b}: rows from lout on are not zero"
    return blk


def check(lib, group, name, d, *, idt=F32, odt=F32, rows, lout=None, **kw):
    key = (group, name, idt, odt)
    got = launch(lib, key, d, idt=idt, odt=odt, rows=rows, lout=lout, **kw)
    B, Cout = d["x"].shape[0], d["w"].shape[0]
    blk = layout_ok(got, B, rows, Cout, lout)
    assert np.all(blk != SENT), "an output element inside [rows][Cout] was left unwritten"
    ref, bound = reference(d, rows=rows, lout=lout, odt=odt, **kw)
    worst = 0.0
    for b in range(B):
        n = lout[b] if lout is not None else rows
        if n:
            worst = max(worst, float((np.abs(blk[b, :n].astype(np.float64) - ref[b, :n]) / (bound[b, :n] + 1e-300)).max()))
    report(f"conv_generic/{group}/{name}/{idt}{odt}", ratio=worst)
    assert worst <= 1.0, worst
    return blk


# ------------------------------------------------------------------------------------------------ the cases
def conv_case(lib, group, name, *, L, Cin, Cout, Kw, s=1, p=0, dl=1, in_shift=0, idt=F32, odt=F32, res=False, old=False, bias=True, B=3, **kw):
    """A KK_CONV case on L stored input rows: rows and the lengths follow from the conv arithmetic ((L << in_shift) upsampled rows)."""
    up = 1 << in_shift
    rows = conv_rows(L * up, Kw, s, p, dl)
    lin = lens3(L)[:B]
    lout = [min(rows, conv_rows(n * up, Kw, s, p, dl)) for n in lin]
    d = case_data((group, name), B, L, Cin, Cout, Kw, rows, idt, odt, res=res, old=old, bias=bias)
    return check(lib, group, name, d, idt=idt, odt=odt, rows=rows, stride=s, pad=p, dil=dl, in_shift=in_shift, lin=lin, lout=lout, **kw)


def convT_case(lib, group, name, *, L, Cin, Cout, Kw, s, p, opad=0, idt=F32, odt=F32, res=False, old=False, B=3, **kw):
    rows = convT_rows(L, Kw, s, p, opad)
    lin = lens3(L)[:B]
    lout = [min(rows, convT_rows(n, Kw, s, p, opad)) for n in lin]
    d = case_data((group, name), B, L, Cin, Cout, Kw, rows, idt, odt, w_scale=1.0 / math.sqrt(-(-Kw // s) * Cin), res=res, old=old)
    return check(lib, group, name, d, idt=idt, odt=odt, rows=rows, transposed=True, stride=s, pad=p, lin=lin, lout=lout, **kw)


@pytest.mark.parametrize("Cin", [1, 7, 15, 16, 17, 50])
@pytest.mark.parametrize("Cout", [1, 22, 63, 64, 65])
@pytest.mark.parametrize("L", [1, 127, 128, 129])
def test_tile_edges(lib, L, Cout, Cin):
    """BM = 128 rows, BN = 64 columns, BK = 16 channels: one below, at and one above each; Cout 1 and 22 are the shapes the models send here."""
    conv_case(lib, "edges", f"L{L}_o{Cout}_i{Cin}", L=L, Cin=Cin, Cout=Cout, Kw=3, p=1)


TAPS = [(1, 1, 0, 1, 140), (7, 1, 9, 3, 140), (11, 1, 25, 5, 140), (3, 2, 1, 1, 140), (12, 6, 3, 1, 140), (4, 2, 0, 1, 141), (7, 1, 6, 1, 140)]


@pytest.mark.parametrize("taps", TAPS, ids=lambda t: "k%d_s%d_p%d_d%d_L%d" % t)
def test_taps(lib, taps):
    """(7, 1, 6, 1) is the causal form as the entry states it (symmetric padding Kw - 1; the rows past Lin are the caller's to drop): its first
    row reads six rows of left padding, its last six rows read past the input's end."""
    Kw, s, p, dl, L = taps
    conv_case(lib, "taps", "k%d_s%d_p%d_d%d" % taps[:4], L=L, Cin=20, Cout=24, Kw=Kw, s=s, p=p, dl=dl)


@pytest.mark.parametrize("Kw", [1, 3])
def test_in_shift(lib, Kw):
    """The nearest-upsampled input (row r >> 1) under taps: Kw 3 reads rows -1 (>> 1 stays negative: padding) and 2 Lin (past the end)."""
    conv_case(lib, "in_shift", f"k{Kw}", L=41, Cin=20, Cout=24, Kw=Kw, p=Kw // 2, in_shift=1)


@pytest.mark.parametrize("term", ["res", "scale", "acc", "all"])
@pytest.mark.parametrize("act", list(ACTS))
def test_epilogue(lib, act, term):
    conv_case(lib, "epilogue", f"{act}_{term}", L=70, Cin=24, Cout=22, Kw=3, p=1, act=ACTS[act], act_slope=0.2, res=term in ("res", "all"),
              scale=0.3 if term in ("scale", "all") else 1.0, old=term in ("acc", "all"))


@pytest.mark.parametrize("slope", [0.0, 0.1, 1.0])
def test_in_slope(lib, slope):
    conv_case(lib, "epilogue", f"in_slope{slope}", L=70, Cin=24, Cout=22, Kw=3, p=1, in_slope=slope)


CONVT = [(20, 10, 5, 0), (12, 6, 3, 0), (3, 2, 1, 0), (4, 2, 1, 0), (2, 4, 0, 0), (16, 8, 4, 3)]


@pytest.mark.parametrize("L", [1, 33, 129])
@pytest.mark.parametrize("cfg", CONVT, ids=lambda t: "k%d_s%d_p%d_op%d" % t)
def test_transposed(lib, cfg, L):
    """The polyphase form.  (2, 4, 0): phases 2 and 3 have no tap and store the bias alone.  (16, 8, 4) with output padding 3: Lo_rows is no
    multiple of the stride, so the last q of phases 3 .. 7 lies past the buffer's rows (the next item's first rows, or the guard rows)."""
    Kw, s, p, opad = cfg
    convT_case(lib, "transposed", "k%d_s%d_p%d_op%d_L%d" % (cfg + (L,)), L=L, Cin=20, Cout=24, Kw=Kw, s=s, p=p, opad=opad)


def test_transposed_epilogue(lib):
    convT_case(lib, "transposed", "k12_s6_res_lrelu_acc", L=33, Cin=20, Cout=24, Kw=12, s=6, p=3, act=R.ACT_LRELU, act_slope=0.2, res=True, old=True)


def dtype_cases(lib, idt, odt):
    conv_case(lib, "dtypes", "edge_L129_i17_o65", L=129, Cin=17, Cout=65, Kw=3, p=1, idt=idt, odt=odt)
    conv_case(lib, "dtypes", "taps_k12_s6", L=140, Cin=20, Cout=24, Kw=12, s=6, p=3, idt=idt, odt=odt)
    conv_case(lib, "dtypes", "in_shift_k3", L=41, Cin=20, Cout=24, Kw=3, p=1, in_shift=1, idt=idt, odt=odt)
    conv_case(lib, "dtypes", "epilogue_gelu_all", L=70, Cin=24, Cout=22, Kw=3, p=1, act=R.ACT_GELU, res=True, scale=0.3, old=True, in_slope=0.1,
              idt=idt, odt=odt)
    convT_case(lib, "dtypes", "convT_k12_s6_res_lrelu_acc", L=33, Cin=20, Cout=24, Kw=12, s=6, p=3, act=R.ACT_LRELU, act_slope=0.2, res=True,
               old=True, idt=idt, odt=odt)
    convT_case(lib, "dtypes", "convT_k16_s8_op3", L=33, Cin=20, Cout=24, Kw=16, s=8, p=4, opad=3, idt=idt, odt=odt)


@pytest.mark.parametrize("pair", PAIRS)
def test_dtypes(lib, pair):
    """One case of every group, and the edge case above all three tile sizes, in each of the kernel's four instantiations."""
    dtype_cases(lib, *pair)


@pytest.mark.parametrize("pair", PAIRS)
def test_batch_invariance(lib, pair):
    """Item 1 of the batch of three has the bits of item 1 run alone (another grid, other buffers, other pitches' pads)."""
    idt, odt = pair
    L, Cin, Cout, Kw, p = 129, 17, 65, 3, 1
    lens = lens3(L)
    d = case_data(("invariance", idt, odt), 3, L, Cin, Cout, Kw, L, idt, odt, res=True, old=True)
    kw = dict(idt=idt, odt=odt, rows=L, pad=p, act=R.ACT_GELU, scale=0.3)
    g3 = layout_ok(launch(lib, ("inv3", idt, odt), d, lin=lens, lout=lens, **kw), 3, L, Cout, lens)
    d1 = {k: (v[1:2] if k in ("x", "res", "old") else v) for k, v in d.items()}
    g1 = layout_ok(launch(lib, ("inv1", idt, odt), d1, lin=lens[1:2], lout=lens[1:2], **kw), 1, L, Cout, lens[1:2])
    assert lens[1] > 1 and np.any(g1[0, : lens[1]] != 0)
    assert same_bits(g3[1], g1[0])
    report(f"conv_generic/invariance/{idt}{odt}", worst=0.0)


# ------------------------------------------------------------------------------------------------ bits
def fma_chain(xrows, w, acc):
    """acc [rows][Cout] (float32) after acc = fmaf(x[r][c], w[co][c], acc) over c ascending, as float64 + one rounding (exactness asserted)."""
    for c in range(xrows.shape[1]):
        t = xrows[:, c, None].astype(np.float64) * w[None, :, c].astype(np.float64)  # 16-bit product of two bf16-grid values: exact
        a = acc.astype(np.float64)
        s = t + a
        bp = s - a
        assert np.all((a - (s - bp)) + (t - bp) == 0.0), "the float64 sum is not exact: the emulation would round twice"
        acc = s.astype(np.float32)
    return acc


@pytest.mark.parametrize("Kw,Cin", [(1, 13), (3, 17)], ids=["linear_k1_i13", "k3_i17"])
def test_bits_conv(lib, Kw, Cin):
    """f32 -> f32 on bf16-grid operands, lin / lout NULL (every row), bias + residual + scale 0.3: the kernel's float32 operation order."""
    rng = np.random.default_rng(seed_of("bits", Kw, Cin))
    B, L, Cout, p = 2, 37, 22, Kw // 2
    d = {"x": R.bf16_round(rng.standard_normal((B, L, Cin))), "w": R.bf16_round(rng.standard_normal((Cout, Kw, Cin))),
         "bias": rng.standard_normal(Cout).astype(np.float32), "res": rng.standard_normal((B, L, Cout)).astype(np.float32), "old": None}
    blk = layout_ok(launch(lib, ("bits", Kw, Cin), d, idt=F32, odt=F32, rows=L, pad=p, scale=0.3), B, L, Cout, None)
    want = np.zeros((B, L, Cout), np.float32)
    for b in range(B):
        acc = np.zeros((L, Cout), np.float32)
        for t in range(Kw):
            r = np.arange(L) - p + t
            ok = (r >= 0) & (r < L)
            xr = np.where(ok[:, None], d["x"][b, np.where(ok, r, 0)], np.float32(0.0))
            acc = fma_chain(xr, d["w"][:, t, :], acc)
        want[b] = ((acc + d["bias"][None, :]) + d["res"][b]) * np.float32(0.3)
    assert want.dtype == np.float32 and same_bits(blk, want)
    report(f"conv_generic/bits/k{Kw}_i{Cin}", worst=0.0)


def test_bits_transposed_tap_free_phase(lib):
    """Kw 2 < stride 4, pad 0: output rows with row % 4 >= 2 have no tap; they hold (bias + res) * scale, each one float32 rounding, for every
    live row, and the other rows differ from that."""
    rng = np.random.default_rng(seed_of("bits", "convT"))
    B, L, Cin, Cout, Kw, s = 3, 33, 20, 24, 2, 4
    rows = convT_rows(L, Kw, s, 0, 2)  # output padding 2: the last tap-free rows are live too
    lin = lens3(L)
    lout = [convT_rows(n, Kw, s, 0, 2) for n in lin]
    d = case_data(("bits", "convT"), B, L, Cin, Cout, Kw, rows, F32, F32, res=True)
    blk = layout_ok(launch(lib, ("bits", "convT"), d, idt=F32, odt=F32, rows=rows, transposed=True, stride=s, pad=0, scale=0.3, lin=lin, lout=lout),
                    B, rows, Cout, lout)
    want = (d["bias"][None, None, :] + d["res"]) * np.float32(0.3)
    for b, n in enumerate(lout):
        free = np.arange(n)[np.arange(n) % s >= Kw]
        assert same_bits(blk[b, free], want[b, free])
        if n:
            assert len(free) and not np.any(blk[b, : n : s] == want[b, : n : s])
    report("conv_generic/bits/convT_tap_free", worst=0.0)
