"""GPU parity tests of the Kokoro forward's glue kernels (csrc/kk_misc.hip), the Albert embedding and attention (kk_albert.hip), the harmonic source
and STFT(20) (kk_source.hip) and the LSTM recurrence (kk_lstm.hip), kernel by kernel through kk_op_* entries that make the calls kk_forward makes,
against tests/_kokoro_ref.py (pinned by tests/test_kokoro_ref_cpu.py).

Inputs carry NaN in pad columns, in rows past the valid length and in table rows no valid id names; outputs start as a sentinel; the source's phase
scratch has a NaN guard in front of it, so a low index that fails to wrap reads NaN.  Every case reports its worst error over bound (report()).

Bits (the build has -ffp-contract=off; np.float32 reproduces the operations): embedding, fill_style, gather_rows, copy_slice, convert, lens,
alignment, the constructed roundings of the duration head, the source's phase accumulator.

Bounds (u = 2^-24; the device expf / sinf / tanhf / atan2f are taken within 2 ulp, which HIP's math-API table states as 1 - 2):
  style_fc   (128 + 2) u (sum |w s| + |bias|): one FMA chain of 128 and the bias add.
  duration   _kokoro_ref.duration_bound; dur = rint(d) wherever the float64 d is farther than that from a half-integer and from 1.
  embed      x = (w + p) + t carries e_x = 2u (|w| + |p| + |t|); the mean 16u mean|x| + mean e_x (8 serial adds, 6 shuffle steps); d = x - mean carries
             e_d = e_x + e_mean + u |d|; var relatively 2 rms(e_d) / sqrt(var) + 16u (Cauchy-Schwarz on sum d^2); rstd half that + 4u; the output
             |ln_w| (e_d rstd + |z| (rel_rstd + 3u)) + 2u |y|, with a factor 2 of slack; bf16 + 2^-8 |y|.
  source     the sine's ARGUMENT is formed in float32 exactly as the kernel forms it (checked as bits through the phase scratch), so what is left is
             sum_h |w_h| 0.1 * 2^-22 uv (sinf, 2 ulp of a value <= 1) + 4u sum_h |w_h| (|0.1 sin| + |namp nz|) + 10u (sum |sw w| + |b|) + 2^-22 (tanhf).
  philox     z = r cos / sin(theta): -2 ln a carries dL = max(2^-20.41, 3 * 2^-23 r^2) (__logf: 2^-21.41 absolute on [0.5, 2], 3 ulp elsewhere, times 2),
             r = sqrt(.) min(dL / r, sqrt dL) + u r; __sincosf 2^-21 + 4 pi u (the hardware sine on theta / 2 pi, itself rounded); the injected copy
             is rounded to float32 (u |z|).  Output: sum_h |w_h| namp dz_h plus the source bound of both runs.
  stft20     re / im: e_c = 22 u S, S = sum_j |x_j w_j| (product, 20 FMAs, one of slack); |X|: sqrt 2 e_c + 4u |X|; angle, compared wrapped and only
             where |X| exceeds the magnitude bound: (pi / 2) sqrt 2 e_c / |X| + 2^-21 (atan2f); bf16 + 2^-8 |ref|.
  attention  a score carries e_s = 18u A, A = max_k sum_d |q_d k_d| / 8 (four FMA chains of 16, two adds); weights relatively 2 e_s + 8u; the running
             sums (2 ceil(L / 8) + 16) u (a rescale and an FMA per key of a partition, the merge); numerator and denominator: bound = 2 (2 e_s + 8u +
             (2 ceil(L / 8) + 16) u) W, W = sum_k p_k |v_k|.  bf16 generic kernel + 2^-8 |ref|.  Matrix-core kernel: e_s = 70u A (64 exact products
             summed in fp32, the log2 e scale), P rounded to bf16 under a float32 denominator 2^-8 W, the output 2^-8 |ref|.
  lstm       carried forward through the steps by _kokoro_ref.lstm: the dot (H + 1) u (|xproj| + sum |w h|) + sum |w| e_h, gates of slope 1/4 (tanh 1)
             + 2^-22, c and h by the product rule + 3u per rounded term; it grows by about sum_j |Wh_j| per step, so Wh is drawn with that sum = 1;
             factor 2 of slack; bf16 output + 2^-8 |ref| (the state stays fp32)."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

import _kokoro_ref as R
from _util import report

pytestmark = pytest.mark.gpu

SENT, ISENT = -512.0, -7777  # -512 is exact in bf16; no output here comes near either
U24 = 2.0**-24
F32, BF16 = 0, 1
NOISE_ZERO, NOISE_INJECTED, NOISE_PHILOX = 0, 1, 2
DT = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]


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


_LIVE = []  # every device tensor of a test lives until the test is over: an operand built inside a call's argument list would otherwise be
# freed before the launch, and the allocator hands its block to the next operand built there


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def live(t):
    _LIVE.append(t)
    return t


def dev(a, dtype=F32):
    return live(torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).to(tdt(dtype)).cuda())


def idev(a):
    return live(torch.tensor(np.ascontiguousarray(a, dtype=np.int32)).cuda())


def sent(shape, dtype=F32):
    return live(torch.full(shape, SENT, dtype=tdt(dtype), device="cuda"))


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def ok(lib, rc):
    assert rc == 0, lib.kk_last_error()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def values(rng, shape, dtype):
    v = rng.standard_normal(shape).astype(np.float32)
    return R.bf16_round(v) if dtype == BF16 else v


def embed(vals, rows, ld, fill=np.nan):
    """vals [B][r][c] inside a [B][rows][ld] buffer of `fill`."""
    B, r, c = vals.shape
    buf = np.full((B, rows, ld), fill, np.float32)
    buf[:, :r, :c] = vals
    return buf


def nan_past(vals, lens):
    out = np.array(vals, np.float32, copy=True)
    for b, n in enumerate(lens):
        out[b, n:] = np.nan
    return out


def slice_only(buf, c0, c1):
    """True when every column outside [c0, c1) still holds the sentinel."""
    m = np.ones(buf.shape, bool)
    m[..., c0:c1] = False
    return bool(np.all(buf[m] == SENT))


def ratio(got, ref, bound):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "non-finite output (a NaN pad element leaked)"
    return float((np.abs(got - ref) / (bound + 1e-300)).max()) if got.size else 0.0


def cast(a, dtype):
    return R.bf16_round(a) if dtype == BF16 else np.asarray(a, np.float32)


LENS3 = lambda n: [n, 1, 0]  # noqa: E731  B = 3: full, one row, none


# ------------------------------------------------------------------------------------------------ glue kernels, bits
@pytest.mark.parametrize("dtype", DT)
def test_embedding(lib, dtype):
    rng = np.random.default_rng(11)
    B, T, C_, V, ldo = 3, 7, 37, 5, 40  # 7 * 37 = 259 elements: a second block of three threads
    lens = LENS3(T)
    table = np.concatenate([rng.standard_normal((V, C_)).astype(np.float32), np.full((1, C_), np.nan, np.float32)])
    ids = rng.integers(0, V, (B, T))
    ids[0, :2] = [0, V - 1]
    for b, n in enumerate(lens):
        ids[b, n:] = V  # the NaN row: not read past the length
    out = sent((B, T, ldo), dtype)
    ok(lib, lib.kk_op_kokoro_embedding(stream(), B, P(idev(ids)), P(dev(table)), P(out), ldo, C_, T, P(idev(lens)), dtype))
    got = host(out)
    assert same_bits(got[:, :, :C_], cast(R.embedding(ids, table, lens), dtype)) and slice_only(got, 0, C_)
    out2 = sent((B, T, ldo), dtype)  # len == NULL: every row
    ids2 = np.minimum(ids, V - 1)
    ok(lib, lib.kk_op_kokoro_embedding(stream(), B, P(idev(ids2)), P(dev(table)), P(out2), ldo, C_, T, None, dtype))
    assert same_bits(host(out2)[:, :, :C_], cast(table[ids2], dtype))
    report(f"kokoro/embedding/{dtype}", worst=0.0)


@pytest.mark.parametrize("dtype", DT)
def test_fill_style(lib, dtype):
    rng = np.random.default_rng(12)
    B, rows, S, soff, coff, ldo = 3, 3, 100, 128, 5, 112  # 3 * 100 = 300 elements
    lens = LENS3(rows)
    ref_s = np.full((B, 256), np.nan, np.float32)
    ref_s[:, soff : soff + S] = rng.standard_normal((B, S))
    out = sent((B, rows, ldo), dtype)
    ok(lib, lib.kk_op_kokoro_fill_style(stream(), B, P(dev(ref_s)), soff, P(out), ldo, coff, S, rows, P(idev(lens)), dtype))
    got = host(out)
    assert same_bits(got[:, :, coff : coff + S], cast(R.fill_style(ref_s, soff, S, rows, lens), dtype)) and slice_only(got, coff, coff + S)
    report(f"kokoro/fill_style/{dtype}", worst=0.0)


@pytest.mark.parametrize("dtype", DT)
def test_gather_rows(lib, dtype):
    rng = np.random.default_rng(13)
    B, T, Fm, C_, ldi, coff, ldo = 3, 4, 9, 37, 39, 3, 45  # 9 * 37 = 333 elements
    dur = np.array([[3, 0, 4, 5], [1, 1, 1, 1], [2, 2, 2, 2]], np.int32)
    idx, lenF = R.alignment(dur, [4, 1, 0], Fm)
    assert lenF.tolist() == [9, 1, 0]
    x = values(rng, (B, T, C_), dtype)
    out = sent((B, Fm, ldo), dtype)
    ok(lib, lib.kk_op_kokoro_gather_rows(stream(), B, P(dev(embed(x, T, ldi), dtype)), ldi, T, P(idev(idx)), Fm, P(idev(lenF)), P(out), ldo, coff, C_, dtype))
    got = host(out)
    assert same_bits(got[:, :, coff : coff + C_], R.gather_rows(x, idx, lenF)) and slice_only(got, coff, coff + C_)
    report(f"kokoro/gather_rows/{dtype}", worst=0.0)


@pytest.mark.parametrize("dtype", DT)
def test_copy_slice(lib, dtype):
    rng = np.random.default_rng(14)
    B, rows, C_, ldi, coff, ldo = 3, 7, 37, 38, 6, 50
    lens = LENS3(rows)
    x = values(rng, (B, rows, C_), dtype)
    out = sent((B, rows, ldo), dtype)
    ok(lib, lib.kk_op_kokoro_copy_slice(stream(), B, P(dev(embed(nan_past(x, lens), rows, ldi), dtype)), ldi, P(out), ldo, coff, C_, rows, P(idev(lens)), dtype))
    got = host(out)
    assert same_bits(got[:, :, coff : coff + C_], R.masked_rows(x, lens)) and slice_only(got, coff, coff + C_)
    report(f"kokoro/copy_slice/{dtype}", worst=0.0)


@pytest.mark.parametrize("pair", [(F32, F32), (F32, BF16), (BF16, F32)], ids=["f32_f32", "f32_bf16", "bf16_f32"])
def test_convert(lib, pair):
    sdt, ddt = pair
    rng = np.random.default_rng(15)
    B, rows, C_, lds, ldd = 2, 7, 37, 38, 41
    x = rng.standard_normal((B, rows, C_)).astype(np.float32)
    x[0, 0, :4] = [1.00390625, 1.01171875, -0.0, 3.0e38]  # ties of the bf16 rounding (to even: down, up), a signed zero, near the top
    x = cast(x, sdt)
    out = sent((B, rows, ldd), ddt)
    ok(lib, lib.kk_op_kokoro_convert(stream(), B, P(dev(embed(x, rows, lds), sdt)), sdt, lds, P(out), ddt, ldd, C_, rows))
    got = host(out)
    assert same_bits(got[:, :, :C_], cast(x, ddt)) and slice_only(got, 0, C_)
    report(f"kokoro/convert/{sdt}{ddt}", worst=0.0)


def test_convert_refuses_bf16_to_bf16(lib):
    x, out = dev(np.zeros((1, 2, 8)), BF16), sent((1, 2, 8), BF16)
    assert lib.kk_op_kokoro_convert(stream(), 1, P(x), BF16, 8, P(out), BF16, 8, 8, 2) != 0
    assert np.all(host(out) == SENT)


def test_lens(lib):
    rng = np.random.default_rng(16)
    for lenF in ([5, 0, 1], rng.integers(0, 40, 70) * (rng.random(70) > 0.2)):  # 70 items: a second block; F = 0 gives 0 frames, not 1
        B = len(lenF)
        out = torch.full((4, B), ISENT, dtype=torch.int32, device="cuda")
        ok(lib, lib.kk_op_kokoro_lens(stream(), B, P(idev(lenF)), P(out), 10, 6, 5))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), R.lens4(lenF, 10, 6, 5))
    report("kokoro/lens", worst=0.0)


def alignment_case(Tmax):
    """-> dur [B][Tmax], lenT, Fmax: sums below, at and above Fmax (cut inside a token), zeros and negatives among the durations, an empty item,
    and durations past lenT that must not count."""
    if Tmax == 1:
        return np.array([[3], [0], [-1], [5], [9]], np.int32), [1, 1, 1, 1, 0], 3
    if Tmax == 7:
        dur = np.array([[2, 0, -3, 3, 1, 0, 2], [3, 0, 4, 5, 1, 1, 1], [1, 1, 0, 100, 100, 100, 100], [4, 4, 4, 4, 4, 4, 4]], np.int32)
        return dur, [7, 7, 3, 0], 8
    rng = np.random.default_rng(17)
    Fmax = 600
    dur = rng.integers(-2, 5, (4, Tmax)).astype(np.int32)
    lenT = [Tmax, 300, Tmax, 0]
    assert np.maximum(dur[0], 0).sum() > Fmax + 3 and np.maximum(dur[1, :300], 0).sum() < Fmax
    dur[2][np.cumsum(np.maximum(dur[2], 0)) > 100] = 0  # item 2 sums to exactly Fmax: 100 frames, a run of empty tokens, the last token owns the rest
    dur[2, Tmax - 1] = Fmax - np.maximum(dur[2, : Tmax - 1], 0).sum()
    assert np.maximum(dur[2], 0).sum() == Fmax
    return dur, lenT, Fmax


@pytest.mark.parametrize("Tmax", [1, 7, 512])
def test_alignment(lib, Tmax):
    dur, lenT, Fmax = alignment_case(Tmax)
    B = dur.shape[0]
    idx_ref, lenF_ref = R.alignment(dur, lenT, Fmax)
    assert (lenF_ref == Fmax).any() and (lenF_ref < Fmax).any() and (lenF_ref == 0).any()
    idx = torch.full((B, Fmax), ISENT, dtype=torch.int32, device="cuda")
    lenF = torch.full((B,), ISENT, dtype=torch.int32, device="cuda")
    ok(lib, lib.kk_op_kokoro_alignment(stream(), B, P(idev(dur)), Tmax, P(idev(lenT)), P(idx), P(lenF), Fmax))
    torch.cuda.synchronize()
    assert np.array_equal(lenF.cpu().numpy(), lenF_ref)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)  # the tail from lenF on is written 0
    report(f"kokoro/alignment/T{Tmax}", worst=0.0)


def test_alignment_refuses_513_tokens(lib):
    dur, lenT = idev(np.ones((1, 513))), idev([513])
    idx = torch.full((1, 8), ISENT, dtype=torch.int32, device="cuda")
    lenF = torch.full((1,), ISENT, dtype=torch.int32, device="cuda")
    assert lib.kk_op_kokoro_alignment(stream(), 1, P(dur), 513, P(lenT), P(idx), P(lenF), 8) != 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == ISENT).all() and int(lenF.cpu()[0]) == ISENT


def run_duration(lib, x, W, bias, speed, lens, dtype, ldx):
    B, T, Cin = x.shape
    dur = torch.full((B, T), ISENT, dtype=torch.int32, device="cuda")
    dur_f = sent((B, T))
    xd = dev(embed(nan_past(x, lens), T, ldx), dtype)
    ok(lib, lib.kk_op_kokoro_duration(stream(), B, P(xd), ldx, P(dev(W)), P(dev(bias)), Cin, W.shape[1], P(dev(speed)), P(dur), P(dur_f), T,
                                      P(idev(lens)), dtype))
    torch.cuda.synchronize()
    return dur.cpu().numpy(), dur_f.cpu().numpy()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("nout,want,want_f", [(50, 12, 12.5), (54, 14, 13.5), (130, 32, 32.5)])
def test_duration_rounding(lib, dtype, nout, want, want_f):
    """Zero weights and bias: every sigmoid is exactly 0.5 (expf(-0) = 1), the sum nout / 2 is exact, and speed 2 lands on a tie: half to even.
    speed 100 gives a quotient under 1/2, which is clamped to 1.  130 outputs: three passes of the o0 loop."""
    rng = np.random.default_rng(18)
    B, T, Cin = 3, 6, 5
    lens = LENS3(T)
    x = values(rng, (B, T, Cin), dtype)
    speed = np.array([2.0, 100.0, 2.0], np.float32)
    dur, dur_f = run_duration(lib, x, np.zeros((Cin, nout), np.float32), np.zeros(nout, np.float32), speed, lens, dtype, 8)
    ref = np.zeros((B, T), np.int32)
    ref_f = np.zeros((B, T), np.float32)
    ref[0], ref_f[0] = want, want_f
    ref[1, 0], ref_f[1, 0] = 1, np.float32(0.5 * nout) / np.float32(100.0)
    assert np.array_equal(dur, ref) and same_bits(dur_f, ref_f)
    report(f"kokoro/duration_rounding/{dtype}/{nout}", worst=0.0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("seed", R.DURATION_SEEDS)
def test_duration_random(lib, dtype, seed):
    c = R.duration_case(seed, dtype == BF16)
    dur, dur_f = run_duration(lib, c["x"], c["W"], c["bias"], c["speed"], c["lens"], dtype, c["Cin"] + 3)
    valid = np.zeros(dur.shape, bool)
    for b, n in enumerate(c["lens"]):
        valid[b, :n] = True
    assert not dur[~valid].any() and not dur_f[~valid].any()
    worst = ratio(dur_f[valid], c["d"][valid], c["bound"][valid])
    skipped = float((valid & ~c["sure"]).sum() / valid.sum())
    report(f"kokoro/duration/{dtype}/s{seed}", worst=worst, skipped=skipped)
    assert worst <= 1.0
    assert skipped <= 0.02
    assert np.array_equal(dur[c["sure"]], np.maximum(np.rint(c["d"][c["sure"]]), 1).astype(np.int32))


@pytest.mark.parametrize("soff", [0, 128])
@pytest.mark.parametrize("N", [1, 255, 257, 3000])
def test_style_fc(lib, N, soff):
    rng = np.random.default_rng(seed_of("style_fc", N, soff))
    B = 2
    ref_s = np.full((B, 256), np.nan, np.float32)
    ref_s[:, soff : soff + 128] = rng.standard_normal((B, 128))
    wT, bias = rng.standard_normal((128, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    out = sent((B, N + 3))  # flat [B * N] plus a tail that must stay
    ok(lib, lib.kk_op_kokoro_style_fc(stream(), B, P(dev(ref_s)), soff, P(dev(wT)), P(dev(bias)), P(out), N))
    got = host(out).reshape(-1)
    ref, S = R.style_fc(ref_s, soff, wT, bias)
    worst = ratio(got[: B * N].reshape(B, N), ref, (128 + 2) * U24 * S)
    report(f"kokoro/style_fc/N{N}/soff{soff}", worst=worst)
    assert worst <= 1.0 and np.all(got[B * N :] == SENT)


# ------------------------------------------------------------------------------------------------ Albert embedding
def run_albert(lib, E, dtype, T=6, V=9, B=3):
    rng = np.random.default_rng(seed_of("albert", E))
    lens = LENS3(T)
    word = np.concatenate([rng.standard_normal((V, E)).astype(np.float32), np.full((1, E), np.nan, np.float32)])
    pos, typ = rng.standard_normal((T, E)).astype(np.float32), rng.standard_normal((2, E)).astype(np.float32)
    typ[1] = np.nan  # token type 0 only
    lw, lb = (1.0 + 0.3 * rng.standard_normal(E)).astype(np.float32), rng.standard_normal(E).astype(np.float32)
    ids = rng.integers(0, V, (B, T))
    ids[0, :2] = [0, V - 1]
    for b, n in enumerate(lens):
        ids[b, n:] = V
    ldo = E + 8
    out = sent((B, T, ldo), dtype)
    rc = lib.kk_op_albert_embed(stream(), B, P(idev(ids)), P(dev(word)), P(dev(pos)), P(dev(typ)), P(dev(lw)), P(dev(lb)), 1e-12, P(out), ldo, E, T,
                                P(idev(lens)), dtype)
    return rc, host(out), (ids, word, pos, typ, lw, lb, lens)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("E", [64, 128, 200, 512])
def test_albert_embed(lib, E, dtype):
    rc, got, (ids, word, pos, typ, lw, lb, lens) = run_albert(lib, E, dtype)
    ok(lib, rc)
    assert slice_only(got, 0, E)
    worst = 0.0
    for b, n in enumerate(lens):
        assert not got[b, n:, :E].any()
        if not n:
            continue
        y, q = R.albert_embed(ids[b, :n], word, pos, typ, lw, lb, 1e-12)
        e_x = 2 * U24 * (np.abs(word[ids[b, :n]]) + np.abs(pos[:n]) + np.abs(typ[0]))
        e_mean = 16 * U24 * np.abs(q["x"]).mean(1, keepdims=True) + e_x.mean(1, keepdims=True)
        e_d = e_x + e_mean + U24 * np.abs(q["d"])
        rel_rstd = 0.5 * (2 * np.sqrt((e_d**2).mean(1, keepdims=True)) / np.sqrt(q["var"]) + 16 * U24) + 4 * U24
        bound = 2 * (np.abs(lw) * (e_d * q["rstd"] + np.abs(q["z"]) * (rel_rstd + 3 * U24)) + 2 * U24 * np.abs(y))
        if dtype == BF16:
            bound = bound + 2.0**-8 * np.abs(y)
        worst = max(worst, ratio(got[b, :n, :E], y, bound))
    report(f"kokoro/albert_embed/E{E}/{dtype}", worst=worst)
    assert worst <= 1.0


def test_albert_embed_refuses_513(lib):
    rc, got, _ = run_albert(lib, 513, F32)
    assert rc != 0 and np.all(got == SENT)


# ------------------------------------------------------------------------------------------------ source + STFT
def run_source(lib, f0, len2, lenN, lw, lb, mode, noise, seed, dtype, ldhar):
    """-> phase [B][9][L2], har_source [B][300 L2], har [B][60 L2 + 1][ldhar].  The phase scratch sits behind a guard of NaN."""
    B, L2 = f0.shape
    guard = torch.full((64 + B * 9 * L2,), float("nan"), device="cuda")
    phase = guard[64:]
    phase.fill_(SENT)
    hs = sent((B, 300 * L2))
    har = sent((B, 60 * L2 + 1, ldhar), dtype)
    keep = [dev(f0), idev(len2) if len2 is not None else None, idev(lenN) if lenN is not None else None, dev(lw), dev(noise) if noise is not None else None]
    ok(lib, lib.kk_op_source_stft_ragged(stream(), B, P(keep[0]), L2, P(keep[1]), P(keep[2]), P(keep[3]), float(lb), mode, P(keep[4]), C.c_uint64(seed),
                                         P(phase), P(hs), P(har), ldhar, dtype))
    return host(phase).reshape(B, 9, L2), host(hs), host(har)


def f0_curve(rng, B, L2, lens):
    f0 = (rng.standard_normal((B, L2)) * 80 + 150).astype(np.float32)
    f0[:, 1::5] = -3.0  # negative: the r < 0 branch of the python-style modulo; unvoiced
    return nan_past(f0, lens)


@pytest.mark.parametrize("L2", [1, 48, 1024, 1025, 2100])
def test_source_phase_bits(lib, L2):
    """1024 entries are staged per pass: 1024 is one full pass, 1025 a second pass of one, 2100 three."""
    rng = np.random.default_rng(seed_of("phase", L2))
    lens = [L2, (L2 + 1) // 2, 0]
    f0 = f0_curve(rng, 3, L2, lens)
    if L2 == 1:
        f0[0, 0] = -3.0
    lw = rng.standard_normal(9).astype(np.float32)
    phase, hs, _ = run_source(lib, f0, lens, [300 * n for n in lens], lw, 0.05, NOISE_ZERO, None, 0, F32, 22)
    for b, n in enumerate(lens):
        assert same_bits(phase[b, :, :n], R.source_phase32(f0[b, :n])), (b, n)
        assert np.all(phase[b, :, n:] == SENT) and not hs[b, 300 * n :].any()
    assert np.isfinite(hs).all()
    report(f"kokoro/source_phase/L{L2}", worst=0.0)


def source_bound(T, sw_abs, uv, lw, lb):
    return (np.abs(lw).sum() * 0.1 * 2.0**-22) * uv + 4 * U24 * T + 10 * U24 * (sw_abs + abs(lb)) + 2.0**-22


def test_source_sample_injected(lib):
    rng = np.random.default_rng(31)
    B, L2 = 3, 7
    lens = [7, 3, 0]
    f0 = nan_past(np.tile(np.array([150.0, -3.0, 10.0, 0.0, 220.0, 95.5, 330.0], np.float32), (B, 1)), lens)  # 10.0 exactly is unvoiced (f0 > 10)
    lw, lb = (rng.standard_normal(9) * 0.7).astype(np.float32), np.float32(0.05)
    noise = rng.standard_normal((B, 300 * L2, 9)).astype(np.float32)
    for b, n in enumerate(lens):
        noise[b, 300 * n :] = np.nan
    phase, hs, _ = run_source(lib, f0, lens, [300 * n for n in lens], lw, lb, NOISE_INJECTED, noise, 0, F32, 22)
    worst = {}
    for b, n in enumerate(lens):
        assert not hs[b, 300 * n :].any()
        if not n:
            continue
        assert same_bits(phase[b, :, :n], R.source_phase32(f0[b, :n]))
        ph, lo_w, hi = R.source_arg32(phase[b], n)
        assert (lo_w[:150] == n - 1).all() and lo_w[150] == 0 and hi[-150:].tolist() == [n - 1] * 150  # the wrap and the clamp are in the case
        ref, pre, T, sw_abs = R.source_sample(ph, f0[b, :n], noise[b, : 300 * n], lw, lb)
        uv, _ = R.noise_amp32(f0[b, :n])
        r = np.abs(hs[b, : 300 * n].astype(np.float64) - ref) / source_bound(T, sw_abs, uv, lw, lb)
        assert np.isfinite(hs[b]).all()
        worst[b] = float(r.max())
        worst[f"first150_{b}"] = float(r[:150].max())
    report("kokoro/source_sample/injected", worst=max(worst.values()), **{f"w_{k}": v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


def test_source_sample_philox(lib):
    rng = np.random.default_rng(32)
    B, L2, seed = 2, 3, 0x5EED0123456789AB
    lens = [3, 2]
    f0 = nan_past(np.array([[150.0, 0.0, 220.0], [-3.0, 95.5, 0.0]], np.float32), lens)
    lw, lb = (rng.standard_normal(9) * 0.7).astype(np.float32), np.float32(0.05)
    Nmax = 300 * L2
    lenN = [300 * n for n in lens]
    z = np.zeros((B, Nmax, 9))
    rad = np.zeros((B, Nmax, 9))
    for b in range(B):
        z[b], rad[b] = R.source_normals(seed, b, Nmax, Nmax)
    phase, hs_p, _ = run_source(lib, f0, lens, lenN, lw, lb, NOISE_PHILOX, None, seed, F32, 22)
    _, hs_i, _ = run_source(lib, f0, lens, lenN, lw, lb, NOISE_INJECTED, z.astype(np.float32), 0, F32, 22)
    _, hs_q, _ = run_source(lib, f0, lens, lenN, lw, lb, NOISE_PHILOX, None, seed + 1, F32, 22)
    worst = 0.0
    for b, n in enumerate(lens):
        N = 300 * n
        ph, _, _ = R.source_arg32(phase[b], n)
        ref, pre, T, sw_abs = R.source_sample(ph, f0[b, :n], z[b, :N], lw, lb)
        uv, namp = R.noise_amp32(f0[b, :n])
        r = rad[b, :N]
        dL = np.maximum(2.0**-20.41, 3 * 2.0**-23 * r * r)
        dz = np.minimum(dL / np.maximum(r, 1e-30), np.sqrt(dL)) + U24 * r + r * (2.0**-21 + 4 * math.pi * U24) + U24 * np.abs(z[b, :N])
        base = source_bound(T, sw_abs, uv, lw, lb)
        e_noise = (np.abs(lw)[None, :] * namp[:, None].astype(np.float64) * dz).sum(1)
        worst = max(worst, ratio(hs_p[b, :N], hs_i[b, :N].astype(np.float64), e_noise + 2 * base), ratio(hs_p[b, :N], ref, e_noise + base))
        assert not hs_p[b, N:].any() and (hs_q[b, :N] != hs_p[b, :N]).mean() > 0.99  # another seed, another signal
    report("kokoro/source_sample/philox", worst=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DT)
def test_stft20(lib, dtype):
    rng = np.random.default_rng(33)
    B, L2 = 5, 5
    lenN = [1500, 300, 20, 5, 0]
    ldhar = 24 if dtype == BF16 else 25
    f0 = (rng.standard_normal((B, L2)) * 60 + 200).astype(np.float32)
    lw = (rng.standard_normal(9) * 0.7).astype(np.float32)
    _, hs, har = run_source(lib, f0, None, lenN, lw, 0.05, NOISE_ZERO, None, 0, dtype, ldhar)
    assert slice_only(har, 0, 22) and (np.abs(hs[:, 1490:]) > 1e-3).any(1).all()  # the signal goes on past every lenN
    worst_m = worst_p = 0.0
    left_out = []
    pi_out = float(cast(np.array([math.pi], np.float32), dtype)[0])
    for b, N in enumerate(lenN):
        Tf = N // 5 + 1 if N else 0
        assert not har[b, Tf:, :22].any()
        if not N:
            continue
        re, im, S = R.stft20(hs[b], N)
        mag, ang = np.hypot(re, im), np.arctan2(im, re)
        e_c = 22 * U24 * S[:, None]
        b_mag = math.sqrt(2) * e_c + 4 * U24 * mag + (2.0**-8 * mag if dtype == BF16 else 0)
        worst_m = max(worst_m, ratio(har[b, :Tf, :11], mag, b_mag))
        strong = mag > b_mag
        left_out.append(1.0 - float(strong.mean()))
        b_ang = (math.pi / 2) * math.sqrt(2) * e_c / np.maximum(mag, 1e-300) + 2.0**-21 + (2.0**-8 * np.abs(ang) if dtype == BF16 else 0)
        dphi = np.abs(np.angle(np.exp(1j * (har[b, :Tf, 11:22].astype(np.float64) - ang))))
        worst_p = max(worst_p, float((dphi / b_ang)[strong].max()))
        edge = har[b, :Tf][:, [11, 21]]  # bins 0 and 10: a +0 imaginary part, so the angle is exactly 0 or pi
        assert np.all((edge == 0) | (edge == pi_out))
        sure = np.abs(re[:, [0, 10]]) > e_c
        assert np.array_equal((edge == pi_out)[sure], (re[:, [0, 10]] < 0)[sure])
    report(f"kokoro/stft20/{dtype}", worst=max(worst_m, worst_p), worst_mag=worst_m, worst_phase=worst_p, left_out=max(left_out))
    assert worst_m <= 1.0 and worst_p <= 1.0


# ------------------------------------------------------------------------------------------------ attention
ATT_SHAPES = [(33, [1, 5, 32, 33], 3), (130, [128, 129, 5, 0], 1), (260, [257, 33, 1, 130], 3), (33, [33, 1, 5, 32], 1)]
ATT_KINDS = ["f32", "bf16_mfma", "bf16_generic"]


def attention_bound(kind, W, A, L, ref):
    es = (70 if kind == "bf16_mfma" else 18) * U24 * A
    bound = 2 * (2 * es + 8 * U24 + (2 * math.ceil(L / 8) + 16) * U24)
    bound = np.repeat(bound, 64, axis=1) * W
    if kind == "bf16_mfma":
        bound = bound + 2.0**-8 * W
    if kind != "f32":
        bound = bound + 2.0**-8 * np.abs(ref)
    return bound


def run_attention(lib, kind, qkv, lens, heads, T_rows):
    """qkv [B][T_rows][3 hs] -> out [B][T_rows][ldo]; pitches padded (the matrix-core kernel needs multiples of 8, the generic bf16 one gets odd ones)."""
    dtype = F32 if kind == "f32" else BF16
    B, hs = qkv.shape[0], heads * 64
    ld, ldo = (3 * hs + 3, hs + 1) if kind == "bf16_generic" else (3 * hs + 8, hs + 8)
    out = sent((B, T_rows, ldo), dtype)
    xd = dev(embed(nan_past(qkv, lens), T_rows, ld), dtype)
    ok(lib, lib.kk_op_attention(stream(), B, P(xd), ld, T_rows, P(idev(lens)), heads, P(out), ldo, dtype))
    return host(out)


def check_attention(kind, got, qkv, lens, heads, name):
    hs = heads * 64
    assert slice_only(got, 0, hs)
    worst = 0.0
    for b, L in enumerate(lens):
        assert not got[b, L:, :hs].any()
        if L:
            ref, W, A = R.attention(qkv[b, :L], heads)
            worst = max(worst, ratio(got[b, :L, :hs], ref, attention_bound(kind, W, A, L, ref)))
    report(name, worst=worst)
    assert worst <= 1.0


@pytest.mark.parametrize("kind", ATT_KINDS)
@pytest.mark.parametrize("shape", ATT_SHAPES, ids=[f"T{s[0]}_h{s[2]}" for s in ATT_SHAPES])
def test_attention(lib, shape, kind):
    T_rows, lens, heads = shape
    rng = np.random.default_rng(seed_of("attention", T_rows, heads))
    qkv = values(rng, (len(lens), T_rows, 3 * heads * 64), F32 if kind == "f32" else BF16)
    got = run_attention(lib, kind, qkv, lens, heads, T_rows)
    check_attention(kind, got, qkv, lens, heads, f"kokoro/attention/{kind}/T{T_rows}_h{heads}")


@pytest.mark.parametrize("kind", ATT_KINDS)
def test_attention_late_maximum(lib, kind):
    """Keys grow along the query's direction, so the running maximum moves at almost every key and what was accumulated is rescaled by factors far
    from 1 (the scores span about 16)."""
    rng = np.random.default_rng(41)
    T_rows, lens, heads = 130, [129, 70], 1
    u = rng.standard_normal(64)
    u /= np.linalg.norm(u)
    qkv = 0.3 * rng.standard_normal((2, T_rows, 192))
    qkv[:, :, :64] += 16.0 * u
    qkv[:, :, 64:128] += (np.arange(T_rows)[None, :, None] / 129.0) * 8.0 * u
    qkv = cast(qkv.astype(np.float32), F32 if kind == "f32" else BF16)
    got = run_attention(lib, kind, qkv, lens, heads, T_rows)
    check_attention(kind, got, qkv, lens, heads, f"kokoro/attention/{kind}/late_max")


# ------------------------------------------------------------------------------------------------ LSTM recurrence
def run_lstm(lib, H, L, dtype):
    rng = np.random.default_rng(seed_of("lstm", H, L))
    B, lens, ldo = 3, LENS3(L), 2 * H + 8
    xproj = rng.standard_normal((B, L, 2, 4 * H)).astype(np.float32)
    whT = (rng.uniform(-1, 1, (2, H, 4 * H)) * (2.0 / H)).astype(np.float32)  # sum_j |w| = 1 per gate row
    out = sent((B, L, ldo), dtype)
    rc = lib.kk_op_lstm(stream(), B, P(dev(nan_past(xproj, lens))), P(dev(whT)), H, L, P(idev(lens)), P(out), ldo, dtype)
    return rc, host(out), xproj, whT, lens


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("L", [1, 9])
@pytest.mark.parametrize("H", [16, 48, 256])
def test_lstm(lib, H, L, dtype):
    rc, got, xproj, whT, lens = run_lstm(lib, H, L, dtype)
    ok(lib, rc)
    assert slice_only(got, 0, 2 * H)
    worst = growth = 0.0
    for b, n in enumerate(lens):
        assert not got[b, n:, : 2 * H].any()
        if n:
            ref, err = R.lstm(xproj[b], whT, n, u_gate=2.0**-22, u_dot=U24, u_op=U24)
            worst = max(worst, ratio(got[b, :n, : 2 * H], ref, 2 * err + (2.0**-8 * np.abs(ref) if dtype == BF16 else 0)))
            growth = max(growth, float(err[n - 1, :H].max() / err[0, :H].max()))
    report(f"kokoro/lstm/H{H}/L{L}/{dtype}", worst=worst, bound_growth=growth)
    assert worst <= 1.0


@pytest.mark.parametrize("H", [8, 272])
def test_lstm_refuses(lib, H):
    B, L = 1, 2
    out = sent((B, L, 2 * H))
    rc = lib.kk_op_lstm(stream(), B, P(dev(np.zeros((B, L, 2, 4 * H)))), P(dev(np.zeros((2, H, 4 * H)))), H, L, None, P(out), 2 * H, F32)
    assert rc != 0 and np.all(host(out) == SENT)
