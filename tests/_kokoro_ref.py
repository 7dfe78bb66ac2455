"""Numpy restatements of the Kokoro forward's glue, embedding, source, STFT, attention and recurrence kernels (csrc/kk_misc.hip, kk_albert.hip,
kk_source.hip, kk_lstm.hip), shared by tests/test_kokoro_ref_cpu.py (which pins them against torch float64, the oracle and _sampler_ref) and
tests/test_gpu_kokoro_kernels.py.  Two kinds:

  *  float64 statements of the operation, for the cases where a derived bound is asserted;
  *  float32 statements op for op, for the cases where bits are asserted.  The library is built with -ffp-contract=off and the compiler's
     correctly rounded fp32 divide, so np.float32 arithmetic (one rounding per operation), np.fmod (exact) and np.cumsum in float32 (a
     sequential sum) are the kernels' operations.  No bit-level tricks: bf16 rounding goes through torch's conversion.
"""
import math

import numpy as np
import torch

f32 = np.float32
UP = 300  # samples per F0 entry in the source entry points


def bf16_round(a):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# ------------------------------------------------------------------------------------------------ glue (exact)
def masked_rows(vals, lens):
    """vals [B][rows][C] with rows >= len zeroed."""
    out = np.array(vals, copy=True)
    for b, n in enumerate(lens):
        out[b, n:] = 0
    return out


def embedding(ids, table, lens):
    B, T = ids.shape
    out = np.zeros((B, T, table.shape[1]), table.dtype)
    for b, n in enumerate(lens):
        out[b, :n] = table[ids[b, :n]]
    return out


def fill_style(ref_s, soff, S, rows, lens):
    out = np.zeros((ref_s.shape[0], rows, S), ref_s.dtype)
    for b, n in enumerate(lens):
        out[b, :n] = ref_s[b, soff : soff + S]
    return out


def alignment(dur, lenT, Fmax):
    """kokoro.py:151-156: token t owns max(dur_t, 0) frames, in order; frames past Fmax are dropped; the tail of frame_idx is 0."""
    B, Tmax = dur.shape
    idx = np.zeros((B, Fmax), np.int32)
    lenF = np.zeros(B, np.int32)
    for b in range(B):
        d = np.maximum(dur[b, : min(int(lenT[b]), Tmax)].astype(np.int64), 0)
        fr = np.repeat(np.arange(d.size, dtype=np.int32), d)[:Fmax]
        idx[b, : fr.size] = fr
        lenF[b] = fr.size
    return idx, lenF


def gather_rows(x, idx, lenF):
    B, F = idx.shape
    out = np.zeros((B, F, x.shape[2]), x.dtype)
    for b in range(B):
        out[b, : lenF[b]] = x[b, idx[b, : lenF[b]]]
    return out


def lens4(lenF, up0, up1, hop):
    F = np.asarray(lenF, np.int64)
    return np.stack([2 * F, 2 * F * up0, np.where(F > 0, 2 * F * up0 * up1 + 1, 0), 2 * F * up0 * up1 * hop]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ float64 statements
def style_fc(ref_s, soff, wT, bias):
    """-> (out [B][N], S [B][N] = sum |w s| + |bias|)."""
    s = np.asarray(ref_s, np.float64)[:, soff : soff + 128]
    w, b = np.asarray(wT, np.float64), np.asarray(bias, np.float64)
    return s @ w + b, np.abs(s) @ np.abs(w) + np.abs(b)


def duration(x, W, bias, speed):
    """x [T][Cin] -> (d [T] = sum_o sigmoid(x W + bias) / speed, S [T][nout] = sum |x w| + |bias|, sg [T][nout])."""
    x, W, bias = np.asarray(x, np.float64), np.asarray(W, np.float64), np.asarray(bias, np.float64)
    acc = x @ W + bias
    sg = 1.0 / (1.0 + np.exp(-acc))
    return sg.sum(1) / float(speed), np.abs(x) @ np.abs(W) + np.abs(bias), sg


def albert_embed(ids, word, pos, typ, ln_w, ln_b, eps):
    """modules.py:451-465 for one item: ids [L] -> y [L][E] float64, plus the pieces the bound needs."""
    x = np.asarray(word, np.float64)[ids] + np.asarray(pos, np.float64)[: len(ids)] + np.asarray(typ, np.float64)[0]
    mean = x.mean(1, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    z = d * rstd
    return z * np.asarray(ln_w, np.float64) + np.asarray(ln_b, np.float64), dict(x=x, d=d, var=var, rstd=rstd, z=z)


def attention(qkv, heads, scale=0.125):
    """qkv [L][>= 3 hs] (q | k | v, head h at columns 64 h) -> (out [L][hs], W = sum_k p_k |v_k| [L][hs], A [L][heads] = max_k sum_d |q_d k_d| scale)."""
    L, hs = qkv.shape[0], heads * 64
    t = np.asarray(qkv, np.float64)
    out, W, A = np.zeros((L, hs)), np.zeros((L, hs)), np.zeros((L, heads))
    for h in range(heads):
        q, k, v = (t[:, i * hs + h * 64 : i * hs + h * 64 + 64] for i in range(3))
        s = (q @ k.T) * scale
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        out[:, h * 64 : h * 64 + 64] = p @ v
        W[:, h * 64 : h * 64 + 64] = p @ np.abs(v)
        A[:, h] = (np.abs(q) @ np.abs(k).T).max(1) * scale
    return out, W, A


def lstm(xproj, whT, L, u_gate=0.0, u_dot=0.0, u_op=0.0):
    """One item of the bidirectional recurrence (modules.py:152-239): xproj [rows][2][4H] (gates i, f, g, o), whT [2][H][4H] -> out [L][2H].
    With the u_* terms it also carries a bound on |h_fp32 - h| forward through the steps (returned second), see test_gpu_kokoro_kernels.py:
    u_dot per term of a dot, u_gate absolute per activation, u_op per rounded product or sum."""
    H = whT.shape[1]
    xp, wh = np.asarray(xproj, np.float64), np.asarray(whT, np.float64)
    out, err = np.zeros((L, 2 * H)), np.zeros((L, 2 * H))
    for dr in range(2):
        h, c, eh, ec = np.zeros(H), np.zeros(H), np.zeros(H), np.zeros(H)
        for step in range(L):
            t = L - 1 - step if dr else step
            acc = xp[t, dr] + h @ wh[dr]
            eacc = (H + 1) * u_dot * (np.abs(xp[t, dr]) + np.abs(h) @ np.abs(wh[dr])) + eh @ np.abs(wh[dr])
            i, f, o = (1.0 / (1.0 + np.exp(-acc[k * H : (k + 1) * H])) for k in (0, 1, 3))
            g = np.tanh(acc[2 * H : 3 * H])
            ei, ef, eo = (0.25 * eacc[k * H : (k + 1) * H] + u_gate for k in (0, 1, 3))
            eg = eacc[2 * H : 3 * H] + u_gate
            cn = f * c + i * g
            ec = np.abs(c) * ef + f * ec + np.abs(g) * ei + i * eg + 3 * u_op * (np.abs(f * c) + np.abs(i * g))
            c = cn
            h = o * np.tanh(c)
            eh = np.abs(np.tanh(c)) * eo + o * (ec + u_gate) + u_op * np.abs(h)
            out[t, dr * H : (dr + 1) * H] = h
            err[t, dr * H : (dr + 1) * H] = eh
    return out, err


# ------------------------------------------------------------------------------------------------ source
def source_phase32(f0, up=UP):
    """source_phase_kernel for one item, float32 op for op: f0 [L2] -> phase [9][L2] = ((cumsum(python_mod(f0 h / 24000, 1)) * 2) * pi) * up."""
    f0 = np.asarray(f0, f32)
    h = np.arange(1, 10, dtype=np.int32).astype(f32)[:, None]
    fn = (f0[None, :] * h).astype(f32)
    r = np.fmod((fn / f32(24000.0)).astype(f32), f32(1.0)).astype(f32)  # C fmodf: exact, sign of the dividend
    r = np.where(r < 0, (r + f32(1.0)).astype(f32), r).astype(f32)
    cum = np.cumsum(r, axis=1, dtype=f32)  # sequential
    return (((cum * f32(2.0)).astype(f32) * f32(math.pi)).astype(f32) * f32(up)).astype(f32)


def source_arg32(phase, L2, up=UP):
    """The sine's argument of source_sample_kernel for n < L2 * up, float32 op for op (interpolate.py:80-106: un-clamped low index that wraps to
    the LAST sample, high index clamped, un-fused blend).  phase [9][>= L2] -> (ph [9][N] float32, lo_w [N], hi [N])."""
    xs, xh = f32(1.0 / up), f32(0.5 * (1.0 / up))
    n = np.arange(L2 * up, dtype=np.int32).astype(f32)
    x = (((n * xs).astype(f32) + xh).astype(f32) - f32(0.5)).astype(f32)
    xl = np.floor(x).astype(f32)
    lo = xl.astype(np.int32)
    hi = np.minimum(lo + 1, L2 - 1)
    fr = (x - xl).astype(f32)
    omf = (f32(1.0) - fr).astype(f32)
    lo_w = np.where(lo < 0, lo + L2, lo)
    ph = ((phase[:, lo_w] * omf[None]).astype(f32) + (phase[:, hi] * fr[None]).astype(f32)).astype(f32)
    return ph, lo_w, hi


def noise_amp32(f0, up=UP):
    """(uv [N], namp [N]) in float32 as the kernel forms them: uv = f0 > 10, namp = uv * 0.003 + ((1 - uv) * 0.1) / 3."""
    f = np.repeat(np.asarray(f0, f32), up)
    uv = (f > f32(10.0)).astype(f32)
    namp = ((uv * f32(0.003)).astype(f32) + (((f32(1.0) - uv).astype(f32) * f32(0.1)).astype(f32) / f32(3.0)).astype(f32)).astype(f32)
    return uv, namp


def source_sample(ph, f0, noise, lin_w, lin_b, up=UP):
    """tanh(sum_h ((sin(ph_h) 0.1) uv + namp nz_h) w_h + b) in float64 on the float32 argument `ph` [9][N]; noise [N][9] or None.
    -> (out [N], pre [N] the pre-tanh sum, T [N] = sum_h |w_h| (|0.1 sin| + |namp nz|), sw_abs [N] = sum_h |sw_h w_h|)."""
    uv, namp = noise_amp32(f0, up)
    uv, namp = uv.astype(np.float64), namp.astype(np.float64)
    w = np.asarray(lin_w, np.float64)[:, None]
    nz = np.zeros(ph.shape) if noise is None else np.asarray(noise, np.float64).T
    s = np.sin(ph.astype(np.float64)) * float(f32(0.1))
    sw = s * uv + namp * nz
    pre = (sw * w).sum(0) + float(f32(lin_b))
    T = (np.abs(w) * (np.abs(s) * uv + np.abs(namp * nz))).sum(0)
    return np.tanh(pre), pre, T, np.abs(sw * w).sum(0)


# ------------------------------------------------------------------------------------------------ Philox + Box-Muller (kk_philox.h, kk_source.hip)
def philox4_vec(seed, ctr, sub):
    """csrc/kk_philox.h's philox4 for arrays of counters: ctr uint64 [n], sub a scalar -> uint32 [4][n]."""
    M = np.uint64(0xFFFFFFFF)
    ctr = np.asarray(ctr, np.uint64)
    c = [ctr & M, (ctr >> np.uint64(32)) & M, np.full(ctr.shape, sub, np.uint64), np.full(ctr.shape, 0x4B4B5352, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]  # 32 x 32 bits: fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c).astype(np.uint32)


def unit24(r):
    """((float)(r >> 8) + 0.5f) * 2^-24 in float32 (the sum rounds for r >> 8 >= 2^23; the top value gives exactly 1)."""
    return (((r >> np.uint32(8)).astype(f32) + f32(0.5)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)


def source_normals(seed, b, Nmax, n_count):
    """The nine normals per sample of source_sample_kernel's Philox mode (ctr = b * Nmax + n, sub = g in 0..2, two Box-Muller pairs per draw),
    Box-Muller in float64 on the kernel's float32 uniforms and float32 angle.  -> (z [n_count][9] float64, r [n_count][9] the radius)."""
    ctr = np.uint64(b) * np.uint64(Nmax) + np.arange(n_count, dtype=np.uint64)
    z, rad = np.zeros((n_count, 12)), np.zeros((n_count, 12))
    for g in range(3):
        r = philox4_vec(seed, ctr, g)
        for pair in range(2):
            a, bq = unit24(r[2 * pair]).astype(np.float64), unit24(r[2 * pair + 1])
            th = (f32(6.28318530717958647692) * bq).astype(f32).astype(np.float64)
            rr = np.sqrt(-2.0 * np.log(a))
            z[:, 4 * g + 2 * pair], z[:, 4 * g + 2 * pair + 1] = rr * np.cos(th), rr * np.sin(th)
            rad[:, 4 * g + 2 * pair] = rad[:, 4 * g + 2 * pair + 1] = rr
    return z[:, :9], rad[:, :9]


# ------------------------------------------------------------------------------------------------ STFT(20)
def stft_tables():
    """kk_source.hip's make_tables: symmetric Hann(20) and the twiddles, double precision rounded to float32, exact where they are exact."""
    n = np.arange(20)
    hann = (0.5 * (1.0 - np.cos(2.0 * np.pi * n / 19.0))).astype(f32)
    cs, sn = np.cos(2.0 * np.pi * n / 20.0).astype(f32), np.sin(2.0 * np.pi * n / 20.0).astype(f32)
    cs[[0, 5, 10, 15]] = [1, 0, -1, 0]
    sn[[0, 5, 10, 15]] = [0, 1, 0, -1]
    return hann, cs, sn


def reflect_index(m, N):
    """Index of padded sample m (any integer) in a signal of N >= 1 samples, numpy's reflect mode (no edge repeat, folded as often as needed)."""
    p = 2 * (N - 1)
    m = np.abs(m)
    m = m % p if p else m * 0
    return np.where(m >= N, p - m, m)


def stft20(x, N, window=None, exact_tables=False):
    """MLXSTFT.transform (istftnet.py:463-495) of x[:N]: n_fft 20, hop 5, centre, reflect padding.  float64 sums on the float32 frame products
    x w (one rounding, as the kernel) and the float32 twiddles; exact_tables = True uses float64 window and twiddles (for the torch.stft pin).
    -> (re [Tf][11], im [Tf][11], S [Tf] = sum |x w|) with Tf = N // 5 + 1; bins 0 and 10 carry im = 0."""
    hann, cs, sn = stft_tables()
    n = np.arange(20)
    if exact_tables:
        hann, cs, sn = (0.5 * (1.0 - np.cos(2.0 * np.pi * n / 19.0)) if window is None else window), np.cos(2 * np.pi * n / 20), np.sin(2 * np.pi * n / 20)
    Tf = N // 5 + 1
    m = 5 * np.arange(Tf)[:, None] + n[None, :] - 10
    xs = np.asarray(x)[reflect_index(m, N)]
    fr = (xs.astype(np.float64) * hann) if exact_tables else (xs.astype(f32) * hann).astype(f32).astype(np.float64)
    kj = (np.arange(11)[:, None] * n[None, :]) % 20
    re = fr @ cs.astype(np.float64)[kj].T
    im = -(fr @ sn.astype(np.float64)[kj].T)
    im[:, [0, 10]] = 0.0
    return re, im, np.abs(fr).sum(1)


# ------------------------------------------------------------------------------------------------ the duration head's random case
U24 = 2.0**-24


def duration_bound(S, sg, d, speed, Cin):
    """|dur_f - d|: per output an FMA chain of Cin terms plus the bias ((Cin + 2) u S), through a sigmoid of slope <= 1/4 whose expf (2 ulp), sum
    and quotient add <= 5 u; <= 10 rounded adds on the way to the total (serial over the o0 passes, 6 shuffle steps); the quotient by speed."""
    return ((0.25 * (Cin + 2) * U24 * S + 5 * U24).sum(1) + 10 * U24 * sg.sum(1)) / float(speed) + 2 * U24 * np.abs(d)


def duration_case(seed, bf16):
    """Random operands of the duration head: B = 3 items of lengths {9, 1, 0} in 9 rows, Cin = 40, nout = 70 (two o0 passes).  -> dict with the
    float64 d, its bound and the mask of rows whose rounding the bound decides (farther than it from a half-integer and from 1)."""
    rng = np.random.default_rng(seed)
    B, T, Cin, nout = 3, 9, 40, 70
    lens = [9, 1, 0]
    x = rng.standard_normal((B, T, Cin)).astype(f32)
    if bf16:
        x = bf16_round(x)
    W = (rng.standard_normal((Cin, nout)) / math.sqrt(Cin)).astype(f32)
    bias = (rng.standard_normal(nout) * 0.5 - 1.0).astype(f32)
    speed = np.array([1.0, 0.7, 1.3], f32)
    d, bound, sure = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T), bool)
    for b, n in enumerate(lens):
        if n:
            d[b, :n], S, sg = duration(x[b, :n], W, bias, speed[b])
            bound[b, :n] = duration_bound(S, sg, d[b, :n], speed[b], Cin)
            half = np.abs(d[b, :n] - (np.floor(d[b, :n]) + 0.5))
            sure[b, :n] = (half > bound[b, :n]) & (np.abs(d[b, :n] - 1.0) > bound[b, :n])
    return dict(B=B, T=T, Cin=Cin, nout=nout, lens=lens, x=x, W=W, bias=bias, speed=speed, d=d, bound=bound, sure=sure)


DURATION_SEEDS = (101, 102)  # test_kokoro_ref_cpu.py checks that the float64 reference alone leaves <= 2 % of their rows undecided
