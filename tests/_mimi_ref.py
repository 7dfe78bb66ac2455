"""Plain numpy references of the operations of mlx-audio_amd/csrc/kk_mimi.hip, one function per kernel, for
tests/test_gpu_mimi_kernels.py.  tests/test_mimi_ref_cpu.py pins them (1e-12 against torch float64, exactly against the pieces of
oracle/mimi_oracle.py on data its fp32 arithmetic is exact on).

Two kinds:
  * float64 references (conv, conv_transposed, conv_cout1, rope, elu, gelu_tanh): the caller passes operands already rounded the way the
    kernel sees them (bf16 RNE where it reads bf16);
  * bit references in float32 (rvq_sum, upsample_dw, edge_pad, rvq_argmin, the carry ops): the library is built with -ffp-contract=off, so
    these kernels' few fp32 operations are reproduced operation for operation and the tests compare bits.

Tensors are frames-major: x [L][C]; conv weights are MLX's [O][K][I].
"""
import numpy as np


# ------------------------------------------------------------------------------------------------ number formats
def bf16_round(a):
    """float -> the nearest bf16 (ties to even), returned as float32.  Finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def elu(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def gelu_tanh(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v**3)))


def near_bf16_tie(e, rel=2.0**-14):
    """True where float64 `e` lies within rel * |e| of the midpoint of two neighbouring bf16 values (where a last-bit difference in how
    e was computed could change its bf16 rounding)."""
    e = np.abs(np.asarray(e, np.float64))
    out = np.zeros(e.shape, bool)
    nz = e > 0
    ulp = 2.0 ** (np.floor(np.log2(e[nz])) - 7)  # spacing of bf16 (8 significant bits) in e's binade
    frac = np.mod(e[nz] / ulp, 1.0)
    out[nz] = np.abs(frac - 0.5) * ulp <= rel * e[nz]
    return out


def avoid_elu_ties(x):
    """x (bf16 values) with every element whose elu(x) is near a bf16 tie replaced by |x| (elu of a positive bf16 value is itself: exact).
    Decided by the float64 reference alone; afterwards bf16(elu(x)) is known whatever the last bits of the device's exp are."""
    x = np.array(x, np.float32)
    bad = (x <= 0) & near_bf16_tie(elu(x))
    x[bad] = np.abs(x[bad])
    assert not ((x <= 0) & near_bf16_tie(elu(x))).any()
    return x


# ------------------------------------------------------------------------------------------------ float64 references
def conv(x, w, bias=None, *, pad=0, dil=1, stride=1, Lout=None, absum=False):
    """out[q] = bias + sum_k w[:, k, :] x[q * stride - pad + k * dil], rows outside [0, L) are zeros.  x [L][I], w [O][K][I] -> [Lout][O].
    absum: also sum |x w| + |bias| (the scale of the fp32 accumulation's rounding error)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    L, (O, K, _) = x.shape[0], w.shape
    if Lout is None:
        Lout = (L + pad - (K - 1) * dil - 1) // stride + 1
    out = np.zeros((Lout, O))
    ab = np.zeros((Lout, O))
    q = np.arange(Lout)
    for k in range(K):
        r = q * stride - pad + k * dil
        ok = (r >= 0) & (r < L)
        out[ok] += x[r[ok]] @ w[:, k, :].T
        ab[ok] += np.abs(x[r[ok]]) @ np.abs(w[:, k, :]).T
    if bias is not None:
        out += np.asarray(bias, np.float64)[None, :]
        ab += np.abs(np.asarray(bias, np.float64))[None, :]
    return (out, ab) if absum else out


def conv_transposed(x, w, bias=None, *, stride, pad=0, Lout=None, absum=False):
    """out[r * stride + k - pad] += w[:, k, :] x[r]  (no kernel flip), rows [0, Lout) kept.  x [L][I], w [O][K][I] -> [Lout][O]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    L, (O, K, _) = x.shape[0], w.shape
    full = (L - 1) * stride + K
    if Lout is None:
        Lout = full - pad
    out = np.zeros((max(full, Lout + pad), O))
    ab = np.zeros_like(out)
    for k in range(K):
        out[k : k + (L - 1) * stride + 1 : stride] += x @ w[:, k, :].T
        ab[k : k + (L - 1) * stride + 1 : stride] += np.abs(x) @ np.abs(w[:, k, :]).T
    out, ab = out[pad : pad + Lout], ab[pad : pad + Lout]
    if bias is not None:
        out = out + np.asarray(bias, np.float64)[None, :]
        ab = ab + np.abs(np.asarray(bias, np.float64))[None, :]
    return (out, ab) if absum else out


def conv_cout1(x, w, bias, *, pad):
    """SEANet's last conv: x [L][Cin] (already what the kernel multiplies: elu applied / rounded by the caller), w [K][Cin] ->
    (out [L], sum |x w| + |bias|)."""
    o, ab = conv(x, np.asarray(w, np.float64)[None], None if bias is None else [bias], pad=pad, Lout=np.asarray(x).shape[0], absum=True)
    return o[:, 0], ab[:, 0]


def rope(row, inv_freq, t, D, hd):
    """nn.RoPE(traditional) on one qkv row [>= 3 D] at position t: pairs (2 i, 2 i + 1) of every head of the q and k thirds rotated by the
    angle the kernel uses, float64 of the FP32 product float32(t) * inv_freq[i].  -> (new row, |x0| + |x1| per element: the error scale)."""
    row = np.array(row, np.float64)
    scale = np.zeros_like(row)
    ang = (np.float32(t) * np.asarray(inv_freq, np.float32)).astype(np.float64)  # [hd / 2]
    c, s = np.cos(ang), np.sin(ang)
    for base in range(0, 2 * D, hd):
        x0, x1 = row[base : base + hd : 2].copy(), row[base + 1 : base + hd : 2].copy()
        row[base : base + hd : 2] = x0 * c - x1 * s
        row[base + 1 : base + hd : 2] = x0 * s + x1 * c
        scale[base : base + hd : 2] = scale[base + 1 : base + hd : 2] = np.abs(x0) + np.abs(x1)
    return row, scale


# ------------------------------------------------------------------------------------------------ bit references (float32)
def rvq_sum(codes, cb):
    """codes [nq][Nf] int, cb [nq][bins][qdim] float32 -> (q_first, q_rest) [Nf][qdim] float32: row of code book 0; e_1, then + e_i ascending in
    fp32 (zeros for nq == 1).  Codes are clamped into [0, bins)."""
    cb = np.asarray(cb, np.float32)
    nq, bins, _ = cb.shape
    ids = np.clip(np.asarray(codes), 0, bins - 1)
    first = cb[0][ids[0]]
    rest = np.zeros_like(first)
    for i in range(1, nq):
        e = cb[i][ids[i]]
        rest = e.copy() if i == 1 else (rest + e).astype(np.float32)
    return first, rest


def upsample_dw(x, w, s):
    """x [Lin][C], w [2 s][C] float32 -> [Lin * s][C] float32: out[s t + j] = x[t] w[j] (+ x[t - 1] w[j + s] for t > 0), each product and the
    sum rounded to fp32."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    Lin, C = x.shape
    out = np.empty((Lin * s, C), np.float32)
    for t in range(Lin):
        for j in range(s):
            v = (x[t] * w[j]).astype(np.float32)
            if t > 0:
                v = (v + (x[t - 1] * w[j + s]).astype(np.float32)).astype(np.float32)
            out[t * s + j] = v
    return out


def edge_pad(x, left, Lp):
    x = np.asarray(x)
    return x[np.clip(np.arange(Lp) - left, 0, x.shape[0] - 1)]


def rvq_argmin(dots, c2, cb, residual):
    """dots [T][bins], c2 [bins], cb [bins][qdim], residual [T][qdim], all float32 -> (codes [T], new residual): v = c2 - dots in fp32, the
    first index of the smallest v below +inf (NaN never compares below), bins - 1 when there is none; residual - cb[code] in fp32."""
    v = (np.asarray(c2, np.float32)[None, :] - np.asarray(dots, np.float32)).astype(np.float32)
    bins = v.shape[1]
    codes = np.empty(v.shape[0], np.int32)
    for t in range(v.shape[0]):
        ok = v[t] < np.inf  # False for NaN and +inf
        codes[t] = bins - 1 if not ok.any() else int(np.flatnonzero(ok & (v[t] == v[t][ok].min()))[0])
    return codes, (np.asarray(residual, np.float32) - np.asarray(cb, np.float32)[codes]).astype(np.float32)


def state_shift(buf, S, n):
    """buf [rows >= S + n][C] of one item: rows [n, n + S) -> [0, S); the rest stays."""
    out = np.array(buf)
    out[:S] = np.asarray(buf)[n : n + S]
    return out


def state_edge_fill(buf, S):
    out = np.array(buf)
    out[:S] = out[S]
    return out
