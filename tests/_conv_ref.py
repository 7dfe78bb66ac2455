"""float64 restatements of the generic conv family (csrc/kk_conv.hip) and the streaming Linear (csrc/kk_linear_rows.hip), written from the op's
definition in the header of kk_conv.hip and the ABI comments of kk_op_conv1d / kk_op_linear_rows in include/kokoro_hip.h.  Plain NumPy, loops over
taps; pinned against torch float64 by tests/test_conv_ref_cpu.py.

Layouts: x [B][Lin][Cin], w [Cout][Kw][Cin] (the packed device form [Kw][Cin][ldw] is pack_w(w)), bias [Cout], res / accumulate_into
[B][rows][Cout], lin / lout per-item lengths (None = every row).  The caller passes operands as the kernel reads them (bf16 inputs already rounded)
and the float32 values of in_slope / act_slope / scale.

  conv1d            out[b][q][co]  = sum_t sum_ci w[co][t][ci] f(x[b][(q stride - pad + t dil) >> in_shift][ci]),  rows outside [0, lin[b]) are zero
  conv_transpose1d  out[b][op][co] = sum over (i, k) with i stride - pad + k = op, 0 <= i < lin[b], of w[co][k][ci] f(x[b][i][ci])
  f(v) = v if v > 0 else v in_slope  (in_slope 1: identity), or elu(v) = v if v > 0 else exp(v) - 1
  epilogue          v = pre + bias; v = act(v); v += res; v *= scale; v += accumulate_into; rows q >= lout[b] are exactly 0.
  linear_rows       out[b][t][:] = act(x[b][t] W^T + bias) for t < lens[b], zeros past it.

Each returns (ref, S): S is the float64 sum of |w f(x)| per output element (no bias), the scale of the dot product's rounding error.  With parts=True
the pre-activation value (dot + bias) comes third, for the error propagation of the tests' bounds."""
import math

import numpy as np

ACT_NONE, ACT_LRELU, ACT_GELU, ACT_GELU_TANH = 0, 1, 2, 4
_erf = np.vectorize(math.erf, otypes=[np.float64])


def bf16_round(a):
    """float -> the nearest bf16 (ties to even), returned as float32.  Finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def pack_w(w):
    """[Cout][Kw][Cin] -> ([Kw][Cin][ldw] float32, ldw): Cout rounded up to 64 columns, zero filled, as the loaders pack it."""
    O_, K, I = w.shape
    ldw = (O_ + 63) // 64 * 64
    p = np.zeros((K, I, ldw), np.float32)
    p[:, :, :O_] = np.transpose(w, (1, 2, 0))
    return p, ldw


def gelu(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def gelu_tanh(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v**3)))


def activation(v, act, act_slope=0.0):
    if act == ACT_NONE:
        return v
    if act == ACT_LRELU:
        return np.where(v > 0, v, v * float(act_slope))
    if act == ACT_GELU:
        return gelu(v)
    if act == ACT_GELU_TANH:
        return gelu_tanh(v)
    raise ValueError(act)


def input_transform(x, in_slope=1.0, elu=False):
    x = np.asarray(x, np.float64)
    if elu:
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    return np.where(x > 0, x, x * float(in_slope))


def _lens(v, B, full):
    return [full] * B if v is None else [int(n) for n in v]


def _epilogue(dot, S, bias, act, act_slope, res, scale, accumulate_into, lout, parts):
    B, rows, _ = dot.shape
    pre = dot + (0.0 if bias is None else np.asarray(bias, np.float64)[None, None, :])
    v = activation(pre, act, act_slope)
    if res is not None:
        v = v + np.asarray(res, np.float64)
    v = v * float(scale)
    if accumulate_into is not None:
        v = v + np.asarray(accumulate_into, np.float64)
    for b, n in enumerate(_lens(lout, B, rows)):
        v[b, n:] = 0.0
    return (v, S, pre) if parts else (v, S)


def conv1d(x, w, bias=None, *, stride=1, pad=0, dil=1, in_shift=0, in_slope=1.0, elu=False, act=ACT_NONE, act_slope=0.0, res=None, scale=1.0,
           accumulate_into=None, lin=None, lout=None, rows, parts=False):
    """`rows` output rows per item; see the module docstring."""
    B, Lin, Cin = x.shape
    w64 = np.asarray(w, np.float64)
    Cout, Kw, _ = w64.shape
    xt = input_transform(x, in_slope, elu)
    dot = np.zeros((B, rows, Cout))
    S = np.zeros((B, rows, Cout))
    q = np.arange(rows)
    for b, n in enumerate(_lens(lin, B, Lin)):
        for t in range(Kw):
            r = q * stride - pad + t * dil
            ok = r >= 0
            r = np.where(ok, r, 0) >> in_shift
            ok &= r < n
            xs = np.where(ok[:, None], xt[b, np.where(ok, r, 0)], 0.0)  # [rows][Cin]
            dot[b] += xs @ w64[:, t, :].T
            S[b] += np.abs(xs) @ np.abs(w64[:, t, :]).T
    return _epilogue(dot, S, bias, act, act_slope, res, scale, accumulate_into, lout, parts)


def conv_transpose1d(x, w, bias=None, *, stride=1, pad=0, in_slope=1.0, elu=False, act=ACT_NONE, act_slope=0.0, res=None, scale=1.0,
                     accumulate_into=None, lin=None, lout=None, rows, parts=False):
    """Scatter form: input row i and tap k land on output row i stride - pad + k."""
    B, Lin, Cin = x.shape
    w64 = np.asarray(w, np.float64)
    Cout, Kw, _ = w64.shape
    xt = input_transform(x, in_slope, elu)
    dot = np.zeros((B, rows, Cout))
    S = np.zeros((B, rows, Cout))
    for b, n in enumerate(_lens(lin, B, Lin)):
        i = np.arange(n)
        for k in range(Kw):
            op = i * stride - pad + k
            ok = (op >= 0) & (op < rows)
            dot[b, op[ok]] += xt[b, i[ok]] @ w64[:, k, :].T  # (distinct i give distinct op: no repeated index)
            S[b, op[ok]] += np.abs(xt[b, i[ok]]) @ np.abs(w64[:, k, :]).T
    return _epilogue(dot, S, bias, act, act_slope, res, scale, accumulate_into, lout, parts)


def linear_rows(x, w, bias=None, act=ACT_NONE, lens=None, parts=False):
    """x [B][rows][K], w [N][K] -> out [B][rows][N], zeros from lens[b] on."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    dot = x64 @ w64.T
    S = np.abs(x64) @ np.abs(w64).T
    return _epilogue(dot, S, bias, act, 0.0, None, 1.0, None, lens, parts)
