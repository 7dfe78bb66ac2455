"""float64 references, in plain numpy, of what mlx-audio_amd/csrc/kk_norm.hip computes: instance-norm statistics, AdaIN apply
(+ activation, + the depth-wise pooling transposed conv), LayerNorm / AdaLayerNorm, and the step from per-tile column sums to
mean / rstd / folded AdaIN parameters.  Tensors are frames-major ([rows][channels]); every function takes ONE item of a batch and
converts what it is given to float64 first, so a caller that hands over the bf16-rounded operands gets the reference on exactly the
numbers the kernel reads (a bf16 value is exact in fp32 and in fp64).  tests/test_norm_ref_cpu.py pins these against torch."""
import numpy as np

ACT_NONE, ACT_LRELU, ACT_SNAKE = 0, 1, 3  # KK_ACT_* (mlx-audio_amd/_lib.py)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def instnorm_stats(x, n, eps=1e-5):
    """x [rows][C] -> (mean [C], 1 / sqrt(var + eps) [C]) over the first n rows; two passes, ddof 0; 0 / 0 for n == 0."""
    x = _f64(x)
    C = x.shape[1]
    if n == 0:
        return np.zeros(C), np.zeros(C)
    v = x[:n]
    mean = v.sum(0) / n
    var = ((v - mean) ** 2).sum(0) / n
    return mean, 1.0 / np.sqrt(var + eps)


def activation(y, act, slope=0.0, alpha=None):
    if act == ACT_LRELU:
        return np.where(y > 0, y, y * slope)
    if act == ACT_SNAKE:
        a = np.ones(y.shape[-1]) if alpha is None else _f64(alpha)
        return y + (1.0 / a) * np.sin(a * y) ** 2
    assert act == ACT_NONE, act
    return y


def adain(x, n, gb, act=ACT_NONE, slope=0.0, alpha=None, pool_w=None, pool_b=None, eps=1e-5):
    """x [rows][C], gb [2C] = gamma | beta  ->  act((1 + gamma) * xn + beta) over the first n rows: [n][C].
    With pool_w [C][3] / pool_b [C]: then the depth-wise ConvTranspose1d(k3, s2, p1) and one zero row in FRONT: [2n][C]."""
    x, gb = _f64(x), _f64(gb)
    C = x.shape[1]
    mean, rstd = instnorm_stats(x, n, eps)
    y = activation((1.0 + gb[:C]) * ((x[:n] - mean) * rstd) + gb[C : 2 * C], act, slope, alpha)
    if pool_w is None:
        return y
    if n == 0:
        return np.zeros((0, C))
    w, b = _f64(pool_w), _f64(pool_b)
    full = np.zeros((2 * n + 1, C))  # un-cropped transposed conv: input row m lands on rows 2m + k, k = 0..2
    for k in range(3):
        full[k : k + 2 * n : 2] += y * w[:, k]
    ct = full[1 : 2 * n] + b  # padding 1 crops one row at each end: 2n - 1 rows
    return np.concatenate([np.zeros((1, C)), ct], 0)


def layernorm(x, res, n, C, w=None, b=None, gb=None, eps=1e-5, act=ACT_NONE, slope=0.0):
    """x (+ res) [rows][>= C] -> LayerNorm over the first C channels of the first n rows: [n][C].
    Affine: y * w + b, or with gb [2C] the AdaLayerNorm form (1 + gamma) * y + beta."""
    t = _f64(x)[:n, :C]
    if res is not None:
        t = t + _f64(res)[:n, :C]
    mean = t.sum(1, keepdims=True) / C
    var = ((t - mean) ** 2).sum(1, keepdims=True) / C
    y = (t - mean) / np.sqrt(var + eps)
    if gb is not None:
        gb = _f64(gb)
        y = (1.0 + gb[:C]) * y + gb[C : 2 * C]
    else:
        y = y * _f64(w) + _f64(b)
    return activation(y, act, slope)


def fold(mean, rstd, gb):
    """pa = rstd * (1 + gamma), pb = beta - mean * pa."""
    mean, rstd, gb = _f64(mean), _f64(rstd), _f64(gb)
    C = mean.shape[0]
    pa = rstd * (1.0 + gb[:C])
    return pa, gb[C : 2 * C] - mean * pa


def finalize_tiles(partials, L, eps=1e-5, gb=None):
    """partials [ntiles][2][C]: un-shifted column sums / sums of squares per tile, taken AS GIVEN (the fp32 values).
    -> mean, rstd, pa, pb (pa = pb = None without gb); mean = rstd = 0 for L == 0."""
    p = _f64(partials)
    C = p.shape[2]
    if L == 0:
        mean, rstd = np.zeros(C), np.zeros(C)
    else:
        S, SS = p[:, 0].sum(0), p[:, 1].sum(0)
        mean = S / L
        var = np.maximum(SS / L - mean * mean, 0.0)
        rstd = 1.0 / np.sqrt(var + eps)
    pa, pb = fold(mean, rstd, gb) if gb is not None else (None, None)
    return mean, rstd, pa, pb
