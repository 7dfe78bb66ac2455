"""The CSM sampler's rule (include/kokoro_hip.h, kk_csm_sampler) and its device RNG, restated in numpy: float64 arithmetic for the rule, exact
integer arithmetic for Philox4x32-10.  Shared by test_csm_sampler_cpu.py and test_gpu_csm_sampler.py."""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123 philox4x32-10: ctr four and key two 32-bit words -> four 32-bit words."""
    c = [int(x) & M32 for x in ctr]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def philox4(seed, ctr, sub):
    """csrc/kk_philox.h: counter words (ctr low, ctr high, sub, a fixed tag), key = seed."""
    return philox4x32_10([ctr & M32, (ctr >> 32) & M32, sub, 0x4B4B5352], [seed & M32, (seed >> 32) & M32])


def device_uniform(seed, sid, pos, cb):
    """The uniform of (seed, stream id, position, code book): ((out[0] >> 8) + 0.5) 2^-24, exact in float32."""
    r = philox4(int(seed), ((int(sid) & M32) << 32) | (int(pos) & M32), int(cb))
    return np.float32((float(r[0] >> 8) + 0.5) / 16777216.0)


def sorted_row(l):
    """order (logit descending, index ascending; NaN reads as -inf), p (whole vocabulary, temperature 1) and l - l_max along it, float64."""
    l = np.asarray(l, np.float64).copy()
    l[np.isnan(l)] = -np.inf
    order = np.lexsort((np.arange(l.size), -l))
    ls = l[order]
    with np.errstate(invalid="ignore"):
        d = np.where(ls == ls[0], 0.0, ls - ls[0])
    e = np.exp(d)
    return order, e / e.sum(), d


def kept(l, top_k=0, top_p=0.0, min_p=0.0, min_keep=1, dp=0.0):
    """n = min(n_k, n_p, n_m); dp moves the two thresholds (relative) for the admissible-set tests."""
    order, p, d = sorted_row(l)
    V = p.size
    n_k = top_k if 0 < top_k < V else V
    n_p = n_m = V
    if 0.0 < top_p < 1.0:
        before = np.concatenate([[0.0], np.cumsum(p)[:-1]])
        out = np.nonzero(~(before < top_p * (1.0 + dp)))[0]
        n_p = int(out[0]) if out.size else V
    if min_p > 0.0:
        out = np.nonzero(~(p >= min_p * (1.0 - dp) * p[0]))[0]
        n_m = max(int(out[0]) if out.size else V, min_keep)
    return max(1, min(n_k, n_p, n_m, V)), order, p, d


def cdf(d, n, temp):
    c = np.cumsum(np.exp(d[:n] / temp))
    return c / c[-1]


def pick(l, temp, u, **kw):
    """The rule's pick for one row and one uniform."""
    n, order, p, d = kept(l, **kw)
    c = cdf(d, n, temp)
    j = int(np.searchsorted(c, float(u), side="left"))
    return int(order[min(j, n - 1)])


def admissible(l, temp, u, d_rel, **kw):
    """Every code the rule gives when the cut thresholds and the target each move by +-d_rel (relative)."""
    n_lo, order, p, d = kept(l, dp=-d_rel, **kw)
    n_hi = kept(l, dp=+d_rel, **kw)[0]
    ok = set()
    for n in range(min(n_lo, n_hi), max(n_lo, n_hi) + 1):
        c = cdf(d, n, temp)
        j0 = min(int(np.searchsorted(c, float(u) * (1.0 - d_rel), side="left")), n - 1)
        j1 = min(int(np.searchsorted(c, float(u) * (1.0 + d_rel), side="left")), n - 1)
        ok.update(int(order[j]) for j in range(j0, j1 + 1))
    return ok
