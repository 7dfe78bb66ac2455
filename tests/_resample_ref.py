"""The float64 reference of the polyphase resampler, written from its defining sum alone; it imports nothing of the package.

    g = gcd(src, dst), L = dst / g, M = src / g, half = 10 max(L, M)
    h = firwin(2 half + 1, 1 / max(L, M), window=("kaiser", 5.0)) L
    y[n] = sum_j h[n M + half - j L] x[j]      x = 0 outside [0, N), 0 <= n < ceil(N L / M)
"""
import math

import numpy as np

TO_24K = [8000, 16000, 22050, 44100, 48000]
FROM_24K = [8000, 16000, 44100, 48000]
PAIRS = [(r, 24000) for r in TO_24K] + [(24000, r) for r in FROM_24K]  # the nine pairs


def ratio(src, dst):
    g = math.gcd(src, dst)
    return dst // g, src // g


def half_len(L, M):
    return 10 * max(L, M)


def out_len(n, L, M):
    return (n * L + M - 1) // M


def ready(n, L, M):
    return max(0, (n * L - 1 - half_len(L, M)) // M + 1)


def taps(L, M):
    """firwin by hand in float64: the ideal low-pass at 1 / max(L, M) of Nyquist, a Kaiser window (beta 5), unity gain at DC, times L."""
    half = half_len(L, M)
    c = 1.0 / max(L, M)
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = c * np.sinc(c * m) * np.kaiser(2 * half + 1, 5.0)
    return h / np.sum(h) * L


def outputs(x, L, M, first, last, h=None):
    """y[first .. last) of the clip x (float64), each output the defining sum over every tap that meets a sample."""
    x = np.asarray(x, np.float64)
    h = taps(L, M) if h is None else np.asarray(h, np.float64)
    half, N = half_len(L, M), x.shape[0]
    y = np.zeros(last - first, np.float64)
    for n in range(first, last):
        c = n * M + half                       # tap index k = c - j L must lie in [0, 2 half]
        j_lo = max(0, -((2 * half - c) // L))  # ceil((c - 2 half) / L)
        j_hi = min(N - 1, c // L)
        if j_hi >= j_lo:
            j = np.arange(j_lo, j_hi + 1)
            y[n - first] = np.dot(h[c - j * L], x[j])
    return y


def resample(x, L, M, h=None):
    return outputs(x, L, M, 0, out_len(len(x), L, M), h)
