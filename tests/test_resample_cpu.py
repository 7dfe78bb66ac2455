"""The arithmetic of the polyphase resampler (mlx-audio_amd/resample.py) on the CPU: the tap design against scipy's firwin, the
float64 reference of tests/_resample_ref.py against scipy's resample_poly, `ready` / `out_len`, and a numpy model of the streaming rule --
emit only ready outputs, flush at the end, zeros multiplied like samples -- that reproduces the whole-clip result exactly."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _resample_ref as R  # noqa: E402

from scipy import signal  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402


@pytest.mark.parametrize("src,dst", R.PAIRS)
def test_design_equals_firwin(src, dst):
    L, M = RS.ratio(src, dst)
    assert (L, M) == R.ratio(src, dst)
    half = 10 * max(L, M)
    want = signal.firwin(2 * half + 1, 1.0 / max(L, M), window=("kaiser", 5.0)) * L
    h = RS.design(L, M)
    assert h.dtype == np.float64 and h.shape == want.shape
    assert np.abs(h - want).max() <= 1e-12
    assert np.abs(R.taps(L, M) - want).max() <= 1e-12
    T = RS.taps_per_output(L, M)
    assert 21 <= T <= 61 and 2 * half + 1 <= 3201
    tab = RS.phase_table(L, M)  # phase-major, zero-padded, fp32
    assert tab.shape == (L, T) and tab.dtype == np.float32
    flat = tab.T.reshape(-1)
    np.testing.assert_array_equal(flat[: 2 * half + 1], h.astype(np.float32))
    assert not flat[2 * half + 1 :].any()


@pytest.mark.parametrize("src,dst", R.PAIRS)
def test_reference_equals_resample_poly(src, dst):
    L, M = R.ratio(src, dst)
    g = np.random.default_rng(src + dst)
    for N in ([997] if max(L, M) < 10 else []) + [4001]:
        x = g.standard_normal(N)
        want = signal.resample_poly(x, L, M)
        got = R.resample(x, L, M)
        assert got.shape == want.shape == (RS.out_len(N, L, M),)
        assert np.abs(got - want).max() <= 1e-12


def test_ratio_refusals_and_equal_rates():
    assert RS.ratio(24000, 24000) == (1, 1) and RS.ratio(11025, 24000) == (320, 147) and RS.ratio(24000, 8000) == (1, 3)
    for bad in ((24000, 24001), (0, 24000), (24000, -1), (44100.5, 24000), (7, 24000)):
        with pytest.raises(ValueError):
            RS.ratio(*bad)
    with pytest.raises(ValueError):
        RS.design(321, 1)
    assert RS.phase_table(320, 147).size <= 6720 and RS.phase_table(1, 320).shape == (1, 6401)


@pytest.mark.parametrize("L,M", [(3, 1), (1, 3), (80, 147), (147, 80), (3, 2), (2, 3), (1, 2), (320, 147)])
def test_ready_is_monotone_and_never_exceeds_out_len(L, M):
    half = 10 * max(L, M)
    prev = 0
    for n in range(0, 700):
        r, o = RS.ready(n, L, M), RS.out_len(n, L, M)
        assert (r, o) == (R.ready(n, L, M), R.out_len(n, L, M))
        assert prev <= r <= o
        if r:  # the last ready output reads no input at or behind n; the next one does
            assert ((r - 1) * M + half) // L <= n - 1 and (r * M + half) // L >= n
        prev = r
    assert RS.ready(0, L, M) == 0 and RS.out_len(0, L, M) == 0


def _chain(h32, x32, L, M, T, half, n):
    """Output n as the kernel computes it: one fp32 fma chain from 0 over the phase's T taps in ascending input order, zeros outside the
    clip multiplied like samples.  (float64 holds an fp32 product exactly, so rounding the sum to fp32 is the fused multiply-add, but for
    double rounding, which cannot differ between two runs over the same values.)"""
    c = n * M + half
    j0, p = c // L, c % L
    acc = np.float32(0)
    for i in range(T):
        t = T - 1 - i
        j = j0 - t
        k = p + t * L
        tap = h32[k] if k <= 2 * half else np.float32(0)
        v = x32[j] if 0 <= j < x32.shape[0] else np.float32(0)
        acc = np.float32(np.float64(tap) * np.float64(v) + np.float64(acc))
    return acc


@pytest.mark.parametrize("src,dst", [(8000, 24000), (44100, 24000), (24000, 16000)])
@pytest.mark.parametrize("slice_len", [1, 7, 160, 1000])
def test_streaming_model_reproduces_the_whole_clip(src, dst, slice_len):
    L, M = RS.ratio(src, dst)
    half, T = 10 * max(L, M), RS.taps_per_output(L, M)
    h32 = RS.design(L, M).astype(np.float32)
    N = {1: 131, 7: 311, 160: 523, 1000: 2203}[slice_len]
    x = np.random.default_rng(N + slice_len).standard_normal(N).astype(np.float32)
    whole = np.array([_chain(h32, x, L, M, T, half, n) for n in range(RS.out_len(N, L, M))], np.float32)
    assert np.abs(whole - R.resample(x, L, M)).max() <= (T + 2) * 2.0 ** -24 * np.abs(h32).sum() * np.abs(x).max()
    fed, emitted, got = 0, 0, []
    hist = np.zeros(T, np.float32)  # the carried state: the last T inputs (zeros in front of the clip)
    while fed < N:
        new = x[fed : fed + slice_len]
        cat = np.concatenate([hist, new])  # element r is input fed - T + r
        upto = RS.ready(fed + new.shape[0], L, M)
        for n in range(emitted, upto):
            j0 = (n * M + half) // L
            assert fed <= j0 < fed + new.shape[0]  # its last input is new (else it was ready a step earlier), its first is in the history
            window = cat[j0 - T + 1 - (fed - T) : j0 + 1 - (fed - T)]
            assert window.shape[0] == T
            got.append(_window_chain(h32, window, L, M, T, half, n))
        emitted, fed = upto, fed + new.shape[0]
        hist = cat[-T:]
    cat = np.concatenate([hist, np.zeros(T + M, np.float32)])  # the flush: zeros behind the clip
    for n in range(emitted, RS.out_len(N, L, M)):
        j0 = (n * M + half) // L
        got.append(_window_chain(h32, cat[j0 - T + 1 - (fed - T) : j0 + 1 - (fed - T)], L, M, T, half, n))
    got = np.array(got, np.float32)
    assert got.shape == whole.shape
    np.testing.assert_array_equal(got.view(np.uint32), whole.view(np.uint32))


def _window_chain(h32, window, L, M, T, half, n):
    """`_chain` on the T inputs a streaming step holds for output n (history, new samples, flush zeros) instead of the clip."""
    p = (n * M + half) % L
    acc = np.float32(0)
    for i in range(T):
        k = p + (T - 1 - i) * L
        tap = h32[k] if k <= 2 * half else np.float32(0)
        acc = np.float32(np.float64(tap) * np.float64(window[i]) + np.float64(acc))
    return acc
