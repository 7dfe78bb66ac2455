"""The polyphase resampler on the device (kk_resample.hip through mlx-audio_amd/resample.py) against the float64 reference of
tests/_resample_ref.py: whole clips on the nine rate pairs within a derived bound, and the row-mode object -- rows with different ratios that
start at different steps, sit out steps and take slices of 1, 7, 160 and 1 000 samples beside NaN entries -- bit-equal to the whole clip."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _resample_ref as R  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402
from mlx_audio_amd._lib import KokoroHipError, load  # noqa: E402

pytestmark = pytest.mark.gpu

SLICES = [1, 7, 160, 1000]


def _clip(seed, n):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _bound(L, M, x):
    """|err| <= (T + 2) 2^-24 S max|x|, S = the largest per-phase sum of |h|: the taps' rounding to fp32 (one part) and an fmaf chain of T
    terms whose partial sums stay below S max|x| (T parts), one part to spare for the second-order terms.  Derived, not measured."""
    h = RS.design(L, M)
    S = max(np.abs(h[p::L]).sum() for p in range(L))
    return (RS.taps_per_output(L, M) + 2) * 2.0 ** -24 * S * float(np.abs(x).max())


def _check_clip(src, dst, x):
    L, M = RS.ratio(src, dst)
    y = RS.resample(torch.from_numpy(x), src, dst).cpu().numpy()
    want = R.resample(x, L, M)
    assert y.dtype == np.float32 and y.shape == want.shape == (R.out_len(x.shape[0], L, M),)
    err, bound = float(np.abs(y - want).max()), _bound(L, M, x)
    print(f"resample {src} -> {dst}: N = {x.shape[0]}, max|err| = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound
    return y


def _lengths_for(L, M, outs):
    """The smallest N with out_len(N) >= each of `outs`: exactly that many outputs where L <= M, the next multiple the ratio reaches else."""
    return sorted({next(n for n in range(1, outs[-1] * M + 2) if R.out_len(n, L, M) >= o) for o in outs})


# ---- (a) whole clips, the nine pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", R.PAIRS)
def test_whole_clip_against_the_float64_reference(src, dst):
    _check_clip(src, dst, _clip(src + dst, 4001))


# ---- (b) rows with their own ratio, start and slicing -------------------------------------------------------------------------------------
def test_rows_are_bit_equal_to_the_whole_clip_whatever_the_slicing_and_the_neighbours():
    rates = [(8000, 24000), (44100, 24000), (48000, 24000)]  # 3 / 1, 80 / 147, 1 / 2
    assert [RS.ratio(*r) for r in rates] == [(3, 1), (80, 147), (1, 2)]
    clips = [_clip(10 + r, n) for r, n in enumerate((2400, 3100, 2777))]
    whole = [RS.resample(torch.from_numpy(c), *rates[r]).cpu().numpy() for r, c in enumerate(clips)]
    rows, start = 4, [0, 2, 5]  # row 3 is never set: its entries are NaN throughout
    rs = RS.RowResampler(rows, 1000)
    fed, emitted, got = [0] * 3, [0] * 3, [[] for _ in range(3)]
    flushed, started = [False] * 3, [False] * 3
    step = 0
    while not all(flushed):
        x = np.full((rows, 1000), np.nan, np.float32)
        n_in, flush, want = [0] * rows, [False] * rows, [0] * rows
        for r in range(3):
            if step < start[r] or flushed[r] or (step + r) % 3 == 0:  # not started yet, done, or sitting this step out
                continue
            if not started[r]:
                rs.set_row(r, *rates[r])
                started[r] = True
            k = min(SLICES[(step + r) % 4], clips[r].shape[0] - fed[r])
            x[r, :k] = clips[r][fed[r] : fed[r] + k]
            n_in[r], fed[r] = k, fed[r] + k
            flush[r] = flushed[r] = fed[r] == clips[r].shape[0]
            L, M = RS.ratio(*rates[r])
            want[r] = (R.out_len(fed[r], L, M) if flush[r] else R.ready(fed[r], L, M)) - emitted[r]
            emitted[r] += want[r]
        y, n_out = rs.step(torch.from_numpy(x), n_in, flush)
        assert n_out == want  # host integer arithmetic, no sync
        for r in range(3):
            got[r].append(y[r, : n_out[r]].cpu().numpy())
        step += 1
    assert step > 12
    for r in range(3):
        out = np.concatenate(got[r])
        assert out.shape == whole[r].shape
        np.testing.assert_array_equal(out.view(np.uint32), whole[r].view(np.uint32))
    rs.close()


# ---- (c) edge lengths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(8000, 24000), (44100, 24000), (48000, 24000), (24000, 44100)])
def test_edge_lengths(src, dst):
    L, M = RS.ratio(src, dst)
    B = int(load().kk_resampler_block_outputs())
    assert B >= 2 * L or (L, M) != (80, 147)
    lengths = [1, 5] + _lengths_for(L, M, [B - 1, B, B + 1])
    outs = [R.out_len(n, L, M) for n in lengths[2:]]
    if L <= M:
        assert outs == [B - 1, B, B + 1]
    else:
        # Upsampling reaches only some counts (3 / 1: multiples of 3 -> 255 and 258; 147 / 80 -> 256 and 258).  What these cases exercise is a
        # last workgroup that is partly filled: a count at or below B and one that spills into a second workgroup.  The exact B - 1, B, B + 1
        # boundary is covered by the 80 / 147 and 1 / 2 cases.
        assert min(outs) <= B < max(outs) <= B + L
    assert 5 < R.half_len(L, M) / L
    rs = RS.RowResampler(1, max(lengths))
    for N in lengths:
        x = _clip(N, N)
        y = _check_clip(src, dst, x)
        # the same clip through the row object: one sample first, the rest with the flush
        rs.set_row(0, src, dst)
        parts = []
        for lo, hi in ((0, 1), (1, N)):
            buf = torch.from_numpy(x[lo:hi][None]) if hi > lo else torch.zeros((1, 4))
            out, n = rs.step(buf, [hi - lo], [hi == N])
            parts.append(out[0, : n[0]].cpu().numpy())
            if hi == N:
                break
        np.testing.assert_array_equal(np.concatenate(parts).view(np.uint32), y.view(np.uint32))
    rs.close()


@pytest.mark.parametrize("src,dst,N", [(24000, 75, 257 * 320 - 17), (11025, 24000, 300), (24000, 11025, 1500)])
def test_the_widest_ratios(src, dst, N):
    """1 / 320: 6 401 taps per output and a window of many LDS passes; 320 / 147 and 147 / 320: the largest tap table."""
    x = _clip(N, N)
    y = _check_clip(src, dst, x)
    rs = RS.RowResampler(2, 40000)
    rs.set_row(1, src, dst)
    got, fed = [], 0
    for k in (40000, 7, 40000, 40000):
        k = min(k, N - fed)
        buf = torch.full((2, max(4, k)), float("nan"))
        buf[1, :k] = torch.from_numpy(x[fed : fed + k])
        fed += k
        out, n = rs.step(buf, [0, k], [False, fed == N])
        got.append(out[1, : n[1]].cpu().numpy())
        if fed == N:
            break
    np.testing.assert_array_equal(np.concatenate(got).view(np.uint32), y.view(np.uint32))
    rs.close()


# ---- (d) a row reused with another ratio ---------------------------------------------------------------------------------------------------
def test_a_row_reused_with_another_ratio():
    rs = RS.RowResampler(2, 512)
    a, b = _clip(1, 700), _clip(2, 900)
    rs.set_row(0, 16000, 24000)
    rs.step(torch.from_numpy(np.stack([a[:512], a[:512]])), [512, 0], [False, False])  # row 0 holds a stream's history and counts
    rs.set_row(0, 24000, 48000)  # ... and starts over at another ratio without a flush
    got = []
    for lo in (0, 512):
        k = min(512, 900 - lo)
        buf = np.zeros((2, 512), np.float32)
        buf[0, :k] = b[lo : lo + k]
        out, n = rs.step(torch.from_numpy(buf), [k, 0], [lo + k == 900, False])
        got.append(out[0, : n[0]].cpu().numpy())
    want = RS.resample(torch.from_numpy(b), 24000, 48000).cpu().numpy()
    np.testing.assert_array_equal(np.concatenate(got).view(np.uint32), want.view(np.uint32))
    rs.close()


# ---- (e) refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    rs = RS.RowResampler(2, 64)
    clip = _clip(3, 150)
    want = RS.resample(torch.from_numpy(clip), 8000, 24000).cpu().numpy()
    rs.set_row(0, 8000, 24000)
    x = torch.zeros((2, 128))
    x[0, :64] = torch.from_numpy(clip[:64])
    y, n = rs.step(x, [64, 0], [False, False])
    got = [y[0, : n[0]].cpu().numpy()]
    with pytest.raises(KokoroHipError, match="outside"):
        rs.set_row(2, 8000, 24000)
    with pytest.raises(KokoroHipError, match="outside"):
        rs.set_row(-1, 8000, 24000)
    with pytest.raises(ValueError, match="320"):
        rs.set_row(1, 24000, 24001)
    with pytest.raises(KokoroHipError, match="created for 64"):
        rs.step(x, [65, 0], [False, False])
    with pytest.raises(KokoroHipError, match="no ratio"):
        rs.step(x, [8, 8], [False, False])  # row 1 was never set: row 0 must not advance either
    x[0, :64] = torch.from_numpy(clip[64:128])
    y, n = rs.step(x, [64, 0], [False, False])
    got.append(y[0, : n[0]].cpu().numpy())
    x[0, :22] = torch.from_numpy(clip[128:])
    y, n = rs.step(x, [22, 0], [True, False])
    got.append(y[0, : n[0]].cpu().numpy())
    with pytest.raises(KokoroHipError, match="flushed"):
        rs.step(x, [1, 0], [False, False])
    with pytest.raises(KokoroHipError, match="flushed"):
        rs.step(x, [0, 0], [True, False])
    np.testing.assert_array_equal(np.concatenate(got).view(np.uint32), want.view(np.uint32))  # the refused calls changed nothing
    with pytest.raises(KokoroHipError, match="max_rows"):
        RS.RowResampler(65, 64)
    with pytest.raises(ValueError):
        RS.resample(torch.zeros(0), 8000, 24000)
    rs.close()
    with pytest.raises(KokoroHipError, match="closed"):
        rs.step(x, [1, 0], [False, False])
