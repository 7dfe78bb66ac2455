"""The kernels of Whisper's token timestamps on their own (csrc/kk_whisper_align.hip), each driven through its raw entry: `dtw` exactly equal
to the numpy restatement of timing.py:47-95 (tests/_whisper_align_ref.py, itself pinned against transformers), `align_matrix` against the float64
restatement of timing.py:147-155, `qk_rows` against float64 from the same bf16 keys, the stand-alone median filter exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_align_ref as A  # noqa: E402

from mlx_audio_amd import _lib  # noqa: E402
from mlx_audio_amd import whisper_timing as WT  # noqa: E402

# align_matrix: max |device - float64| / rms(float64).  Measured on an MI355X over the 144 cases of test_align_matrix_against_float64: between
# 4.1e-07 and 2.341e-06 (the largest at frames 73, width 9); the bound is 4 x the largest value seen, which leaves room for other seeds.
ALIGN_BOUND = 4 * 2.341e-06


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- dtw ----------------------------------------------------------------------------------------------------------------------------------------
def _dtw_inputs(n, m, seed):
    g = np.random.default_rng(seed)
    rnd = g.standard_normal((n, m)).astype(np.float32)
    inf = g.standard_normal((n, m)).astype(np.float32)
    inf[g.random((n, m)) < 0.15] = np.inf
    nan = g.standard_normal((n, m)).astype(np.float32)
    nan[g.random((n, m)) < 0.1] = np.nan
    return {"random": rnd, "zero": np.zeros((n, m), np.float32), "integers": g.integers(-2, 3, (n, m)).astype(np.float32), "inf": inf, "nan": nan}


def _check_dtw(got, x, n, m, what):
    ti, tj, ln, first = got
    ri, rj = A.dtw(x)
    L = int(ln)
    assert L == len(ri), (what, L, len(ri))
    assert np.array_equal(ti[:L], ri) and np.array_equal(tj[:L], rj), what
    assert np.array_equal(first[:n], A.first_cols(ri, rj, n)), what
    assert L <= n + m


@pytest.mark.parametrize("m", [1, 7, 64, 100])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_dtw_equals_the_restatement_exactly(n, m):
    """the five kinds of input as one batch of five items of the same shape"""
    xs = _dtw_inputs(n, m, 1000 * n + m)
    ti, tj, ln, first = (t.cpu().numpy() for t in WT.dtw_rows(_dev(np.stack(list(xs.values()))), [n] * 5, [m] * 5))
    for b, (kind, x) in enumerate(xs.items()):
        _check_dtw((ti[b], tj[b], ln[b], first[b]), x, n, m, (kind, n, m))


def test_dtw_over_three_bands_and_1500_columns():
    xs = _dtw_inputs(130, 1500, 7)
    ti, tj, ln, first = (t.cpu().numpy() for t in WT.dtw_rows(_dev(np.stack(list(xs.values()))), [130] * 5, [1500] * 5))
    for b, (kind, x) in enumerate(xs.items()):
        _check_dtw((ti[b], tj[b], ln[b], first[b]), x, 130, 1500, kind)
    path = WT.dtw(_dev(xs["random"]))  # the (2, L) array of the reference's dtw
    ri, rj = A.dtw(xs["random"])
    assert path.shape == (2, len(ri)) and np.array_equal(path[0], ri) and np.array_equal(path[1], rj)
    neg = WT.dtw_rows(_dev(xs["random"][None]), [130], [1500], negate=True)  # what find_alignment asks for: the path of -x
    ni, nj = A.dtw(-xs["random"])
    assert np.array_equal(neg[0][0, : len(ni)].cpu().numpy(), ni) and np.array_equal(neg[1][0, : len(nj)].cpu().numpy(), nj)


@pytest.mark.parametrize("kind", ["random", "integers", "nan"])
def test_dtw_ragged_batch_is_bit_equal_to_each_item_alone(kind):
    """NaN fills the memory behind every item's rows and columns: it is never read"""
    shapes = [(65, 100), (2, 7), (130, 64)]
    buf = np.full((3, 130, 104), np.nan, np.float32)
    items = []
    for b, (n, m) in enumerate(shapes):
        x = _dtw_inputs(n, m, 50 + b)[kind]
        buf[b, :n, :m] = x
        items.append(x)
    ti, tj, ln, first = (t.cpu().numpy() for t in WT.dtw_rows(_dev(buf), [s[0] for s in shapes], [s[1] for s in shapes]))
    for b, (n, m) in enumerate(shapes):
        _check_dtw((ti[b], tj[b], ln[b], first[b]), items[b], n, m, (kind, b))
        ai, aj, al, af = (t.cpu().numpy() for t in WT.dtw_rows(_dev(items[b][None]), [n], [m]))
        L = int(al[0])
        assert L == int(ln[b]) and np.array_equal(ai[0, :L], ti[b, :L]) and np.array_equal(aj[0, :L], tj[b, :L]) and np.array_equal(af[0, :n], first[b, :n])


def test_dtw_refuses_counts_outside_the_buffer():
    x = _dev(np.zeros((2, 4, 8), np.float32))
    for rows, cols, word in (([4, 5], [8, 8], r"n_rows\[1\] = 5"), ([4, 0], [8, 8], r"n_rows\[1\] = 0"), ([4, 4], [9, 8], r"n_cols\[0\] = 9"),
                             ([4, 4], [8, 0], r"n_cols\[1\] = 0")):
        with pytest.raises(_lib.KokoroHipError, match=word):
            WT.dtw_rows(x, rows, cols)


# ---- align_matrix -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 7, 9])
@pytest.mark.parametrize("frames", [3, 4, 73, 750])
def test_align_matrix_against_float64(frames, width):
    """heads {1, 2, 7} x rows {5, 37} x qk_scale {1.0, 0.5}, each as an item of its own and the two row counts as one ragged batch.  frames 3 with
    width 7 or 9 takes the skip rule (3 <= width // 2), frames 4 is the smallest filtered case of width 7.  Both sides see the same fp32 scores, so
    the error is fp32 arithmetic amplified by 1 / std."""
    g = np.random.default_rng(100 * frames + width)
    worst = 0.0
    for heads in (1, 2, 7):
        ld = frames + 5
        qk = np.full((2, heads, 37, ld), np.nan, np.float32)  # NaN behind every item's rows and frames
        qk[0, :, :5, :frames] = 2.0 * g.standard_normal((heads, 5, frames))
        qk[1, :, :, :frames] = 2.0 * g.standard_normal((heads, 37, frames))
        for scale in (1.0, 0.5):
            got = WT.align_matrix_rows(_dev(qk), [5, 37], [frames, frames], width, scale).cpu().numpy()
            for b, rows in enumerate((5, 37)):
                ref = A.align_matrix(qk[b, :, :rows, :frames], scale, width)
                err = np.abs(got[b, :rows, :frames] - ref).max() / A.rms(ref)
                print(f"align_matrix frames {frames} width {width} heads {heads} rows {rows} scale {scale}: max|diff| / rms {err:.3e} (rms {A.rms(ref):.3f})")
                worst = max(worst, err)
                alone = WT.align_matrix_rows(_dev(qk[b:b + 1, :, :rows]), [rows], [frames], width, scale).cpu().numpy()
                assert np.array_equal(alone[0, :, :frames], got[b, :rows, :frames])  # an item alone gives the bits it has in the batch
            assert (got[0, 5:] == 0).all() and (got[:, :, frames:] == 0).all()  # nothing is written behind an item
    print(f"align_matrix frames {frames} width {width}: worst {worst:.3e}, bound {ALIGN_BOUND:.1e}")
    assert worst <= ALIGN_BOUND


def test_align_matrix_frames_differ_per_item_and_the_skip_rule():
    g = np.random.default_rng(5)
    qk = (2.0 * g.standard_normal((3, 2, 9, 80))).astype(np.float32)
    frames = [3, 80, 41]
    got = WT.align_matrix_rows(_dev(qk), [9, 4, 7], frames, 7).cpu().numpy()
    for b, (rows, f) in enumerate(zip([9, 4, 7], frames)):
        ref = A.align_matrix(qk[b, :, :rows, :f], 1.0, 7)
        err = np.abs(got[b, :rows, :f] - ref).max() / A.rms(ref)
        print(f"align_matrix ragged item {b} rows {rows} frames {f}: max|diff| / rms {err:.3e}")
        assert err <= ALIGN_BOUND
    unfiltered = A.align_matrix(qk[0, :, :, :3], 1.0, 1)  # 3 <= 7 // 2: the filter is skipped
    assert np.abs(got[0, :, :3] - unfiltered).max() / A.rms(unfiltered) <= ALIGN_BOUND


@pytest.mark.parametrize("width", [7, 9])
def test_align_matrix_bits_do_not_depend_on_the_head_group(width):
    g = np.random.default_rng(6)
    qk = _dev((2.0 * g.standard_normal((2, 7, 11, 70))).astype(np.float32))
    base = WT.align_matrix_rows(qk, [11, 6], [70, 33], width, group=0).cpu().numpy()  # the default group holds all 7
    for group in (1, 2, 3, 7, 16):
        assert np.array_equal(WT.align_matrix_rows(qk, [11, 6], [70, 33], width, group=group).cpu().numpy(), base), group
    lib = _lib.load()
    assert lib.kk_op_whisper_align_matrix_workspace_bytes(2, 7, 11, 70, 2) == 2 * 2 * 11 * 70 * 4


@pytest.mark.parametrize("width", [1, 3, 7, 9, 31])
def test_the_stand_alone_median_filter_is_exact(width):
    g = np.random.default_rng(width)
    for n in (3, 4, 16, 17, 300):
        x = g.standard_normal((3, 5, n)).astype(np.float32)
        x[0] = g.integers(0, 3, (5, n))  # ties
        got = WT.median_filter(_dev(x), width).cpu().numpy()
        assert np.array_equal(got, A.median_filter(x, width)), (width, n)
    with pytest.raises(ValueError, match="odd"):
        WT.median_filter(_dev(x), 4)


# ---- qk_rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 63, 65, 750, 1500])
def test_qk_rows_against_float64(n_keys):
    """items 2, rows 11 (two chunks of 8, the second cut), 6 heads of which 3 are wanted in an order that is not sorted; the keys at and past n_keys are
    NaN in the store and the V half of every row is NaN.  Bound as DESIGN 8g bounds attention scores: (64 + 8) 2^-23 sum |q k| / 8."""
    import torch

    items, rows, heads, T_rows = 2, 11, 6, 1500
    D, sel = heads * 64, [4, 1, 5]
    g = np.random.default_rng(n_keys)
    q = g.standard_normal((items * rows, heads, 64)).astype(np.float32)
    k = torch.from_numpy(g.standard_normal((items, T_rows, 2 * D)).astype(np.float32)).bfloat16()
    k[:, n_keys:] = float("nan")
    k[:, :, D:] = float("nan")
    kd, qd = k.cuda(), _dev(q)
    ldo = n_keys + 3
    out = torch.full((len(sel), items * rows, ldo), -7.0, dtype=torch.float32, device="cuda")
    lib = _lib.load()
    assert lib.kk_op_whisper_qk_rows_workspace_bytes(items, rows, len(sel), n_keys) == 0
    _lib.check(lib.kk_op_whisper_qk_rows(None, items, rows, heads, C.c_void_p(qd.data_ptr()), C.c_void_p(kd.data_ptr()), T_rows, 2 * D,
                                         (C.c_int32 * len(sel))(*sel), len(sel), n_keys, C.c_void_p(out.data_ptr()), ldo), "kk_op_whisper_qk_rows")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :, n_keys:] == -7.0).all()  # nothing is written at or past n_keys
    kf = k[:, :n_keys, :D].float().numpy().astype(np.float64).reshape(items, n_keys, heads, 64)
    worst = 0.0
    for j, h in enumerate(sel):
        for it in range(items):
            qq = q[it * rows:(it + 1) * rows, h].astype(np.float64)  # (rows, 64)
            ref = qq @ kf[it, :, h].T / 8.0
            mag = np.abs(qq) @ np.abs(kf[it, :, h]).T / 8.0
            frac = np.abs(got[j, it * rows:(it + 1) * rows, :n_keys] - ref) / ((64 + 8) * 2.0 ** -23 * mag)
            worst = max(worst, float(frac.max()))
    print(f"qk_rows n_keys {n_keys}: worst error {worst:.4f} of the bound")
    assert worst <= 1.0
