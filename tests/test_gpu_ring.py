"""The row-table ring copies on the device (kk_ring.hip, mlx-audio_amd/ring.py) against numpy modulo indexing: a copy is a
copy, so every comparison is bit equality (the samples carry NaN payloads and both zeros)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mlx_audio_amd import ring  # noqa: E402
from mlx_audio_amd._lib import KokoroHipError  # noqa: E402

pytestmark = pytest.mark.gpu

RING = 1031  # not a multiple of 4: a wrap changes the alignment
COUNTS = [0, 1, 3, 4, 5, 255, 256, 257, RING]
# aligned and not, wrapping (for the longer counts) and not, and beyond 2^31 and 2^40
POSITIONS = [0, 4, 5, 1028, 1030, RING * 7 + 12, (1 << 31) + 8, (1 << 31) + 1029, (1 << 40) + 3, RING * (1 << 33)]


def _bits(g, shape):
    """float32 patterns of every kind: a copy must keep NaN payloads, infinities, denormals and the sign of zero"""
    return g.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _cases():
    out = [(p, c) for p in POSITIONS for c in COUNTS]
    return [out[i : i + 9] for i in range(0, len(out), 9)]  # 9 rows per launch: every launch mixes counts


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned tensors", "tensors one float off"])
def test_write_and_read_against_numpy_modulo_indexing(misaligned):
    g = np.random.default_rng(12)
    dev = torch.device("cuda")
    W, rows, o = 1040, 9, int(misaligned)
    for batch in _cases():
        pos, n = [p for p, _ in batch], [c for _, c in batch]
        src = _bits(g, (rows, W + o))
        before = _bits(g, (rows, W + o))
        d_src, d_ring = torch.from_numpy(src).to(dev)[:, o:], torch.from_numpy(before).to(dev)[:, o:]
        ring.write_rows(d_src, d_ring, RING, pos, n)
        want = before[:, o:].copy()
        for b in range(rows):
            want[b, (pos[b] + np.arange(n[b])) % RING] = src[b, o : o + n[b]]
        got = d_ring.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))  # (and nothing behind ring_len, nothing of an n = 0 row)
        # read it back, zero-filled behind n: n_total = n + 0, 1, 3, 4, 5 ..., and a row that sits out
        tot = [min(W, c + [0, 1, 3, 4, 5, 8, 9][b % 7]) for b, c in enumerate(n)]
        tot[4] = n[4] = 0
        dst0 = _bits(g, (rows, W + o))
        d_dst = torch.from_numpy(dst0).to(dev)[:, o:]
        ring.read_rows(d_ring, RING, d_dst, pos, n, tot)
        want_d = dst0[:, o:].copy()
        for b in range(rows):
            want_d[b, : n[b]] = want[b, (pos[b] + np.arange(n[b])) % RING]
            want_d[b, n[b] : tot[b]] = 0.0
        np.testing.assert_array_equal(d_dst.cpu().numpy().view(np.uint32), want_d.view(np.uint32))


def test_long_rows_stride_over_the_workgroups():
    g = np.random.default_rng(13)
    dev = torch.device("cuda")
    L = 64 * 1024 * 2 + 1028  # more than 64 workgroups of 1024 samples
    src = _bits(g, (2, L))
    d_ring = torch.zeros((2, L), dtype=torch.float32, device=dev)
    ring.write_rows(torch.from_numpy(src).to(dev), d_ring, L, [(1 << 35) * L + 8, 3], [L - 8, L])
    want = np.zeros((2, L), np.float32)
    want[0, 8:] = src[0, : L - 8]
    want[1, (3 + np.arange(L)) % L] = src[1]
    np.testing.assert_array_equal(d_ring.cpu().numpy().view(np.uint32), want.view(np.uint32))
    d_dst = torch.full((2, L), 7.0, dtype=torch.float32, device=dev)
    ring.read_rows(d_ring, L, d_dst, [8, 3], [L - 8, L - 1], [L, L - 1])
    back = d_dst.cpu().numpy()
    np.testing.assert_array_equal(back[0, : L - 8].view(np.uint32), src[0, : L - 8].view(np.uint32))
    assert not back[0, L - 8 :].any() and back[1, L - 1] == 7.0
    np.testing.assert_array_equal(back[1, : L - 1].view(np.uint32), src[1, : L - 1].view(np.uint32))


def test_refusals_change_nothing():
    dev = torch.device("cuda")
    a = torch.arange(2 * 64, dtype=torch.float32, device=dev).reshape(2, 64)
    r = torch.full((2, 48), -1.0, dtype=torch.float32, device=dev)
    keep_a, keep_r = a.clone(), r.clone()
    for kw, msg in [
        (dict(ring_len=49, pos=[0, 0], n=[1, 1]), "a ring of 49 in a row of 48"),
        (dict(ring_len=0, pos=[0, 0], n=[1, 1]), "a ring of 0"),
        (dict(ring_len=40, pos=[0, 0], n=[41, 1]), "above ring_len"),
        (dict(ring_len=40, pos=[0, -1], n=[1, 1]), "negative position"),
        (dict(ring_len=40, pos=[0, 0], n=[1, -1]), "negative count"),
    ]:
        with pytest.raises(KokoroHipError, match=msg):
            ring.write_rows(a, r, kw["ring_len"], kw["pos"], kw["n"])
        with pytest.raises(KokoroHipError, match=msg):
            ring.read_rows(r, kw["ring_len"], a, kw["pos"], kw["n"])
    with pytest.raises(KokoroHipError, match="in a row of 32"):
        ring.write_rows(a[:, :32].contiguous(), r, 48, [0, 0], [33, 1])
    with pytest.raises(KokoroHipError, match="in a row of 32"):
        ring.read_rows(r, 48, a[:, :32].contiguous(), [0, 0], [8, 1], [33, 1])
    with pytest.raises(KokoroHipError, match="above n_total"):
        ring.read_rows(r, 48, a, [0, 0], [8, 1], [7, 1])
    with pytest.raises(KokoroHipError, match="rows 65"):
        ring.write_rows(torch.zeros((65, 8), device=dev), torch.zeros((65, 8), device=dev), 8, [0] * 65, [1] * 65)
    with pytest.raises(ValueError):
        ring.write_rows(a, r, 48, [0], [1])
    with pytest.raises(ValueError):
        ring.write_rows(a.double(), r, 48, [0, 0], [1, 1])
    torch.cuda.synchronize()
    assert torch.equal(a, keep_a) and torch.equal(r, keep_r)
