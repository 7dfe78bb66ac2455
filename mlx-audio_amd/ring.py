"""Row-table ring copies (kk_ring.hip): what a continuous listener's samples take into and out of its ring -- every row in one
launch, the table a launch argument.  No CPU or PyTorch fallback: without the library both raise."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

MAX_ROWS = 64


def _args(t, name):
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.ndim == 2 and t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])):
        raise ValueError(f"{name} must be a float32 device tensor [rows, W] with contiguous rows")
    return C.c_void_p(t.data_ptr()), int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _table(v, rows, dtype, name):
    a = np.ascontiguousarray(np.asarray(v, dtype))
    if a.shape != (rows,):
        raise ValueError(f"{name} must hold {rows} entries")
    return a


def _stream(device):
    import torch

    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def write_rows(src, ring, ring_len: int, pos: Sequence[int], n: Sequence[int]) -> None:
    """ring[b, (pos[b] + i) % ring_len] = src[b, i] for i < n[b]; a row with n = 0 sits out.  src [rows, W], ring [rows, >= ring_len] on the
    device; pos (64-bit) and n on the host.  One launch, no sync."""
    import torch

    from ._lib import check, load

    rows = int(ring.shape[0])
    if src.shape[0] != rows:
        raise ValueError("src and ring must have the same rows")
    (sp, lds), (rp, ldr) = _args(src, "src"), _args(ring, "ring")
    p, k = _table(pos, rows, np.int64, "pos"), _table(n, rows, np.int32, "n")
    with torch.cuda.device(ring.device):
        check(load().kk_ring_write_rows(_stream(ring.device), rows, sp, lds, rp, ldr, int(ring_len), p.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)),
              "kk_ring_write_rows")


def read_rows(ring, ring_len: int, dst, pos: Sequence[int], n: Sequence[int], n_total: Optional[Sequence[int]] = None) -> None:
    """dst[b, i] = ring[b, (pos[b] + i) % ring_len] for i < n[b], and 0.0 for n[b] <= i < n_total[b] (n_total None: n); a row with
    n_total = 0 is not touched.  One launch, no sync."""
    import torch

    from ._lib import check, load

    rows = int(ring.shape[0])
    if dst.shape[0] != rows:
        raise ValueError("dst and ring must have the same rows")
    (rp, ldr), (dp, ldd) = _args(ring, "ring"), _args(dst, "dst")
    p, k = _table(pos, rows, np.int64, "pos"), _table(n, rows, np.int32, "n")
    t = k if n_total is None else _table(n_total, rows, np.int32, "n_total")
    with torch.cuda.device(ring.device):
        check(load().kk_ring_read_rows(_stream(ring.device), rows, rp, ldr, int(ring_len), dp, ldd, p.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p),
                                       t.ctypes.data_as(C.c_void_p)), "kk_ring_read_rows")
