"""Polyphase FIR resampling for the audio edges of CSM serving: `scipy.signal.resample_poly(x, L, M)` with its defaults, as
one kernel that serves whole clips and streams fed in arbitrary slices with the same bits.

For source rate `src` and destination rate `dst`: g = gcd, L = dst / g, M = src / g, half = 10 max(L, M),
    h = firwin(2 half + 1, 1 / max(L, M), window=("kaiser", 5.0)) L                          (`design`, float64, numpy only)
    y[n] = sum_j h[n M + half - j L] x[j],   x = 0 outside [0, N),   0 <= n < out_len(N) = ceil(N L / M)
While a stream is open and N samples have been fed, the outputs below ready(N) = max(0, (N L - 1 - half) // M + 1) are final; the rest follow
at the flush, with zeros behind the clip.  Every output is one fp32 fmaf chain over its phase's T = ceil((2 half + 1) / L) taps in ascending
input order, zeros multiplied like samples, so the bits of output n depend on n and the clip alone (kk_resample.hip).

`resample(x, src, dst)`: a whole clip on the device.  `RowResampler(max_rows, max_in)`: one object, one launch per step, a ratio, a position
and a lifetime per row -- the structure of `Mimi.row_decoder` / `Mimi.row_encoder`.  No CPU or PyTorch fallback: without the library both raise.

PCM formats (`pcm.py`): `set_row(..., in_format=, out_format=)` and `resample(..., in_format=, out_format=)` let a row read
and write "s16le", "mulaw" or "alaw" samples inside the same launch; its outputs are `encode(resample(decode(clip)))` bit for bit."""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import pcm as PCM
from ._lib import KokoroHipError, check, load

MAX_RATIO = 320  # max(L, M) the kernel takes: 11.025 kHz <-> 24 kHz is 147 / 320; at most 6 401 taps, 6 720 floats (26.9 KB) as the zero-padded [L][T] table


def ratio(src: int, dst: int) -> Tuple[int, int]:
    """(L, M) = (dst, src) / gcd.  ValueError for rates that are not positive integers or whose ratio the kernel does not take."""
    if int(src) != src or int(dst) != dst or int(src) < 1 or int(dst) < 1:
        raise ValueError(f"sample rates must be positive integers, got {src!r} -> {dst!r}")
    src, dst = int(src), int(dst)
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    if max(L, M) > MAX_RATIO:
        raise ValueError(f"resampling {src} -> {dst} Hz is {L} / {M}: the resampler takes max(L, M) <= {MAX_RATIO}")
    return L, M


def half_len(L: int, M: int) -> int:
    return 10 * max(int(L), int(M))


def taps_per_output(L: int, M: int) -> int:
    return -(-(2 * half_len(L, M) + 1) // int(L))


def design(L: int, M: int) -> np.ndarray:
    """The 2 half + 1 taps in float64: firwin(2 half + 1, 1 / max(L, M), window=("kaiser", 5.0)) * L -- the windowed sinc, scaled to unity
    gain at DC as firwin does, times L."""
    L, M = int(L), int(M)
    if L < 1 or M < 1 or max(L, M) > MAX_RATIO:
        raise ValueError(f"L = {L}, M = {M}: both must be in [1, {MAX_RATIO}]")
    half = half_len(L, M)
    cutoff = 1.0 / max(L, M)
    m = np.arange(2 * half + 1, dtype=np.float64) - half
    h = cutoff * np.sinc(cutoff * m) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * L


@functools.lru_cache(maxsize=64)
def phase_table(L: int, M: int) -> np.ndarray:
    """What the library takes: fp32 [L][T], table[p][t] = h[p + t L], zero where p + t L > 2 half.  Read-only (cached per ratio)."""
    h = design(L, M)
    T = taps_per_output(L, M)
    flat = np.zeros(L * T, np.float64)
    flat[: h.shape[0]] = h
    tab = np.ascontiguousarray(flat.reshape(T, L).T.astype(np.float32))
    tab.setflags(write=False)
    return tab


def out_len(n: int, L: int, M: int) -> int:
    return -(-int(n) * int(L) // int(M))


def ready(n: int, L: int, M: int) -> int:
    """Outputs that are final once n samples of an open stream have been fed: output k needs inputs up to (k M + half) // L."""
    return max(0, (int(n) * int(L) - 1 - half_len(L, M)) // int(M) + 1)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def resample(x, src: int, dst: int, device=None, in_format=None, out_format=None) -> torch.Tensor:
    """A whole mono clip [N] (N >= 1) from `src` to `dst` Hz on the device -> float32 [out_len(N)] (kk_op_resample; synchronises).  Equal
    rates return the clip as it is.  With a format (`pcm.FORMATS`) the clip holds samples stored as `in_format` and the result samples stored
    as `out_format`, each in the format's dtype: `pcm.encode(resample(pcm.decode(x)))`, bit for bit, in one launch (equal rates: `pcm.convert`)."""
    if PCM.check(in_format) != "f32" or PCM.check(out_format) != "f32":
        return _resample_fmt(x, src, dst, device, PCM.check(in_format), PCM.check(out_format))
    L, M = ratio(src, dst)
    x = torch.as_tensor(x)
    device = torch.device(device) if device is not None else (x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    x = x.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if x.shape[0] < 1:
        raise ValueError("resample: an empty clip")
    if L == M:
        return x
    if x.data_ptr() % 16:  # (a view that starts inside another tensor)
        x = x.clone()
    tab = phase_table(L, M)
    with torch.cuda.device(device):
        y = torch.empty(out_len(x.shape[0], L, M), dtype=torch.float32, device=device)
        check(load().kk_op_resample(_stream(device), C.c_void_p(x.data_ptr()), int(x.shape[0]), L, M, tab.ctypes.data_as(C.c_void_p), int(tab.shape[1]),
                                    C.c_void_p(y.data_ptr())), "kk_op_resample")
    return y


def _resample_fmt(x, src, dst, device, fi, fo) -> torch.Tensor:
    L, M = ratio(src, dst)
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.array(PCM.samples(x, fi)))
    if x.dtype != PCM.torch_dtype(fi):
        raise ValueError(f"{fi} samples are {PCM.torch_dtype(fi)}, got {x.dtype}")
    device = torch.device(device) if device is not None else (x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    x = x.to(device).reshape(-1)
    if x.shape[0] < 1:
        raise ValueError("resample: an empty clip")
    if L == M:
        return PCM.convert(x, fi, fo, device)
    rs = RowResampler(1, int(x.shape[0]), device=device)
    try:
        rs.set_row(0, src, dst, in_format=fi, out_format=fo)
        y, n = rs.step(x.reshape(1, -1), [int(x.shape[0])], [True])
        out = rs.out_view(y, 0)[: n[0]].clone()
        torch.cuda.current_stream(device).synchronize()
    finally:
        rs.close()
    return out


class RowResampler:
    """`max_rows` independent streams, each with its own ratio.  `set_row(row, src, dst)` starts a stream (zero history, zero counts);
    `step(x, n_in, flush)` is ONE launch for every row that takes part; a row's concatenated outputs are, bit for bit, `resample(clip)`
    whatever the slicing and whatever the other rows do.  All work goes to the current stream of `device`.
    A row set with `in_format` / `out_format` reads / writes samples stored in that format.  While any row of the object has a format other
    than "f32", `step` takes x as its BYTES (any dtype; row b's n_in[b] samples of its input format at the start of the row) and returns y as
    bytes [max_rows, W'] uint8: `out_view(y, b)[: n_out[b]]` is row b's outputs in its format's dtype, `in_view(x, b)` the same for a
    uint8 input buffer one fills.  With f32 rows only, `step` is what it was."""

    def __init__(self, max_rows: int, max_in: int, device=None):
        self.lib = load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_rows, self.max_in = int(max_rows), int(max_in)
        self._h = None
        self.byte_mode = False  # a row of the object has a format other than "f32": `step` takes and returns byte buffers
        self._rows: List[object] = [None] * self.max_rows  # per row: [L, M, consumed, emitted, in format, out format], the host arithmetic behind the size of y
        with torch.cuda.device(self.device):
            h = C.c_void_p()
            check(self.lib.kk_resampler_create(self.max_rows, self.max_in, C.byref(h)), "kk_resampler_create")
            self._h = h

    def _handle(self):
        if self._h is None:
            raise KokoroHipError("RowResampler is closed")
        return self._h

    def set_row(self, row: int, src: int, dst: int, in_format=None, out_format=None) -> None:
        """A new stream from `src` to `dst` Hz starts in `row`; whatever the row held is gone.  in_format / out_format (`pcm.FORMATS`; None:
        "f32"): what the row's new samples and its outputs are stored as."""
        L, M = ratio(src, dst)
        fi, fo = PCM.check(in_format), PCM.check(out_format)
        tab = phase_table(L, M)
        with torch.cuda.device(self.device):
            if fi == fo == "f32":
                check(self.lib.kk_resampler_set_row(self._handle(), _stream(self.device), int(row), L, M, tab.ctypes.data_as(C.c_void_p), int(tab.shape[1])),
                      "kk_resampler_set_row")
            else:
                check(self.lib.kk_resampler_set_row_fmt(self._handle(), _stream(self.device), int(row), L, M, tab.ctypes.data_as(C.c_void_p),
                                                        int(tab.shape[1]), PCM.CODES[fi], PCM.CODES[fo]), "kk_resampler_set_row_fmt")
        self._rows[int(row)] = [L, M, 0, 0, fi, fo]
        self.byte_mode = any(st is not None and (st[4] != "f32" or st[5] != "f32") for st in self._rows)

    def in_view(self, x, row: int):
        """Row `row` of a byte buffer for `step` as a 1-d tensor of the row's input format's dtype (no copy): where its new samples go."""
        return PCM.view(x, row, self._rows[int(row)][4]) if x.dtype == torch.uint8 else x[row]

    def out_view(self, y, row: int):
        """Row `row` of what `step` returned as a 1-d tensor of the row's output format's dtype (no copy); of an f32 object's y: y[row]."""
        return PCM.view(y, row, self._rows[int(row)][5]) if y.dtype == torch.uint8 else y[row]

    def _step_bytes(self, x, n, f):
        x = torch.as_tensor(x).to(self.device)
        if x.ndim != 2 or x.shape[0] != self.max_rows:
            raise ValueError(f"x must be [{self.max_rows}, W], got {tuple(x.shape)}")
        x = PCM.as_bytes(x)
        width = 16
        for b in range(self.max_rows):  # the size of y: the same integers the library computes
            st = self._rows[b]
            if st is not None and (n[b] > 0 or f[b]):
                N = st[2] + int(n[b])
                width = max(width, ((out_len(N, st[0], st[1]) if f[b] else ready(N, st[0], st[1])) - st[3]) * PCM.bytes_per_sample(st[5]))
        out = np.zeros(self.max_rows, np.int32)
        with torch.cuda.device(self.device):
            y = torch.empty((self.max_rows, -(-width // 16) * 16), dtype=torch.uint8, device=self.device)
            check(self.lib.kk_resampler_step_fmt(self._handle(), _stream(self.device), C.c_void_p(x.data_ptr()), int(x.shape[1]), n.ctypes.data_as(C.c_void_p),
                                                 f.ctypes.data_as(C.c_void_p), C.c_void_p(y.data_ptr()), int(y.shape[1]), out.ctypes.data_as(C.c_void_p)),
                  "kk_resampler_step_fmt")
        return y, out

    def step(self, x, n_in: Sequence[int], flush: Sequence[bool]):
        """x [max_rows, W] float32 on the device; row b consumes x[b, :n_in[b]].  flush[b]: the row's stream ends here, the rest of its
        outputs follow.  A row with n_in 0 and no flush sits out: its entries may hold anything, NaN included.  -> (y [max_rows, W'], n_out
        list): row b's new outputs are y[b, :n_out[b]].  No synchronisation.  In byte mode (a row with a format): x is taken as its bytes and
        y is [max_rows, W'] uint8; `out_view(y, b)[: n_out[b]]` are row b's outputs."""
        h = self._handle()
        n = np.ascontiguousarray(np.asarray(n_in, np.int32))
        f = np.ascontiguousarray(np.asarray(flush).astype(bool).astype(np.int32))
        if n.shape != (self.max_rows,) or f.shape != (self.max_rows,):
            raise ValueError(f"n_in and flush must hold {self.max_rows} entries")
        if self.byte_mode:
            y, out = self._step_bytes(x, n, f)
            for b in range(self.max_rows):
                if self._rows[b] is not None and (n[b] > 0 or f[b]):
                    self._rows[b][2] += int(n[b])
                    self._rows[b][3] += int(out[b])
            return y, out.tolist()
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32)
        if x.ndim != 2 or x.shape[0] != self.max_rows:
            raise ValueError(f"x must be [{self.max_rows}, W], got {tuple(x.shape)}")
        if x.shape[1] % 4:  # the kernel loads 16 bytes at a time from rows that start on a 16-byte boundary
            x = torch.nn.functional.pad(x, (0, 4 - x.shape[1] % 4))
        x = x.contiguous()
        if x.data_ptr() % 16:  # (a view that starts inside another tensor)
            x = x.clone()
        width = 0
        for b in range(self.max_rows):  # the size of y: the same integers the library computes
            st = self._rows[b]
            if st is not None and (n[b] > 0 or f[b]):
                N = st[2] + int(n[b])
                width = max(width, (out_len(N, st[0], st[1]) if f[b] else ready(N, st[0], st[1])) - st[3])
        out = np.zeros(self.max_rows, np.int32)
        with torch.cuda.device(self.device):
            y = torch.empty((self.max_rows, max(4, -(-width // 4) * 4)), dtype=torch.float32, device=self.device)
            check(self.lib.kk_resampler_step(h, _stream(self.device), C.c_void_p(x.data_ptr()), int(x.shape[1]), n.ctypes.data_as(C.c_void_p),
                                             f.ctypes.data_as(C.c_void_p), C.c_void_p(y.data_ptr()), int(y.shape[1]), out.ctypes.data_as(C.c_void_p)),
                  "kk_resampler_step")
        for b in range(self.max_rows):
            if self._rows[b] is not None and (n[b] > 0 or f[b]):
                self._rows[b][2] += int(n[b])
                self._rows[b][3] += int(out[b])
        return y, out.tolist()

    def close(self) -> None:
        if self._h is not None:
            self.lib.kk_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
