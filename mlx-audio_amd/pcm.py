"""PCM wire formats of the audio edges of CSM serving: what a phone line, a browser microphone and a playback device speak.

    "f32"    4 bytes, the float itself
    "s16le"  2 bytes, little-endian int16 s:  x = s / 32768 (exact in float32);  s = clamp(rint(x 32768), -32768, 32767), ties to even,
             +-inf -> full scale, NaN -> 0
    "mulaw"  1 byte, G.711 mu-law of s (decodes to +-32124);   "alaw"  1 byte, G.711 A-law of s (decodes to +-32256)

The integer rules are those of Python's `audioop` at width 2 (`lin2ulaw`, `ulaw2lin`, `lin2alaw`, `alaw2lin`) on every 16-bit value and every
octet.  `decode` / `encode` are numpy, for callers and for tests without a device; `convert` and `RowConverter` run the same rules on the
device (pcm_convert_rows_kernel; no CPU or PyTorch fallback: without the library they raise), and `resample.RowResampler` rows apply them
inside the resampler's launch."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

FORMATS = ("f32", "s16le", "mulaw", "alaw")
CODES = {"f32": 0, "s16le": 1, "mulaw": 2, "alaw": 3}  # KK_PCM_*
_BYTES = {"f32": 4, "s16le": 2, "mulaw": 1, "alaw": 1}
_DTYPES = {"f32": np.dtype("<f4"), "s16le": np.dtype("<i2"), "mulaw": np.dtype("u1"), "alaw": np.dtype("u1")}


def check(fmt: Optional[str]) -> str:
    """The format's name; None means "f32".  ValueError for anything else."""
    if fmt is None:
        return "f32"
    if fmt not in CODES:
        raise ValueError(f"unknown PCM format {fmt!r}: one of {', '.join(FORMATS)}")
    return fmt


def bytes_per_sample(fmt: Optional[str]) -> int:
    return _BYTES[check(fmt)]


def dtype(fmt: Optional[str]) -> np.dtype:
    """The numpy dtype a sample of `fmt` is stored as."""
    return _DTYPES[check(fmt)]


def samples(data, fmt: Optional[str]) -> np.ndarray:
    """`data` as a 1-d array of the format's dtype, without a copy where there is none to make: `bytes`, `bytearray`, `memoryview`, or a
    numpy array of that dtype.  ValueError for a byte count that is no whole number of samples and for an array of another dtype."""
    dt = dtype(fmt)
    if isinstance(data, (bytes, bytearray, memoryview)):
        n = memoryview(data).nbytes
        if n % dt.itemsize:
            raise ValueError(f"{n} bytes are no whole number of {check(fmt)} samples ({dt.itemsize} bytes each)")
        return np.frombuffer(data, dtype=dt)
    a = np.asarray(data)
    if a.dtype != dt:
        raise ValueError(f"{check(fmt)} samples are {dt.name}, got an array of {a.dtype.name}")
    return a.reshape(-1)


def _mulaw_to_s16(u: np.ndarray) -> np.ndarray:
    u = ~u.astype(np.int32) & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def _alaw_to_s16(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.int32) ^ 0x55
    m, e = a & 15, (a >> 4) & 7
    t = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, t, -t)


def _log2(v: np.ndarray) -> np.ndarray:
    """floor(log2(v)) of int32 v in [1, 2^15]: exact, by counting shifts."""
    e = np.zeros_like(v)
    for k in range(1, 16):
        e += (v >> k) > 0
    return e


def _s16_to_mulaw(s: np.ndarray) -> np.ndarray:
    v = s.astype(np.int32) >> 2
    neg = v < 0
    mag = np.minimum(np.abs(v), 8159) + 0x21
    e = _log2(mag) - 5
    code = np.where(e >= 8, 0x7F, (e << 4) | ((mag >> (e + 1)) & 15))
    return (code ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def _s16_to_alaw(s: np.ndarray) -> np.ndarray:
    v = s.astype(np.int32) >> 3
    pos = v >= 0
    mag = np.minimum(np.where(pos, v, -v - 1), 4095)
    e = np.where(mag < 32, 0, _log2(np.maximum(mag, 1)) - 4)
    m = np.where(e == 0, (mag >> 1) & 15, (mag >> e) & 15)
    return ((((e << 4) | m) | np.where(pos, 0x80, 0)) ^ 0x55).astype(np.uint8)


def _f32_to_s16(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.clip(np.rint(x * np.float32(32768.0)), -32768.0, 32767.0)  # (rint: ties to even; +-inf clip to full scale)
    return np.where(np.isnan(x), 0, r).astype(np.int16)


def decode(data, fmt: Optional[str]) -> np.ndarray:
    """Stored samples (`samples(data, fmt)`) -> float32 [n].  Exact: a 16-bit linear value over 2^15."""
    a = samples(data, fmt)
    if check(fmt) == "f32":
        return a.astype(np.float32)
    s = a.astype(np.int32) if fmt == "s16le" else _mulaw_to_s16(a) if fmt == "mulaw" else _alaw_to_s16(a)
    return (s.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def encode(x, fmt: Optional[str]) -> np.ndarray:
    """float32 [n] -> the stored samples: float32, int16 ("s16le") or uint8 ("mulaw", "alaw")."""
    x = np.asarray(x, np.float32).reshape(-1)
    if check(fmt) == "f32":
        return x.copy()
    s = _f32_to_s16(x)
    return s if fmt == "s16le" else _s16_to_mulaw(s) if fmt == "mulaw" else _s16_to_alaw(s)


# ---- on the device ----------------------------------------------------------------------------------------------------------------------------
def torch_dtype(fmt: Optional[str]):
    import torch

    return {"f32": torch.float32, "s16le": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8}[check(fmt)]


def view(buf, row: int, fmt: Optional[str]):
    """Row `row` of a byte buffer [rows, W] (W a multiple of 16) as a 1-d tensor of the format's dtype: no copy."""
    return buf[row].view(torch_dtype(fmt))


def as_bytes(x):
    """A 2-d device tensor as its bytes, [rows, W] uint8 with W a multiple of 16 and a 16-byte aligned start: what the library's byte
    entry points take.  No copy for a contiguous, aligned tensor whose rows are whole 16-byte groups."""
    import torch

    if x.ndim != 2:
        raise ValueError(f"a [rows, W] tensor is needed, got {tuple(x.shape)}")
    b = x.contiguous().view(torch.uint8)
    if b.shape[1] % 16:
        b = torch.nn.functional.pad(b, (0, 16 - b.shape[1] % 16))
    if b.data_ptr() % 16:  # (a view that starts inside another tensor)
        b = b.clone()
    return b


class RowConverter:
    """Rows that need no ratio (`kk_pcm_convert_rows`): `convert(x, in_formats, out_formats, n)` is ONE stateless launch on the current
    stream of `device` for every row with n > 0, any format to any format.  The audio edge of serving for rows at the model's own rate."""

    def __init__(self, device=None):
        import torch

        from ._lib import load

        self.lib = load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def convert(self, x, in_formats: Sequence[Optional[str]], out_formats: Sequence[Optional[str]], n: Sequence[int]):
        """x [rows, W] on the device, taken as its bytes: row b holds n[b] samples of in_formats[b].  -> y [rows, W'] uint8: row b's first
        n[b] samples of out_formats[b] (`view(y, b, fmt)[: n[b]]`).  A row with n 0 sits out: nothing of it is read.  No synchronisation."""
        import torch

        from ._lib import check as _check

        x = as_bytes(torch.as_tensor(x).to(self.device))
        rows = int(x.shape[0])
        if not (len(in_formats) == len(out_formats) == len(n) == rows):
            raise ValueError(f"in_formats, out_formats and n must hold {rows} entries")
        fi = np.array([CODES[check(f)] for f in in_formats], np.int32)
        fo = np.array([CODES[check(f)] for f in out_formats], np.int32)
        cnt = np.ascontiguousarray(np.asarray(n, np.int32))
        width = max([int(k) * bytes_per_sample(f) for k, f in zip(cnt, out_formats)] + [16])
        with torch.cuda.device(self.device):
            y = torch.empty((rows, -(-width // 16) * 16), dtype=torch.uint8, device=self.device)
            _check(self.lib.kk_pcm_convert_rows(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), rows, C.c_void_p(x.data_ptr()),
                                                int(x.shape[1]), fi.ctypes.data_as(C.c_void_p), C.c_void_p(y.data_ptr()), int(y.shape[1]),
                                                fo.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)), "kk_pcm_convert_rows")
        return y

    def close(self) -> None:
        pass


def convert(x, in_format: Optional[str], out_format: Optional[str], device=None):
    """Stored samples [n] of `in_format` (a tensor of the format's dtype, or what `samples` takes) -> a device tensor [n] of `out_format`'s
    dtype: `encode(decode(x, in_format), out_format)` on the device (`kk_op_pcm_convert`)."""
    import torch

    from ._lib import check as _check, load

    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.array(samples(x, in_format)))
    if x.dtype != torch_dtype(in_format):
        raise ValueError(f"{check(in_format)} samples are {torch_dtype(in_format)}, got {x.dtype}")
    device = torch.device(device) if device is not None else (x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    x = x.to(device).reshape(-1).contiguous()
    if x.shape[0] < 1:
        raise ValueError("convert: no samples")
    if x.data_ptr() % 16:
        x = x.clone()
    with torch.cuda.device(device):
        y = torch.empty(x.shape[0], dtype=torch_dtype(out_format), device=device)
        _check(load().kk_op_pcm_convert(C.c_void_p(torch.cuda.current_stream(device).cuda_stream), C.c_void_p(x.data_ptr()), CODES[check(in_format)],
                                        C.c_void_p(y.data_ptr()), CODES[check(out_format)], int(x.shape[0])), "kk_op_pcm_convert")
    return y
