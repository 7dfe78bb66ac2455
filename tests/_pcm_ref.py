"""The PCM wire formats of DESIGN 8d-11 in plain numpy and plain Python integers: the reference the package's `pcm.py` and the device kernels
are compared with.  It imports nothing of the package.  The G.711 rules are written one value at a time, as the issue states them, and
tabulated once over all 65 536 linear values and all 256 octets; test_pcm_cpu.py holds the tables against Python's `audioop`."""
import numpy as np

FORMATS = ("f32", "s16le", "mulaw", "alaw")
BYTES = {"f32": 4, "s16le": 2, "mulaw": 1, "alaw": 1}
DTYPES = {"f32": np.float32, "s16le": np.int16, "mulaw": np.uint8, "alaw": np.uint8}


def mulaw_to_lin(u: int) -> int:
    u = ~u & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return 0x84 - t if u & 0x80 else t - 0x84


def lin_to_mulaw(s: int) -> int:
    v = s >> 2  # Python's >> floors, like an arithmetic shift
    neg = v < 0
    mag = min(abs(v), 8159) + 0x21
    e = mag.bit_length() - 1 - 5
    code = 0x7F if e >= 8 else (e << 4) | ((mag >> (e + 1)) & 15)
    return code ^ (0x7F if neg else 0xFF)


def alaw_to_lin(a: int) -> int:
    a ^= 0x55
    m, e = a & 15, (a >> 4) & 7
    t = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return t if a & 0x80 else -t


def lin_to_alaw(s: int) -> int:
    v = s >> 3
    pos = v >= 0
    mag = min(v if pos else -v - 1, 4095)
    e = 0 if mag < 32 else mag.bit_length() - 1 - 4
    m = (mag >> 1) & 15 if e == 0 else (mag >> e) & 15
    return (((e << 4) | m) | (0x80 if pos else 0)) ^ 0x55


LINEAR = np.arange(-32768, 32768, dtype=np.int32)            # every int16, in order: index s + 32768
MULAW_DECODE = np.array([mulaw_to_lin(u) for u in range(256)], np.int32)
ALAW_DECODE = np.array([alaw_to_lin(a) for a in range(256)], np.int32)
MULAW_ENCODE = np.array([lin_to_mulaw(int(s)) for s in LINEAR], np.uint8)
ALAW_ENCODE = np.array([lin_to_alaw(int(s)) for s in LINEAR], np.uint8)


def f32_to_lin(x) -> np.ndarray:
    """clamp(rint(x 32768)) with ties to even, +-inf to full scale and NaN to 0, in float64 (x 2^15 is exact there for every finite float32)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    out = np.zeros(x.shape, np.int32)
    ok = ~np.isnan(x)
    out[ok] = np.clip(np.rint(x[ok] * 32768.0), -32768, 32767).astype(np.int32)
    return out


def decode(data, fmt: str) -> np.ndarray:
    """Stored samples (an array of DTYPES[fmt]) -> float32."""
    a = np.asarray(data)
    assert a.dtype == DTYPES[fmt], (a.dtype, fmt)
    if fmt == "f32":
        return a.copy()
    s = a.astype(np.int32) if fmt == "s16le" else (MULAW_DECODE if fmt == "mulaw" else ALAW_DECODE)[a]
    return (s.astype(np.float64) / 32768.0).astype(np.float32)  # exact: |s| <= 2^15


def encode(x, fmt: str) -> np.ndarray:
    """float32 -> stored samples of DTYPES[fmt]."""
    x = np.asarray(x, np.float32)
    if fmt == "f32":
        return x.copy()
    s = f32_to_lin(x)
    if fmt == "s16le":
        return s.astype(np.int16)
    return (MULAW_ENCODE if fmt == "mulaw" else ALAW_ENCODE)[s + 32768]


def specials() -> np.ndarray:
    """float32 inputs whose encoding the rules single out: ties at (k + 0.5) / 32768 for even and odd k of either sign, +-1.0, +-1.5, +-inf,
    NaN, -0.0, a denormal, the largest finite values, and the neighbours of the clamp."""
    k = np.array([0, 1, 2, 3, 100, 101, 32765, 32766, -1, -2, -3, -4, -101, -102, -32767, -32768], np.float64)
    ties = ((k + 0.5) / 32768.0).astype(np.float32)
    assert np.array_equal(ties.astype(np.float64) * 32768.0, k + 0.5)  # the ties are exact in float32
    rest = np.array([1.0, -1.0, 1.5, -1.5, np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1e-40, 3.4028235e38, -3.4028235e38,
                     32767.0 / 32768.0, 32767.4 / 32768.0, 32767.6 / 32768.0, -32768.4 / 32768.0, -32768.6 / 32768.0, 1e-5, -1e-5], np.float32)
    return np.concatenate([ties, rest])
