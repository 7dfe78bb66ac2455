"""The PCM wire formats on the device (kk_pcm.h, kk_resample.hip) against the plain reference of tests/_pcm_ref.py.  The
convert kernel on every 16-bit value, every octet and the float edge cases, at lengths that meet every tail of a 16-byte load; resampler
rows that read and write different formats in one object, bit-equal to `resample(decode(clip))` / `encode(resample(clip))` through the f32
entry points; the refusals.  Every comparison is integer equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _pcm_ref as P  # noqa: E402
import _resample_ref as R  # noqa: E402

from mlx_audio_amd import pcm  # noqa: E402
from mlx_audio_amd import resample as RS  # noqa: E402
from mlx_audio_amd._lib import KokoroHipError, load  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [1, 15, 16, 17, 255, 256, 257]
SLICES = [1, 7, 160, 1000]
ENCODED = ["s16le", "mulaw", "alaw"]


def _bits(a):
    """Stored samples as integers: NaN compares by its bits."""
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _stored(fmt, seed, n):
    """n stored samples of `fmt`: every value of the format is likely among them."""
    g = np.random.default_rng(seed)
    if fmt == "f32":
        return np.concatenate([P.specials(), (0.4 * g.standard_normal(n)).astype(np.float32)])[:n] if n > 40 else (0.4 * g.standard_normal(n)).astype(np.float32)
    return g.integers(-32768, 32768, n).astype(np.int16) if fmt == "s16le" else g.integers(0, 256, n).astype(np.uint8)


def _speech(seed, n):
    return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ---- (a) the convert kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fo", P.FORMATS)
@pytest.mark.parametrize("fi", P.FORMATS)
def test_convert_on_every_value_of_the_input_format(fi, fo):
    if fi == "f32":
        x = np.concatenate([P.decode(P.LINEAR.astype(np.int16), "s16le"), P.specials()])  # every linear value as a float, and the edge cases
    else:
        x = P.LINEAR.astype(np.int16) if fi == "s16le" else np.arange(256, dtype=np.uint8)
    want = P.encode(P.decode(x, fi), fo)
    got = pcm.convert(torch.from_numpy(x), fi, fo)
    assert got.dtype == pcm.torch_dtype(fo) and got.shape == (x.shape[0],)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    if fi != "f32":  # what the host rules take, the device takes: bytes
        assert torch.equal(pcm.convert(x.tobytes(), fi, fo), got)


@pytest.mark.parametrize("fo", P.FORMATS)
@pytest.mark.parametrize("fi", P.FORMATS)
def test_convert_rows_of_lengths_around_the_load(fi, fo):
    """One launch: a row per length, so every tail of a 16-byte load (4, 8 or 16 samples) is met; a row with n = 0 holds 0xFF bytes (NaN as
    floats) and is not read; the bytes of y behind a row's n samples stay as they were."""
    cv = pcm.RowConverter()
    rows = len(LENGTHS) + 1
    xs = [_stored(fi, 100 + n, n) for n in LENGTHS]
    buf = np.full((rows, 257 * 4 + 12), 0xFF, np.uint8)
    for r, x in enumerate(xs):
        buf[r, : x.nbytes] = x.view(np.uint8)
    y = cv.convert(torch.from_numpy(buf), [fi] * rows, [fo] * rows, LENGTHS + [0])
    assert y.dtype == torch.uint8 and y.shape[0] == rows and y.shape[1] % 16 == 0 and y.shape[1] >= 257 * P.BYTES[fo]
    for r, x in enumerate(xs):
        got = pcm.view(y, r, fo)[: LENGTHS[r]].cpu().numpy()
        np.testing.assert_array_equal(_bits(got), _bits(P.encode(P.decode(x, fi), fo)), err_msg=f"{fi} -> {fo}, n = {LENGTHS[r]}")


def test_convert_rows_with_a_format_per_row():
    cv = pcm.RowConverter()
    pairs = [(a, b) for a in P.FORMATS for b in P.FORMATS]
    xs = [_stored(a, 7 + i, 100 + i) for i, (a, _) in enumerate(pairs)]
    buf = np.zeros((len(pairs), 512), np.uint8)
    for r, x in enumerate(xs):
        buf[r, : x.nbytes] = x.view(np.uint8)
    y = cv.convert(torch.from_numpy(buf), [a for a, _ in pairs], [b for _, b in pairs], [x.shape[0] for x in xs])
    for r, (a, b) in enumerate(pairs):
        np.testing.assert_array_equal(_bits(pcm.view(y, r, b)[: xs[r].shape[0]].cpu().numpy()), _bits(P.encode(P.decode(xs[r], a), b)))


# ---- (b) resampler rows with formats ----------------------------------------------------------------------------------------------------------
ROWS = [  # (source rate, destination rate, input format, output format, clip length)
    (8000, 24000, "mulaw", "f32", 2400),
    (44100, 24000, "s16le", "f32", 3100),
    (24000, 8000, "f32", "mulaw", 2777),
    (24000, 48000, "f32", "s16le", 2001),
]


def _want(stored, src, dst, fi, fo):
    """What a row must give, through the f32 entry points alone: encode(resample(decode(clip)))."""
    y = RS.resample(torch.from_numpy(P.decode(stored, fi)), src, dst).cpu().numpy()
    return P.encode(y, fo)


def test_rows_with_mixed_formats_are_bit_equal_whatever_the_slicing_and_the_neighbours():
    clips = [P.encode(_speech(20 + r, n), fi) for r, (_, _, fi, _, n) in enumerate(ROWS)]
    want = [_want(clips[r], *ROWS[r][:4]) for r in range(4)]
    rows, start = 5, [0, 2, 5, 1]  # row 4 is never set: its bytes are 0xFF throughout (NaN as floats)
    rs = RS.RowResampler(rows, 1000)
    fed, emitted, got = [0] * 4, [0] * 4, [[] for _ in range(4)]
    flushed, started = [False] * 4, [False] * 4
    step = 0
    while not all(flushed):
        x = np.full((rows, 4000), 0xFF, np.uint8)
        n_in, flush, cnt = [0] * rows, [False] * rows, [0] * rows
        for r, (src, dst, fi, fo, N) in enumerate(ROWS):
            if step < start[r] or flushed[r] or (step + r) % 3 == 0:  # not started yet, done, or sitting this step out
                continue
            if not started[r]:
                rs.set_row(r, src, dst, in_format=fi, out_format=fo)
                started[r] = True
            k = min(SLICES[(step + r) % 4], N - fed[r])
            piece = clips[r][fed[r] : fed[r] + k]
            x[r, : piece.nbytes] = piece.view(np.uint8)
            n_in[r], fed[r] = k, fed[r] + k
            flush[r] = flushed[r] = fed[r] == N
            L, M = RS.ratio(src, dst)
            cnt[r] = (R.out_len(fed[r], L, M) if flush[r] else R.ready(fed[r], L, M)) - emitted[r]
            emitted[r] += cnt[r]
        y, n_out = rs.step(torch.from_numpy(x), n_in, flush)
        assert n_out == cnt  # host integer arithmetic, no sync
        assert y.dtype == torch.uint8 or not any(started)  # bytes out from the first row with a format on
        for r in range(4):
            if started[r]:
                got[r].append(rs.out_view(y, r)[: n_out[r]].cpu().numpy())
        step += 1
    assert step > 8
    for r in range(4):
        out = np.concatenate(got[r])
        assert out.dtype == P.DTYPES[ROWS[r][3]] and out.shape == want[r].shape
        np.testing.assert_array_equal(_bits(out), _bits(want[r]), err_msg=str(ROWS[r]))
    rs.close()


def _lengths_for(L, M, outs):
    return sorted({next(n for n in range(1, outs[-1] * M + 2) if R.out_len(n, L, M) >= o) for o in outs})


@pytest.mark.parametrize("fi,fo", [("s16le", "f32"), ("mulaw", "f32"), ("alaw", "f32"), ("f32", "s16le"), ("f32", "alaw"), ("mulaw", "s16le")])
def test_edge_lengths_around_a_workgroups_outputs(fi, fo):
    src, dst = 44100, 24000
    L, M = RS.ratio(src, dst)
    B = int(load().kk_resampler_block_outputs())
    lengths = [1, 5] + _lengths_for(L, M, [B - 1, B, B + 1])
    assert [R.out_len(n, L, M) for n in lengths[2:]] == [B - 1, B, B + 1]
    for N in lengths:
        stored = P.encode(_speech(N, N), fi)
        got = RS.resample(torch.from_numpy(stored), src, dst, in_format=fi, out_format=fo)
        assert got.dtype == pcm.torch_dtype(fo)
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(_want(stored, src, dst, fi, fo)), err_msg=f"N = {N}")


@pytest.mark.parametrize("fi", P.FORMATS)
@pytest.mark.parametrize("src", [8000, 44100])
def test_steps_of_1_to_17_new_samples(fi, src):
    """n_in = 1 ... 17 in turn: the window's start falls on every offset within the load granule of the row's format, and every step's new
    samples end inside one."""
    N = sum(range(1, 18))
    stored = P.encode(_speech(src + len(fi), N), fi)
    rs = RS.RowResampler(2, 32)
    rs.set_row(1, src, 24000, in_format=fi, out_format="s16le")
    got, fed = [], 0
    for k in range(1, 18):
        x = np.full((2, 80), 0xFF, np.uint8)
        piece = stored[fed : fed + k]
        x[1, : piece.nbytes] = piece.view(np.uint8)
        fed += k
        y, n = rs.step(torch.from_numpy(x), [0, k], [False, fed == N])
        got.append(rs.out_view(y, 1)[: n[1]].cpu().numpy())
    np.testing.assert_array_equal(np.concatenate(got), _want(stored, src, 24000, fi, "s16le"))
    rs.close()


def test_alaw_through_the_multi_pass_window():
    """11.025 -> 24 kHz is 320 / 147: the largest tap table, and 24 kHz -> 75 Hz (1 / 320) a window of several LDS passes, here over A-law."""
    for src, dst, N in ((11025, 24000, 300), (24000, 75, 40 * 320 - 17)):
        stored = P.encode(_speech(N, N), "alaw")
        want = _want(stored, src, dst, "alaw", "f32")
        rs = RS.RowResampler(2, 40000)
        rs.set_row(1, src, dst, in_format="alaw")
        got, fed = [], 0
        for k in (133, 7, 40000):
            k = min(k, N - fed)
            buf = np.full((2, max(16, -(-k // 16) * 16)), 0xFF, np.uint8)
            buf[1, :k] = stored[fed : fed + k]
            fed += k
            y, n = rs.step(torch.from_numpy(buf), [0, k], [False, fed == N])
            got.append(rs.out_view(y, 1)[: n[1]].cpu().numpy())
        np.testing.assert_array_equal(_bits(np.concatenate(got)), _bits(want))
        rs.close()


def test_a_row_reused_with_another_format():
    rs = RS.RowResampler(2, 512)
    a, b = P.encode(_speech(1, 700), "mulaw"), P.encode(_speech(2, 900), "s16le")
    rs.set_row(0, 8000, 24000, in_format="mulaw")
    buf = np.zeros((2, 512), np.uint8)
    buf[0] = a[:512]
    rs.step(torch.from_numpy(buf), [512, 0], [False, False])  # row 0 holds a mu-law stream's history and counts
    rs.set_row(0, 24000, 48000, in_format="s16le", out_format="alaw")  # ... and starts over with other formats, without a flush
    got = []
    for lo in (0, 512):
        k = min(512, 900 - lo)
        buf = np.zeros((2, 1024), np.uint8)
        buf[0, : 2 * k] = b[lo : lo + k].view(np.uint8)
        y, n = rs.step(torch.from_numpy(buf), [k, 0], [lo + k == 900, False])
        got.append(rs.out_view(y, 0)[: n[0]].cpu().numpy())
    np.testing.assert_array_equal(np.concatenate(got), _want(b, 24000, 48000, "s16le", "alaw"))
    rs.set_row(0, 16000, 24000)  # back to f32 on both sides: the object leaves byte mode and `step` is the f32 entry again
    assert not rs.byte_mode
    c = _speech(3, 300)
    y, n = rs.step(torch.from_numpy(np.stack([c, c])), [300, 0], [True, False])
    assert y.dtype == torch.float32
    assert torch.equal(y[0, : n[0]], RS.resample(torch.from_numpy(c), 16000, 24000))
    rs.close()


# ---- (c) refusals -----------------------------------------------------------------------------------------------------------------------------
def _err(lib):
    return lib.kk_last_error().decode()


def test_refusals_come_before_any_launch_and_leave_y_untouched():
    lib = load()
    rs = RS.RowResampler(2, 64)
    h, st = rs._handle(), RS._stream(rs.device)
    tab = RS.phase_table(3, 1)
    taps, T = tab.ctypes.data_as(C.c_void_p), int(tab.shape[1])
    for bad in ((4, 0), (0, 4), (-1, 0), (0, 99)):
        assert lib.kk_resampler_set_row_fmt(h, st, 0, 3, 1, taps, T, *bad) != 0 and "unknown format" in _err(lib)
    with pytest.raises(ValueError, match="unknown PCM format"):
        rs.set_row(0, 8000, 24000, in_format="s16be")
    clip = P.encode(_speech(3, 150), "mulaw")
    want = _want(clip, 8000, 24000, "mulaw", "s16le")
    rs.set_row(0, 8000, 24000, in_format="mulaw", out_format="s16le")
    x = torch.zeros((2, 80), dtype=torch.uint8, device=rs.device)
    x[0, :64] = torch.from_numpy(clip[:64]).to(rs.device)
    y = torch.full((2, 1024), 0xA5, dtype=torch.uint8, device=rs.device)
    n_in, flush, n_out = (C.c_int32 * 2)(64, 0), (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)()
    xp, yp = x.data_ptr(), y.data_ptr()
    assert xp % 16 == 0 and yp % 16 == 0

    def step(xp=xp, ldx=80, yp=yp, ldy=1024, entry=lib.kk_resampler_step_fmt):
        return entry(h, st, C.c_void_p(xp), ldx, n_in, flush, C.c_void_p(yp), ldy, n_out)

    assert step(entry=lib.kk_resampler_step, ldx=20, ldy=256) != 0 and "f32 entry" in _err(lib)  # the f32 entry on a row with formats
    assert step(xp=xp + 4) != 0 and "x must be 16-byte aligned" in _err(lib)
    assert step(yp=yp + 8) != 0 and "y must be 16-byte aligned" in _err(lib)
    assert step(ldx=72) != 0 and "multiple of 16" in _err(lib)
    assert step(ldy=1000) != 0 and "multiple of 16" in _err(lib)
    assert step(ldx=48) != 0 and "64 samples in a row of 48" in _err(lib)          # 48 bytes hold 48 octets
    k = R.ready(64, 3, 1)
    assert k > 8 and step(ldy=16) != 0 and f"{k} outputs in a row of 8" in _err(lib)  # 16 bytes hold 8 int16
    torch.cuda.synchronize()
    assert bool((y == 0xA5).all())  # nothing was launched
    got = []
    for lo in range(0, 150, 64):  # the refused calls changed nothing: the stream is whole
        k = min(64, 150 - lo)
        buf = np.zeros((2, 64), np.uint8)
        buf[0, :k] = clip[lo : lo + k]
        out, n = rs.step(torch.from_numpy(buf), [k, 0], [lo + k == 150, False])
        got.append(rs.out_view(out, 0)[: n[0]].cpu().numpy())
    np.testing.assert_array_equal(np.concatenate(got), want)
    rs.close()
    # the convert entries
    cx = torch.zeros((2, 64), dtype=torch.uint8, device=rs.device)
    cy = torch.full((2, 64), 0xA5, dtype=torch.uint8, device=rs.device)

    def conv(fi=(2, 2), fo=(1, 1), n=(16, 16), xp=cx.data_ptr(), ldx=64, yp=cy.data_ptr(), ldy=64, rows=2):
        return lib.kk_pcm_convert_rows(st, rows, C.c_void_p(xp), ldx, (C.c_int32 * 2)(*fi), C.c_void_p(yp), ldy, (C.c_int32 * 2)(*fo), (C.c_int32 * 2)(*n))

    assert conv(fi=(2, 7)) != 0 and "unknown format" in _err(lib)
    assert conv(fo=(-1, 1)) != 0 and "unknown format" in _err(lib)
    assert conv(xp=cx.data_ptr() + 2) != 0 and "16-byte aligned" in _err(lib)
    assert conv(yp=cy.data_ptr() + 1) != 0 and "16-byte aligned" in _err(lib)
    assert conv(ldx=40) != 0 and conv(ldy=56) != 0 and "multiples of 16" in _err(lib)
    assert conv(n=(16, 65)) != 0 and "65 samples in a row of 64" in _err(lib)
    assert conv(n=(33, 16)) != 0 and "33 samples into a row of 32" in _err(lib)     # 64 bytes hold 32 int16
    assert conv(n=(-1, 16)) != 0 and conv(rows=0) != 0 and conv(rows=65) != 0
    assert lib.kk_op_pcm_convert(st, C.c_void_p(cx.data_ptr()), 5, C.c_void_p(cy.data_ptr()), 0, 8) != 0 and "unknown format" in _err(lib)
    assert lib.kk_op_pcm_convert(st, C.c_void_p(cx.data_ptr()), 0, C.c_void_p(cy.data_ptr()), 0, 0) != 0
    torch.cuda.synchronize()
    assert bool((cy == 0xA5).all())
    assert conv(fi=(2, 7), n=(16, 0)) == 0  # a row that sits out: its formats are not read either
    torch.cuda.synchronize()
    assert bool((cy[1] == 0xA5).all()) and bool((cy[0, 32:] == 0xA5).all())
    assert torch.equal(cy[0, :32].view(torch.int16).cpu(), torch.from_numpy(P.encode(P.decode(np.zeros(16, np.uint8), "mulaw"), "s16le")))
    with pytest.raises(KokoroHipError):
        pcm.RowConverter().convert(torch.zeros((1, 16), dtype=torch.uint8), ["mulaw"], ["s16le"], [17])
    with pytest.raises(ValueError):
        pcm.convert(torch.zeros(4), "s16le", "f32")
