"""The PCM wire formats without a device: the reference of tests/_pcm_ref.py against Python's `audioop` on all 65 536 linear
values and all 256 octets, `mlx-audio_amd/pcm.py` against the reference on the same sets, the round trips, and the float edge cases of the
encode rule.  Every comparison is integer equality."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pcm_ref as P  # noqa: E402

from mlx_audio_amd import pcm  # noqa: E402

ALL16 = P.LINEAR.astype(np.int16)
ALL8 = np.arange(256, dtype=np.uint8)


def test_the_reference_against_audioop():
    audioop = pytest.importorskip("audioop")  # (leaves the standard library in Python 3.13)
    lin = ALL16.astype("<i2").tobytes()
    np.testing.assert_array_equal(np.frombuffer(audioop.lin2ulaw(lin, 2), np.uint8), P.MULAW_ENCODE)
    np.testing.assert_array_equal(np.frombuffer(audioop.lin2alaw(lin, 2), np.uint8), P.ALAW_ENCODE)
    np.testing.assert_array_equal(np.frombuffer(audioop.ulaw2lin(ALL8.tobytes(), 2), "<i2"), P.MULAW_DECODE)
    np.testing.assert_array_equal(np.frombuffer(audioop.alaw2lin(ALL8.tobytes(), 2), "<i2"), P.ALAW_DECODE)


def test_the_ranges_the_rules_state():
    assert (P.MULAW_DECODE.min(), P.MULAW_DECODE.max()) == (-32124, 32124)
    assert (P.ALAW_DECODE.min(), P.ALAW_DECODE.max()) == (-32256, 32256)
    assert pcm.FORMATS == P.FORMATS == ("f32", "s16le", "mulaw", "alaw")
    assert [pcm.bytes_per_sample(f) for f in pcm.FORMATS] == [4, 2, 1, 1]
    with pytest.raises(ValueError):
        pcm.bytes_per_sample("s16be")


@pytest.mark.parametrize("fmt", ["s16le", "mulaw", "alaw"])
def test_pcm_py_against_the_reference_exhaustively(fmt):
    stored = ALL16 if fmt == "s16le" else ALL8
    want = P.decode(stored, fmt)
    got = pcm.decode(stored, fmt)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(pcm.decode(stored.tobytes(), fmt), want)  # bytes are taken as the format's samples
    np.testing.assert_array_equal(pcm.decode(bytearray(stored.tobytes()), fmt), want)
    np.testing.assert_array_equal(pcm.decode(memoryview(stored.tobytes()), fmt), want)
    x = P.decode(ALL16, "s16le")  # every linear value as a float
    enc = pcm.encode(x, fmt)
    assert enc.dtype == P.DTYPES[fmt]
    np.testing.assert_array_equal(enc, P.encode(x, fmt))


def test_f32_is_the_identity_on_bits():
    x = P.specials()
    np.testing.assert_array_equal(pcm.encode(x, "f32").view(np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(pcm.decode(x, "f32").view(np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(pcm.decode(x.tobytes(), None).view(np.uint32), x.view(np.uint32))


def test_round_trips():
    np.testing.assert_array_equal(pcm.encode(pcm.decode(ALL16, "s16le"), "s16le"), ALL16)  # every int16
    np.testing.assert_array_equal(pcm.encode(pcm.decode(ALL8, "alaw"), "alaw"), ALL8)      # 256 / 256
    back = pcm.encode(pcm.decode(ALL8, "mulaw"), "mulaw")
    moved = np.nonzero(back != ALL8)[0].tolist()
    assert moved == [0x7F] and back[0x7F] == 0xFF                                          # 255 / 256: the negative zero comes back positive


def test_the_float_edge_cases():
    def s16(*v):
        return pcm.encode(np.array(v, np.float32), "s16le").tolist()

    assert s16(0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 3.5 / 32768) == [0, 2, 2, 4]        # ties go to even
    assert s16(-0.5 / 32768, -1.5 / 32768, -2.5 / 32768, -3.5 / 32768) == [0, -2, -2, -4]
    assert s16(1.0, -1.0, 1.5, -1.5) == [32767, -32768, 32767, -32768]
    assert s16(np.inf, -np.inf) == [32767, -32768]
    assert s16(np.nan) == [0]                                                              # not the clamp's -32768
    assert s16(-0.0, 1e-40, -1e-40) == [0, 0, 0]
    x = P.specials()
    for fmt in ("s16le", "mulaw", "alaw"):
        np.testing.assert_array_equal(pcm.encode(x, fmt), P.encode(x, fmt))
    assert pcm.encode(np.array([np.nan], np.float32), "mulaw").tolist() == [0xFF] and pcm.encode(np.array([np.nan], np.float32), "alaw").tolist() == [0xD5]


def test_what_samples_refuses():
    with pytest.raises(ValueError, match="whole number"):
        pcm.samples(b"\x00\x01\x02", "s16le")
    with pytest.raises(ValueError, match="whole number"):
        pcm.samples(b"\x00\x01\x02\x03\x04", "f32")
    with pytest.raises(ValueError, match="int16"):
        pcm.samples(np.zeros(4, np.float32), "s16le")
    with pytest.raises(ValueError, match="unknown PCM format"):
        pcm.samples(b"", "pcm24")
    assert pcm.samples(b"", "mulaw").shape == (0,)
