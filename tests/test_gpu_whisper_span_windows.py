"""kk_op_log_mel_spans / whisper.span_windows on the device (csrc/kk_whisper.hip): a span of a sample buffer -- flat, or the ring of
ring.py at a 64-bit stream position -- becomes a Whisper window in one launch pair.  Every expected value is the composition of the existing ops,
    mel_windows([log_mel_spectrogram(resample(x, src, 16000), n_mels, padding=W * 160)], [0], [W], W)[0],
compared with torch.equal: no tolerance.  Whatever lies outside a span is NaN in these buffers, so a kernel that read or multiplied it would show."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _whisper_ref as R  # noqa: E402

from mlx_audio_amd import resample as RS  # noqa: E402
from mlx_audio_amd import whisper  # noqa: E402

pytestmark = pytest.mark.gpu

W = 200
LENGTHS = [1, 301, 719, 12345, 47999, 48000]  # the last two are both 32000 = W * 160 samples at 16 kHz
PIN = os.path.join(ROOT, "tests", "golden", "whisper_logmel_pin.json")

_clips, _wants = {}, {}


def clip(n, seed=0):
    if (n, seed) not in _clips:
        _clips[(n, seed)] = torch.from_numpy(R.signal(n, 7000 + 13 * seed + n % 991)).cuda()
    return _clips[(n, seed)]


def compose(x, Wn, n_mels, src_rate=24000):
    """-> (the window, the whole padded clip's spectrogram) from the existing ops"""
    a = RS.resample(x.clone(), src_rate, 16000)
    mel = whisper.log_mel_spectrogram(a, n_mels, padding=Wn * 160).contiguous()
    return whisper.mel_windows([mel], [0], [Wn], Wn)[0], mel


def want(n, n_mels, seed=0):
    if (n, n_mels, seed) not in _wants:
        _wants[(n, n_mels, seed)] = compose(clip(n, seed), W, n_mels)[0]
    return _wants[(n, n_mels, seed)]


def flat(x, offset, tail=29):
    """x inside a buffer that is NaN everywhere else -> Span"""
    buf = torch.full((offset + x.shape[0] + tail,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset : offset + x.shape[0]] = x
    return whisper.Span(buf, 0, offset, int(x.shape[0]))


def ring(x, ring_len, pos):
    """x in a ring of ring_len from stream position pos on, NaN in every other slot -> Span"""
    buf = torch.full((ring_len,), float("nan"), dtype=torch.float32, device="cuda")
    idx = (pos + torch.arange(x.shape[0], dtype=torch.int64)) % ring_len
    buf[idx.cuda()] = x
    return whisper.Span(buf, ring_len, pos, int(x.shape[0]))


def check(got, exp, what):
    assert got.dtype == torch.float32 and got.shape == exp.shape, what
    assert bool(torch.isfinite(got).all()), f"{what}: something outside the span was read or multiplied"
    assert torch.equal(got, exp), f"{what}: max difference {float((got - exp).abs().max()):.3e}"


@pytest.mark.parametrize("n_mels", [80, 128])
def test_lengths_at_the_boundaries_on_a_flat_buffer_at_an_odd_offset(n_mels):
    for n in LENGTHS:
        got = whisper.span_windows([flat(clip(n), 37 + n % 5)], W, n_mels)
        assert got.shape == (1, W, n_mels)
        check(got[0], want(n, n_mels), f"n = {n}")
    assert RS.out_len(47999, 2, 3) == RS.out_len(48000, 2, 3) == W * 160
    with pytest.raises(ValueError, match="row 0"):
        whisper.span_windows([flat(torch.zeros(48001, device="cuda"), 3)], W, n_mels)
    with pytest.raises(ValueError, match="row 1"):
        whisper.span_windows([flat(clip(301), 3), flat(torch.zeros(48001, device="cuda"), 3)], W, n_mels)


@pytest.mark.parametrize("ring_len,cases", [(5000, [(301, 4900), (719, 2 ** 32 + 4999), (5000, 2 ** 33 + 1234), (1, 4999)]),
                                            (48000, [(12345, 40000), (48000, 2 ** 32 + 17), (47999, 3 * 48000 + 47000), (719, 0)])])
def test_spans_of_a_ring_wrap_and_start_above_two_to_the_32(ring_len, cases):
    for n, pos in cases:
        x = clip(n, 1)
        got = whisper.span_windows([ring(x, ring_len, pos)], W, 80)
        check(got[0], want(n, 80, 1), f"ring {ring_len}, n = {n}, pos = {pos}")
    assert any(pos % ring_len + n > ring_len for n, pos in cases) and any(pos > 2 ** 32 for n, pos in cases)


def test_five_rows_of_one_launch_equal_their_own_launches_and_the_composition():
    a, b, c, d = clip(12345, 2), clip(719, 2), clip(48000, 2), clip(301, 2)
    shared = torch.full((20000,), float("nan"), dtype=torch.float32, device="cuda")  # two rows name this buffer
    shared[11:11 + 719] = b
    shared[5001:5001 + 12345] = a
    spans = [ring(c, 48000, 2 ** 32 + 40001), whisper.Span(shared, 0, 5001, 12345), flat(d, 3), whisper.Span(shared, 0, 11, 719), ring(d, 5000, 4990)]
    exp = [want(48000, 80, 2), want(12345, 80, 2), want(301, 80, 2), want(719, 80, 2), want(301, 80, 2)]
    got = whisper.span_windows(spans, W, 80)
    assert got.shape == (5, W, 80)
    for r, sp in enumerate(spans):
        check(got[r], exp[r], f"row {r} of five")
        check(whisper.span_windows([sp], W, 80)[0], exp[r], f"row {r} alone")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_identity_ratio(n_mels):
    for n in (1, 719, 31999, 32000):
        x = clip(n, 3)
        exp = whisper.log_mel_spectrogram(x.clone(), n_mels, padding=W * 160)[:W]
        check(whisper.span_windows([flat(x, 5)], W, n_mels, src_rate=16000)[0], exp, f"16 kHz flat, n = {n}")
        check(whisper.span_windows([ring(x, 32000, 2 ** 32 + 31000)], W, n_mels, src_rate=16000)[0], exp, f"16 kHz ring, n = {n}")
    with pytest.raises(ValueError, match="row 0"):
        whisper.span_windows([flat(torch.zeros(32001, device="cuda"), 1)], W, n_mels, src_rate=16000)


def test_other_ratios_are_served_or_refused_by_name():
    for src, n in ((8000, 4001), (48000, 95999), (32000, 64000), (12000, 777)):
        x = clip(n, 4)
        check(whisper.span_windows([flat(x, 9)], W, 80, src_rate=src)[0], compose(x, W, 80, src)[0], f"{src} Hz")
    x = flat(torch.zeros(1000, device="cuda"), 0)
    with pytest.raises(ValueError, match="1 / 6"):  # 96 kHz: a frame reads 2 500 source samples
        whisper.span_windows([x], W, 80, src_rate=96000)
    with pytest.raises(ValueError, match="160 / 441"):  # 44.1 kHz: past resample.ratio's bound
        whisper.span_windows([x], W, 80, src_rate=44100)


def test_the_maximum_comes_from_a_frame_that_is_not_stored():
    g = torch.Generator().manual_seed(5)
    x = 1e-4 * torch.randn(48000, generator=g)
    x[-100:] += 0.5 * torch.randn(100, generator=g)
    x = x.cuda()
    exp, mel = compose(x, W, 80)
    assert mel.shape[0] == 2 * W
    # (the clamp and the scale are monotonic: the arg-max frame of the finished spectrogram is the arg-max frame of the raw one)
    assert int(mel.max(dim=1).values.argmax()) >= W, "the case must put the clip's maximum into a frame that is not stored"
    assert float(mel[W:].max()) > float(mel[:W].max())
    check(whisper.span_windows([flat(x, 7)], W, 80)[0], exp, "burst in the last 100 samples")


def test_production_shape():
    n = 720000
    x = clip(n, 6)
    exp, _ = compose(x, 3000, 128)
    got = whisper.span_windows([flat(x, 1)], 3000, 128)
    assert got.shape == (1, 3000, 128)
    check(got[0], exp, "W = 3000, n = 720000")
    short = whisper.span_windows([flat(x[:48000], 1)], 3000, 128)  # a 2 s utterance: everything past frame 201 is the floor
    check(short[0], compose(x[:48000], 3000, 128)[0], "W = 3000, n = 48000")
    assert float(short[0, 202:].min()) == float(short[0, 202:].max())


def test_log_mel_spectrogram_keeps_the_bits_it_had():
    """The frame body moved into a __device__ function that both kernels call.  The pin holds what kk_op_log_mel gave BEFORE that: a digest of the raw
    float32 bytes of four clips (tests/golden/whisper_logmel_pin.json), next to the float64 restatement's error bar of test_gpu_whisper_logmel.py."""
    import hashlib

    pin = json.load(open(PIN))
    assert len(pin["cases"]) == 4
    for c in pin["cases"]:
        x = R.signal(c["n"], c["seed"])
        g = whisper.log_mel_spectrogram(x, c["n_mels"], c["padding"]).cpu().numpy()
        ref = R.log_mel(x, c["n_mels"], c["padding"])
        assert float(np.abs(g.astype(np.float64) - ref).max()) < 1e-3
        assert hashlib.sha256(np.ascontiguousarray(g).tobytes()).hexdigest() == c["sha256"], c
