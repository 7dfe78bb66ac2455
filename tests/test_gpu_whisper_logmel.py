"""The log-mel front end on the device (kk_op_log_mel, csrc/kk_whisper.hip; mlx-audio_amd/whisper.py) against the float64
restatement tests/_whisper_ref.py:log_mel.

The error bar is not a constant: the yardstick is the SAME restatement run in float32 with a direct DFT (frames32 @ cos32, no FFT) against the
float64 one, pooled over all the cases, and the kernel's maximum error may be 4 x that: its summation order and its log10 differ from
numpy's, which is the margin of two extra roundings in each of two stages.  Both figures are computed and printed every run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _whisper_ref as R  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = [201, 400, 1599, 1600, 1601, 16007]


def test_log_mel_against_the_float64_restatement():
    cases = [(n, p, m) for p in (0, 1600) for m in (80, 128) for n in LENGTHS] + [(whisper.N_SAMPLES, 0, 128)]
    clips = {n: R.signal(n, 900 + n % 977) for n in set(c[0] for c in cases)}
    yard = kern = 0.0
    for p in (0, 1600):
        for m in (80, 128):
            got = whisper.log_mel_spectrogram([clips[n] for n in LENGTHS], m, p)  # one ragged launch
            assert isinstance(got, list) and len(got) == len(LENGTHS)
            for n, g in zip(LENGTHS, got):
                ref = R.log_mel(clips[n], m, p)
                y = float(np.abs(R.log_mel(clips[n], m, p, dtype=np.float32).astype(np.float64) - ref).max())
                assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == ((n + p) // 160, m) == ref.shape
                e = float(np.abs(g.cpu().numpy().astype(np.float64) - ref).max())
                print(f"n {n:6d} padding {p:4d} n_mels {m:3d}: kernel {e:.3e}  float32 restatement {y:.3e}")
                yard, kern = max(yard, y), max(kern, e)
    n, p, m = cases[-1]  # 30 s, a single run
    ref = R.log_mel(clips[n], m, p)
    y = float(np.abs(R.log_mel(clips[n], m, p, dtype=np.float32).astype(np.float64) - ref).max())
    g = whisper.log_mel_spectrogram(torch.from_numpy(clips[n]).cuda(), m, p)  # a device tensor
    assert tuple(g.shape) == (whisper.N_FRAMES, m)
    e = float(np.abs(g.cpu().numpy().astype(np.float64) - ref).max())
    print(f"n {n:6d} padding {p:4d} n_mels {m:3d}: kernel {e:.3e}  float32 restatement {y:.3e}")
    yard, kern = max(yard, y), max(kern, e)
    print(f"pooled: kernel max error {kern:.3e}, float32 restatement {yard:.3e}, bar 4 x = {4 * yard:.3e}")
    assert kern <= 4 * yard


@pytest.mark.parametrize("n_mels", [80, 128])
def test_all_zero_clip_is_exactly_minus_one_and_a_half(n_mels):
    g = whisper.log_mel_spectrogram(np.zeros(4000, np.float32), n_mels, 160)
    assert tuple(g.shape) == (26, n_mels) and bool((g == -1.5).all())


def test_ragged_batch_rows_are_bit_equal_to_each_row_alone():
    lengths = [16007, 1601, 400]
    ldx = 16007 + 333
    x = torch.full((3, ldx), float("nan"), dtype=torch.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = torch.from_numpy(R.signal(n, 40 + b))
    x = x.cuda()
    out = whisper.log_mel_rows(x, lengths, 80, 0)
    assert tuple(out.shape) == (3, 100, 80) and not bool(torch.isnan(out).any())  # the NaN tails are never read
    for b, n in enumerate(lengths):
        F = n // 160
        alone = whisper.log_mel_spectrogram(x[b, :n].clone(), 80, 0)
        assert torch.equal(out[b, :F], alone), f"row {b}"
        assert bool((out[b, F:] == 0).all()), f"row {b}: rows past its frames must be zero"
        assert float(np.abs(alone.cpu().numpy() - R.log_mel(x[b, :n].cpu().numpy(), 80, 0)).max()) < 1e-3
