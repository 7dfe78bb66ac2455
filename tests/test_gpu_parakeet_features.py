"""Parakeet's log-mel features on the device (parakeet.log_mel_spectrogram, kk_op_parakeet_log_mel, csrc/kk_parakeet.hip) against the float64
restatement tests/_parakeet_ref.py:log_mel.  The yardstick, as in test_gpu_whisper_logmel.py, is the SAME restatement run in float32 with a direct DFT, pooled
over the cases; the kernel's maximum error may be 4 x that.  Both figures are printed.  n_fft 512, a 400-sample window zero-padded at its end, hop 160."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _parakeet_ref as R  # noqa: E402

from mlx_audio_amd import parakeet  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS = [400, 1599, 1601, 16007]


def test_log_mel_against_the_float64_restatement():
    cases = [(n, m, norm, 0) for n in LENGTHS for m in (80, 128) for norm in ("per_feature", "all_features")] + [(1599, 80, "per_feature", 2400)]
    yard = kern = 0.0
    for n, m, norm, pad_to in cases:
        x = R.signal(n, 900 + n % 977)
        args = parakeet.PreprocessArgs(sample_rate=16000, normalize=norm, window_size=0.025, window_stride=0.01, window="hann", features=m, n_fft=512,
                                       dither=1e-5, pad_to=pad_to, pad_value=0.0)
        a = (x, 16000, 512, 400, 160, m, norm == "per_feature", pad_to, 0.0)
        ref = R.log_mel(*a)
        y = float(np.abs(R.log_mel(*a, dtype=np.float32).astype(np.float64) - ref).max())
        got = parakeet.log_mel_spectrogram(x, args)
        assert tuple(got.shape) == (1, 1 + max(n, pad_to) // 160, m) == (1,) + ref.shape
        e = float(np.abs(got[0].cpu().numpy().astype(np.float64) - ref).max())
        print(f"n {n:6d} features {m:3d} {norm:12s} pad_to {pad_to:4d}: kernel {e:.3e}  float32 restatement {y:.3e}")
        yard, kern = max(yard, y), max(kern, e)
    print(f"pooled: kernel max error {kern:.3e}, float32 restatement {yard:.3e}, bar 4 x = {4 * yard:.3e}")
    assert kern <= 4 * yard
