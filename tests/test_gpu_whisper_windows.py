"""kk_op_mel_windows / whisper.mel_windows on the device (csrc/kk_whisper.hip): the windows of a transcription round, cut out of whole-file
spectrograms in one launch, are bit-equal to slicing and zero-padding in torch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

from mlx_audio_amd import whisper  # noqa: E402


def _want(mels, seeks, sizes, W):
    import torch

    out = torch.zeros((len(mels), W, mels[0].shape[1]), dtype=torch.float32, device=mels[0].device)
    for r, (m, s, n) in enumerate(zip(mels, seeks, sizes)):
        out[r, :n] = m[s:s + n]
    return out


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("W", [200, 3000])
def test_windows_are_slices_then_zeros(n_mels, W):
    import torch

    g = torch.Generator().manual_seed(n_mels + W)
    # files of different lengths in memory of their own; the third is a view into a larger batch, as log_mel_spectrogram hands them out
    files = [torch.randn((W + 37, n_mels), generator=g).cuda(), torch.randn((3 * W + 1, n_mels), generator=g).cuda(),
             torch.randn((2, 2 * W, n_mels), generator=g).cuda()[1, : W + 5], torch.randn((1, n_mels), generator=g).cuda()]
    a, b, c, e = files
    cases = [([a], [0], [W]),                                           # R = 1, a whole window from the start
             ([b], [W + 3], [1]), ([b], [5], [0]),                      # one frame from the middle; nothing at all
             ([a, b, c, e, b], [37, 2 * W + 1, 5, 0, W - 1], [W, W, W, 1, W - 1]),  # R = 5: tails that end on the file's last frame, one source twice
             ([c, a, b, b, e], [0, 36, 3 * W, 0, 1], [W - 7, 1, 0, W, 0])]          # sizes W, 1 and 0 mixed; an empty window at the very end
    for mels, seeks, sizes in cases:
        got = whisper.mel_windows(mels, seeks, sizes, W)
        torch.cuda.synchronize()
        assert got.shape == (len(mels), W, n_mels) and got.dtype == torch.float32
        assert torch.equal(got, _want(mels, seeks, sizes, W)), (seeks, sizes)
    # NaN behind a window's frames is never read into it
    poisoned = torch.full((W + 10, n_mels), float("nan"), device="cuda")
    poisoned[3:8] = 1.5
    got = whisper.mel_windows([poisoned], [3], [5], W)
    assert torch.equal(got[0, :5], poisoned[3:8]) and not got.isnan().any() and float(got[0, 5:].abs().max()) == 0.0


def test_the_wrapper_refuses_what_the_kernel_must_not_see():
    import torch

    m = torch.zeros((300, 80), device="cuda")
    for args, msg in [(([m], [101], [200], 200), "frames 101 .. 301 of 300"), (([m], [0], [201], 200), "W = 200"), (([m], [-1], [5], 200), "frames -1"),
                      (([m] * 33, [0] * 33, [1] * 33, 200), "1 .. 32"), (([m, m], [0], [1, 1], 200), "one seek and one size"),
                      (([m.cpu()], [0], [1], 200), "on one device"), (([m.double()], [0], [1], 200), "fp32"), (([m[:, :40]], [0], [1], 200), "contiguous")]:
        with pytest.raises(ValueError, match=msg):
            whisper.mel_windows(*args)
