"""`vad.VadConfig` and `vad.span` without a device: the config's arithmetic against the reference's own expressions
(mlx_audio/sts/voice_pipeline.py:109, 123-125, 149) and the status -> samples arithmetic against tests/_vad_ref.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _vad_ref as V  # noqa: E402

from mlx_audio_amd.vad import VadConfig, span  # noqa: E402


def test_defaults_are_the_references_and_the_endpoint_falls_on_the_51st_silent_frame():
    cfg = VadConfig()
    assert (cfg.frame_ms, cfg.threshold, cfg.silence_ms, cfg.pre_roll_ms, cfg.keep_silence_ms) == (30, 0.03, 1500, 0, None)
    assert cfg.hang_frames == V.frames_until_silence(1.5, 30) == 50
    for rate in (8000, 16000, 24000, 44100):
        assert cfg.frame_len(rate) == int(rate * (30 / 1000.0)) == rate * 30 // 1000
    assert cfg.frame_len(24000) == 720
    assert cfg.thr2n(24000) == np.float32(0.03 * 0.03 * 720) and cfg.thr2n(24000).dtype == np.float32
    # one speech frame, then silence: the reference's loop ends the utterance at the 51st silent frame
    fl = 4
    x = np.concatenate([np.ones(fl, np.float32), np.zeros(60 * fl, np.float32)])
    flags, status = V.machine(x, fl, cfg.threshold, cfg.hang_frames)
    assert status == (52, 0, 0, 51) and flags == [True] + [False] * 51
    _, status = V.machine(x[: 51 * fl], fl, cfg.threshold, cfg.hang_frames)  # 50 silent frames: not yet
    assert status == (51, 0, 0, -1)
    assert VadConfig(silence_ms=300).hang_frames == 10 and VadConfig(silence_ms=100).hang_frames == 3 and VadConfig(silence_ms=0).hang_frames == 0


def test_config_refusals():
    with pytest.raises(ValueError, match="4096"):
        VadConfig(frame_ms=200).frame_len(24000)  # 4800 samples
    with pytest.raises(ValueError, match="4096"):
        VadConfig(frame_ms=1).frame_len(500)      # 0 samples
    assert VadConfig(frame_ms=170).frame_len(24000) == 4080
    for bad in (dict(frame_ms=0), dict(frame_ms=2.5), dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold=float("inf")),
                dict(silence_ms=-1), dict(pre_roll_ms=-1), dict(keep_silence_ms=-1)):
        with pytest.raises(ValueError):
            VadConfig(**bad)


RATE = 1000  # 30 samples per frame


def _both(cfg, status, n):
    fl = cfg.frame_len(RATE)
    keep = None if cfg.keep_silence_ms is None else cfg.keep(RATE)
    want = V.span(status, n, fl, cfg.pre_roll(RATE), keep, cfg.hang_frames)
    assert span(cfg, status, n, True, rate=RATE) == want
    return want


def test_span():
    cfg = VadConfig(silence_ms=90)  # hang 3, 30 samples per frame
    assert cfg.frame_len(RATE) == 30 and cfg.hang_frames == 3 and cfg.keep(RATE) == 120
    assert _both(cfg, (10, -1, -1, -1), 317) is None                   # no onset
    assert _both(cfg, (10, 2, 8, -1), 317) == (60, 317)                # no endpoint: the ended stream's partial last frame is silence, kept
    assert _both(cfg, (10, 2, 4, -1), 317) == (60, 270)                # ... unless the kept silence ends before it
    assert _both(cfg, (9, 2, 4, 8), 317) == (60, 270)                  # endpoint: every frame up to the endpoint frame
    assert _both(VadConfig(silence_ms=90, pre_roll_ms=45), (9, 2, 4, 8), 317) == (15, 270)
    assert _both(VadConfig(silence_ms=90, pre_roll_ms=100), (9, 2, 4, 8), 317) == (0, 270)     # a pre-roll clipped at 0
    assert _both(VadConfig(silence_ms=90, keep_silence_ms=40), (9, 2, 4, 8), 317) == (60, 190)  # keep shorter than the hang
    assert _both(VadConfig(silence_ms=90, keep_silence_ms=500), (9, 2, 4, 8), 317) == (60, 270)  # keep longer than the hang: the endpoint frame bounds it
    assert _both(VadConfig(silence_ms=90, keep_silence_ms=0), (9, 2, 4, 8), 317) == (60, 150)
    # an open stream without an endpoint: only what is certain so far
    assert span(cfg, (6, 2, 4, -1), 200, False, rate=RATE) == (60, 180)
    assert span(cfg, (10, 2, 4, -1), 317, False, rate=RATE) == (60, 270)
    assert span(cfg, (6, -1, -1, -1), 200, False, rate=RATE) is None
