"""Reference for the voice-activity detector (mlx-audio_amd/vad.py, kk_vad.hip): float64 frame energies, the reference's silence rule and its
listener loop restated from mlx_audio/sts/voice_pipeline.py:86-158, and the status -> samples arithmetic.  numpy only; nothing of the package."""
import math

import numpy as np


def frames_until_silence(silence_duration, frame_duration_ms):
    """voice_pipeline.py:123-125"""
    return int(silence_duration * 1000 / frame_duration_ms)


def energies(x, frame_len):
    """float64 sum of squares of every whole frame"""
    x = np.asarray(x, np.float64)
    nf = x.shape[0] // frame_len
    return (x[: nf * frame_len].reshape(nf, frame_len) ** 2).sum(axis=1)


def is_silent(frame, threshold):
    """voice_pipeline.py:86-99 on float samples: norm / sqrt(size) < threshold, in float64.  (A NaN compares false there too, which would
    read as speech; `machine` takes the rule of the kernel's documentation for non-finite energies: NaN is silence, inf is speech.)"""
    frame = np.asarray(frame, np.float64)
    with np.errstate(all="ignore"):
        energy = math.sqrt(float((frame ** 2).sum()) / frame.size)
    if math.isnan(energy):
        return True
    return energy < threshold


def machine(x, frame_len, threshold, hang):
    """The loop of voice_pipeline.py:121-158 over the whole frames of x, stopped at the first endpoint.
    -> (flags of the frames classified, (classified, onset, last_speech, endpoint))."""
    x = np.asarray(x)
    nf = x.shape[0] // frame_len
    speaking_detected, silent_frames = False, 0
    onset = last = end = -1
    flags = []
    f = 0
    while f < nf and end < 0:
        is_speech = not is_silent(x[f * frame_len : (f + 1) * frame_len], threshold)
        flags.append(is_speech)
        if is_speech:
            speaking_detected, silent_frames, last = True, 0, f
            if onset < 0:
                onset = f
        elif speaking_detected:
            silent_frames += 1
            if silent_frames > hang:
                end = f
        f += 1
    return flags, (f, onset, last, end)


def span(status, n, frame_len, pre_roll, keep, hang):
    """(start, stop) in samples of an ENDED stream of n samples, None without an onset.  keep None: every frame up to the endpoint frame."""
    _, o, s, e = status
    if o < 0:
        return None
    if keep is None:
        keep = (hang + 1) * frame_len
    return max(0, o * frame_len - pre_roll), min((s + 1) * frame_len + keep, (e + 1) * frame_len if e >= 0 else n)


def noise_clip(g, frame_len, rms_per_frame):
    """One noise frame per entry, scaled to exactly that rms (in float64, then rounded to float32); 0 is digital silence."""
    out = np.zeros(len(rms_per_frame) * frame_len, np.float32)
    for f, r in enumerate(rms_per_frame):
        if r == 0:
            continue
        v = g.standard_normal(frame_len)
        if frame_len == 1:
            v = np.ones(1)
        v *= r / math.sqrt(float((v ** 2).sum()) / frame_len)
        out[f * frame_len : (f + 1) * frame_len] = v.astype(np.float32)
    return out
