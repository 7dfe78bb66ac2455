"""Reference for the re-arming voice-activity detector (mlx-audio_amd/vad.py RingVad and utterances, kk_vad.hip): the listener loop of
mlx_audio/sts/voice_pipeline.py:108-165 restated WITH the reset it does behind an utterance (frames, speaking_detected and silent_frames
cleared; the `while True` goes on), the forced close that keeps an utterance inside the encoder's capacity, float64 frame energies and the
record -> samples arithmetic.  numpy only; nothing of the package."""
import math

import numpy as np

from _vad_ref import energies, is_silent, noise_clip  # noqa: F401  (the one-shot reference's pieces that do not change)

FORCED = 1


def machine_energies(e, thr2, hang, max_frames=None):
    """The loop over per-frame energies e (float64; speech iff e >= thr2, NaN is silence).
    -> (records [(onset, last_speech, endpoint, flags)], (classified, closed, onset, last_speech) with the open utterance or -1, -1)."""
    records = []
    speaking_detected, silent_frames = False, 0
    onset = last = -1
    for f, v in enumerate(np.asarray(e, np.float64).tolist()):
        is_speech = (not math.isnan(v)) and v >= thr2
        closed = None
        if is_speech:
            speaking_detected, silent_frames, last = True, 0, f
            if onset < 0:
                onset = f
        elif speaking_detected:
            silent_frames += 1
            if silent_frames > hang:
                closed = 0
        if closed is None and speaking_detected and max_frames is not None and f - onset + 1 == max_frames:
            closed = FORCED
        if closed is not None:
            records.append((onset, last, f, closed))
            speaking_detected, silent_frames, onset, last = False, 0, -1, -1  # voice_pipeline.py:156-158: the reset, and the loop goes on
    return records, (len(e), len(records), onset, last)


def machine(x, frame_len, threshold, hang, max_frames=None):
    """The loop over the whole frames of x with the reference's own rule per frame (rms < threshold is silence, in float64)."""
    x = np.asarray(x)
    nf = x.shape[0] // frame_len
    flags = [not is_silent(x[f * frame_len : (f + 1) * frame_len], threshold) for f in range(nf)]
    records, status = machine_energies([1.0 if s else 0.0 for s in flags], 0.5, hang, max_frames)
    return flags, records, status


def span(record, frame_len, pre_roll, keep, hang):
    """(start, stop) in samples of a closed record.  keep None: every frame up to the endpoint frame."""
    o, s, e = record[:3]
    if keep is None:
        keep = (hang + 1) * frame_len
    return max(0, o * frame_len - pre_roll), min((s + 1) * frame_len + keep, (e + 1) * frame_len)


def open_span(status, n, frame_len, pre_roll, keep, hang):
    """(start, stop) of the utterance still open when a stream of n samples ends; None without one."""
    _, _, o, s = status
    if o < 0:
        return None
    if keep is None:
        keep = (hang + 1) * frame_len
    return max(0, o * frame_len - pre_roll), min((s + 1) * frame_len + keep, n)
