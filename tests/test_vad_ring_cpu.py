"""`vad.utterances`, the host-side definition of what the ring detector reports (mlx-audio_amd/vad.py), against the restated
reference loop of tests/_vad_ring_ref.py on energy sequences, and the arithmetic of the upload gate (`keep_from`, `ring_max_frames`) against
brute force on small numbers.  No device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _vad_ring_ref as R  # noqa: E402

from mlx_audio_amd import vad  # noqa: E402

RATE = 1000


def _cfg(fl=8, hang=2, pre=0, keep=None, thr=0.5):
    cfg = vad.VadConfig(frame_ms=fl, threshold=thr, silence_ms=hang * fl, pre_roll_ms=pre, keep_silence_ms=keep)
    assert cfg.frame_len(RATE) == fl and cfg.hang_frames == hang and cfg.pre_roll(RATE) == pre
    return cfg


S, Q = 100.0, 0.0  # a speech and a silent energy against thr2n = 0.25 * 8 = 2

CASES = [
    ("several utterances", [Q, S, S, Q, Q, Q, Q, S, Q, S, Q, Q, Q, Q, Q, S], 2, None,
     [(1, 2, 5, 0), (7, 9, 12, 0)], (16, 2, 15, 15)),
    ("one that begins on the frame after an endpoint", [S, Q, Q, S, S, Q, Q], 1, None, [(0, 0, 2, 0), (3, 4, 6, 0)], (7, 2, -1, -1)),
    ("hang 0, alternating frames", [S, Q] * 5, 0, None, [(2 * k, 2 * k, 2 * k + 1, 0) for k in range(5)], (10, 5, -1, -1)),
    ("a forced close followed at once by a new onset", [Q, S, S, S, S, S, Q, Q], 1, 3, [(1, 3, 3, 1), (4, 5, 6, 1)], (8, 2, -1, -1)),
    ("a forced close on a silent frame inside the hang", [S, Q, Q, S], 5, 3, [(0, 0, 2, 1)], (4, 1, 3, 3)),
    ("the hang wins over max_frames on the same frame", [S, Q, Q, S], 1, 3, [(0, 0, 2, 0)], (4, 1, 3, 3)),
    ("max_frames 1: every speech frame is an utterance", [S, S, Q, S], 3, 1, [(0, 0, 0, 1), (1, 1, 1, 1), (3, 3, 3, 1)], (4, 3, -1, -1)),
    ("silence only", [Q] * 9, 2, None, [], (9, 0, -1, -1)),
    ("NaN is silence, inf is speech", [S, float("nan"), float("nan"), float("inf"), Q, Q], 1, None, [(0, 0, 2, 0), (3, 3, 5, 0)], (6, 2, -1, -1)),
]


@pytest.mark.parametrize("name,e,hang,mx,records,status", CASES, ids=[c[0] for c in CASES])
def test_utterances_on_energy_sequences(name, e, hang, mx, records, status):
    cfg = _cfg(8, hang)
    got = vad.utterances(cfg, np.array(e), RATE, mx, energies=True)
    assert got == (records, status)
    assert R.machine_energies(e, float(cfg.thr2n(RATE)), hang, mx) == (records, status)  # (the restated loop says the same)


def test_utterances_on_random_sequences_and_on_samples():
    g = np.random.default_rng(5)
    for trial in range(60):
        hang, mx = int(g.integers(0, 4)), (None if trial % 3 == 0 else int(g.integers(1, 9)))
        e = g.choice([Q, S, float("nan")], size=int(g.integers(1, 80)), p=[0.5, 0.4, 0.1])
        cfg = _cfg(8, hang)
        assert vad.utterances(cfg, e, RATE, mx, energies=True) == R.machine_energies(e, float(cfg.thr2n(RATE)), hang, mx)
    # on samples: frames of noise a factor 2 away from the threshold, a partial last frame never classified
    rms = g.choice([0, 0.003, 0.015, 0.06, 0.3], size=70).tolist()
    x = np.concatenate([R.noise_clip(g, 65, rms), np.full(30, 0.9, np.float32)])
    cfg = _cfg(65, 2, thr=0.03)
    flags, records, status = R.machine(x, 65, 0.03, 2, 7)
    assert flags == [r >= 0.03 for r in rms] and len(records) >= 3
    assert vad.utterances(cfg, x, RATE, 7) == (records, status)
    with pytest.raises(ValueError):
        vad.utterances(cfg, x, RATE, 0)


def test_a_record_goes_through_span():
    for pre, keep in [(0, None), (5, None), (20, 3), (0, 0)]:
        cfg = _cfg(8, 2, pre, keep)
        for rec in [(0, 0, 3, 0), (4, 6, 9, 0), (4, 9, 9, 1), (2, 3, 4, 1)]:
            assert vad.span(cfg, vad.record_status(rec), 10 ** 9, False, RATE) == R.span(rec, 8, pre, keep, 2)
            assert vad.span(cfg, vad.record_status(rec), 0, True, RATE) == R.span(rec, 8, pre, keep, 2)  # a closed record needs no n
        for st, n in [((7, 1, 5, 6), 61), ((7, 0, 5, 5), 48), ((7, 0, -1, -1), 60)]:
            assert vad.span(cfg, (st[0], st[2], st[3], -1), n, True, RATE) == R.open_span(st, n, 8, pre, keep, 2)


def test_gate_arithmetic_against_brute_force():
    """keep_from is the smallest position anything still to come can ask for; with max_frames = ring_max_frames every span fits the ring
    from its start, and an upload that stays below keep_from + ring_len never overwrites a position that is still needed."""
    for fl, pre, frames in [(4, 0, 3), (4, 3, 3), (4, 9, 4), (5, 7, 2), (1, 0, 1), (3, 2, 5)]:
        cfg = _cfg(fl, 1, pre)
        ring_len = pre + frames * fl + (fl - 1)  # (not a multiple of the frame)
        mx = vad.ring_max_frames(cfg, RATE, ring_len)
        assert mx == max(m for m in range(1, 100) if pre + m * fl <= ring_len) == frames
        for c in range(0, 12):
            # every utterance that may still be reported has its onset at a frame >= c: the smallest start among them
            future = min(max(0, o * fl - pre) for o in range(c, c + 40))
            assert vad.keep_from(cfg, RATE, c, None) == future
            for oldest in (0, 1, future - 1, future, future + 3):
                if oldest >= 0:
                    assert vad.keep_from(cfg, RATE, c, oldest) == min(oldest, future)
        # every span of at most mx frames: stop - start <= ring_len, whatever the onset and the keep
        for o in range(0, 10):
            for e in range(o, o + mx):
                for s in range(o, e + 1):
                    a, b = vad.span(cfg, vad.record_status((o, s, e, 0)), 10 ** 9, False, RATE)
                    assert 0 <= a <= b and b - a <= ring_len
    with pytest.raises(ValueError):
        vad.ring_max_frames(_cfg(4, 1, 9), RATE, 12)
