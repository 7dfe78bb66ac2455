"""The re-arming voice-activity detector over a ring on the device (kk_vad_ring in kk_vad.hip, vad.RingVad).

Energies: bit-equal to the flat detector (`vad.detect(..., energy=True)`) on the same stream laid out flat -- only the address is taken
modulo the ring -- and, as in test_gpu_vad.py, within (ceil(frame_len / 64) + 7) 2^-24 relative of the float64 sum: one rounding per fmaf,
one per butterfly addition, one to spare.  Derived, not measured; the observed maximum is printed.
Status and log: against tests/_vad_ring_ref.py on streams of 5 ring lengths of noise frames whose rms is one of {0, 0.003, 0.015, 0.06, 0.3}
against 0.03: every frame is a factor 4 in energy away from the threshold, so fp32 and float64 agree on every frame and none is excluded."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _vad_ring_ref as R  # noqa: E402

from mlx_audio_amd import vad  # noqa: E402
from mlx_audio_amd._lib import KokoroHipError  # noqa: E402

pytestmark = pytest.mark.gpu

RATE = 1000
BIG = 1 << 40  # a max_frames no test reaches
LEVELS = [0, 0.003, 0.015, 0.06, 0.3]


def _cfg(frame_len, threshold=0.03, hang=3):
    cfg = vad.VadConfig(frame_ms=frame_len, threshold=threshold, silence_ms=hang * frame_len)
    assert cfg.frame_len(RATE) == frame_len and cfg.hang_frames == hang
    return cfg


class Mic:
    """One row's stream, its ring on the host (numpy modulo indexing) and what the test has consumed of the row's log."""

    def __init__(self, x, fl, ring_len, sizes):
        self.x, self.fl, self.ring_len, self.sizes = x, fl, ring_len, sizes
        self.n = self.k = 0
        self.acked, self.records = 0, []

    def feed(self, ring_row):
        """The next slice, cut so that no position is overwritten before a step has seen it -> the new n_avail."""
        room = (self.n // self.fl) * self.fl + self.ring_len - self.n
        k = min(self.sizes[self.k % len(self.sizes)], self.x.shape[0] - self.n, room)
        self.k += 1
        idx = (self.n + np.arange(k)) % self.ring_len
        ring_row[idx] = self.x[self.n : self.n + k]
        self.n += k
        return self.n

    def consume(self, status, log):
        """Take the new records out of the log, as a host that acks everything it has seen."""
        closed = int(status[1])
        assert 0 <= closed - self.acked <= vad.RING_LOG
        for r in range(self.acked, closed):
            self.records.append(tuple(int(v) for v in log[r % vad.RING_LOG]))
        self.acked = closed


@pytest.mark.parametrize("fl", [1, 63, 64, 65, 100, 720, 4096])
@pytest.mark.parametrize("smallest", [False, True], ids=["ring 10.3 frames", "ring == frame"])
def test_energies_are_the_flat_detectors_bits(fl, smallest):
    g = np.random.default_rng(900 + fl)
    ring_len = fl if smallest else 10 * fl + max(1, (3 * fl) // 10)  # 1030 for a frame of 100: never a multiple of the frame but at 1
    nf = 5 if smallest else 52  # the stream is 5 ring lengths
    x = (0.3 * g.standard_normal(nf * fl + fl // 2)).astype(np.float32)  # (a partial last frame: never classified)
    x[:fl] *= 1e-3
    x[fl : 2 * fl] *= 30
    cfg = _cfg(fl, threshold=0.0)  # every frame is speech, nothing closes
    dev = torch.device("cuda")
    flat = vad.detect(torch.from_numpy(x), cfg, RATE, energy=True)
    assert flat[:3] == (0, nf - 1, -1)
    want32 = flat[5].cpu().numpy()
    rv = vad.RingVad(1, device=dev)
    rv.set_row(0, fl, cfg.thr2n(RATE), cfg.hang_frames, BIG, ring_len)
    W = ring_len + 5  # the row is wider than the ring: nothing behind ring_len is read
    host = np.full((1, W), np.nan, np.float32)
    en = torch.zeros((1, nf), dtype=torch.float32, device=dev)
    mic = Mic(x, fl, ring_len, [3 * fl + 1, 1, fl - 1 or 1, 1000, 7 * fl])
    steps = 0
    while mic.n < x.shape[0]:
        n = mic.feed(host[0])
        rv.step(torch.from_numpy(host).to(dev), [n], [0], energy=en)
        steps += 1
    assert steps >= 5
    st = rv.status.cpu().numpy()[0].tolist()
    assert st == [nf, 0, 0, nf - 1]
    got = en.cpu().numpy()[0]
    np.testing.assert_array_equal(got.view(np.uint32), want32.view(np.uint32))
    want = R.energies(x, fl)
    rel = np.abs(got.astype(np.float64) - want) / want
    bound = (math.ceil(fl / 64) + 7) * 2.0 ** -24
    print(f"frame_len {fl} ring_len {ring_len}: max relative error {rel.max():.3e}, bound {bound:.3e}")
    assert rel.max() <= bound
    rv.close()


ROWS = [dict(fl=720, hang=2, ring=7 * 720 + 130, mx=6), dict(fl=65, hang=1, ring=13 * 65 + 7, mx=BIG), dict(fl=100, hang=0, ring=1030, mx=2)]


def test_status_and_log_equal_the_reference_whatever_the_slicing():
    dev = torch.device("cuda")
    mics, want = [], []
    for b, r in enumerate(ROWS):
        g = np.random.default_rng(3 + b)
        nf = 5 * r["ring"] // r["fl"] + 1
        rms = g.choice(LEVELS, size=nf, p=[0.3, 0.15, 0.2, 0.2, 0.15]).tolist()
        x = np.concatenate([R.noise_clip(g, r["fl"], rms), (0.2 * g.standard_normal(r["fl"] // 3)).astype(np.float32)])
        assert x.shape[0] >= 5 * r["ring"]
        flags, records, status = R.machine(x, r["fl"], 0.03, r["hang"], None if r["mx"] == BIG else r["mx"])
        assert flags == [v >= 0.03 for v in rms] and len(records) >= 3
        want.append((records, status))
        mics.append(Mic(x, r["fl"], r["ring"], [1, r["fl"] - 1, r["fl"], r["fl"] + 1, 1000]))
    for b in (0, 2):  # forced closes are among them, and closes by the hang
        assert {rec[3] for rec in want[b][0]} == {0, 1}
    W = max(r["ring"] for r in ROWS) + 4
    host = np.full((5, W), np.nan, np.float32)  # row 3: a stream of NaN; row 4 never gets a stream and sits out with NaN in its buffer
    rv = vad.RingVad(5, device=dev)
    for b, r in enumerate(ROWS):
        rv.set_row(b, r["fl"], _cfg(r["fl"], 0.03, r["hang"]).thr2n(RATE), r["hang"], r["mx"], r["ring"])
    rv.set_row(3, 8, 0.1, 1, BIG, 64)
    n3 = 0
    while any(m.n < m.x.shape[0] for m in mics):
        n = [m.feed(host[b]) for b, m in enumerate(mics)]
        n3 = min(n3 + 40, (n3 // 8) * 8 + 64)
        rv.step(torch.from_numpy(host).to(dev), n + [n3, -(1 << 62)], [m.acked for m in mics] + [0, 1 << 62])
        status, log = rv.fetch().take()
        for b, m in enumerate(mics):
            m.consume(status[b], log[b])
            # what the status shows of the open utterance is the reference's on the frames classified so far
            c = int(status[b][0])
            assert c == m.n // m.fl  # (the host acks at once, so the walk never stalls here)
        assert status[3].tolist() == [n3 // 8, 0, -1, -1] and status[4].tolist() == [0, 0, -1, -1]
    for b, m in enumerate(mics):
        records, st = want[b]
        assert m.records == records
        assert tuple(int(v) for v in rv.status.cpu().numpy()[b]) == st
    rv.close()
    with pytest.raises(KokoroHipError, match="closed"):
        rv.step(torch.from_numpy(host).to(dev), [0] * 5, [0] * 5)


def _layout(frames, fl=8):
    x = np.zeros(len(frames) * fl, np.float32)
    for f, k in enumerate(frames):
        if k:
            x[f * fl : (f + 1) * fl] = 0.5
    return x


def test_the_walk_stalls_at_the_log_and_resumes_after_the_ack():
    dev = torch.device("cuda")
    fl, ring = 8, 40 * 8 + 3
    x = _layout([1, 0] * 20)
    _, records, final = R.machine(x, fl, 0.03, 0)
    assert records == [(2 * k, 2 * k, 2 * k + 1, 0) for k in range(20)] and final == (40, 20, -1, -1)
    buf = torch.zeros((1, ring), dtype=torch.float32, device=dev)
    buf[0, : x.shape[0]] = torch.from_numpy(x).to(dev)
    rv = vad.RingVad(1, device=dev)
    rv.set_row(0, fl, _cfg(fl, 0.03, 0).thr2n(RATE), 0, BIG, ring)
    got, acked = [], 0
    for want in [(16, 8, -1, -1), (32, 16, -1, -1), (40, 20, -1, -1)]:
        rv.step(buf, [x.shape[0]], [acked])  # all 40 frames in the first step; the later ones only carry the ack
        status, log = rv.fetch().take()
        assert tuple(status[0].tolist()) == want
        if acked == 0:  # a step with neither a new frame nor a new ack changes nothing
            rv.step(buf, [x.shape[0]], [0])
            again, log2 = rv.fetch().take()
            assert (again == status).all() and (log2 == log).all()
        got += [tuple(log[0][r % vad.RING_LOG].tolist()) for r in range(acked, int(status[0][1]))]
        acked = int(status[0][1])
    assert got == records
    rv.close()


def test_a_forced_close_rearms_on_the_next_frame():
    dev = torch.device("cuda")
    fl, ring = 8, 19
    x = _layout([1] * 7 + [0, 0])
    _, records, final = R.machine(x, fl, 0.03, 5, 3)
    assert records == [(0, 2, 2, 1), (3, 5, 5, 1), (6, 6, 8, 1)] and final == (9, 3, -1, -1)
    rv = vad.RingVad(2, device=dev)
    rv.set_row(1, fl, _cfg(fl, 0.03, 5).thr2n(RATE), 5, 3, ring)
    host = np.zeros((2, 24), np.float32)
    mic = Mic(x, fl, ring, [19, 11, 16, 100])
    while mic.n < x.shape[0]:
        n = mic.feed(host[1])
        rv.step(torch.from_numpy(host).to(dev), [0, n], [0, mic.acked])
        status, log = rv.fetch().take()
        mic.consume(status[1], log[1])
    assert mic.records == records and tuple(status[1].tolist()) == final and status[0].tolist() == [0, 0, -1, -1]
    rv.close()


def test_host_refusals_leave_everything_as_it_was():
    dev = torch.device("cuda")
    rv = vad.RingVad(2, device=dev)
    x = torch.zeros((2, 64), dtype=torch.float32, device=dev)
    x[0, 8:16] = 0.5
    thr = 0.03 * 0.03 * 8
    rv.set_row(0, 8, thr, 0, BIG, 48)
    rv.step(x, [24, 0], [0, 0])
    want = rv._table.cpu().numpy().copy()
    assert want[:8].tolist() == [3, 1, -1, -1, 0, 0, -1, -1] and want[8:12].tolist() == [1, 1, 2, 0]

    def same():
        torch.cuda.synchronize()
        return (rv._table.cpu().numpy() == want).all()

    for row in (-1, 2):
        with pytest.raises(KokoroHipError, match="row"):
            rv.set_row(row, 8, 0.1, 1, BIG, 48)
    for fl in (0, 4097, -8):
        with pytest.raises(KokoroHipError, match="frame_len"):
            rv.set_row(0, fl, 0.1, 1, BIG, 8192)
    with pytest.raises(KokoroHipError, match="hang_frames"):
        rv.set_row(0, 8, 0.1, -1, BIG, 48)
    for mx in (0, -3):
        with pytest.raises(KokoroHipError, match="max_frames"):
            rv.set_row(0, 8, 0.1, 1, mx, 48)
    for t in (-1.0, float("inf"), float("nan")):
        with pytest.raises(KokoroHipError, match="thr2n"):
            rv.set_row(0, 8, t, 1, BIG, 48)
    with pytest.raises(KokoroHipError, match="ring_len"):
        rv.set_row(0, 8, 0.1, 1, BIG, 7)
    assert same()
    with pytest.raises(KokoroHipError, match="previous"):
        rv.step(x, [23, 0], [0, 0])
    with pytest.raises(KokoroHipError, match="previous"):
        rv.step(x, [-1, 0], [0, 0])
    with pytest.raises(KokoroHipError, match="overwritten position 24"):
        rv.step(x, [24 + 49, 0], [0, 0])  # frames 0..2 were handed out: position 24 is the oldest unseen one
    with pytest.raises(KokoroHipError, match="handed out"):
        rv.step(x, [24, 0], [4, 0])
    with pytest.raises(KokoroHipError, match="a ring of 48 in a row of 32"):
        rv.step(x[:, :32].contiguous(), [24, 0], [0, 0])
    assert same()
    rv.step(x, [24, 0], [1, 0])
    with pytest.raises(KokoroHipError, match="below its previous 1"):
        rv.step(x, [24, 0], [0, 0])
    assert same()
    # nothing was changed: the row goes on from frame 3, into the ring's second lap
    x[0, 24:32] = 0.5
    x[0, 0:8] = 0.25  # positions 48..55
    rv.step(x, [56, 0], [1, 0])
    status, log = rv.fetch().take()
    assert status.tolist() == [[7, 2, 6, 6], [0, 0, -1, -1]] and log[0][1].tolist() == [3, 3, 4, 0]
    with pytest.raises(ValueError):
        rv.step(x[:, ::2], [56, 0], [1, 0])  # not contiguous
    with pytest.raises(KokoroHipError, match="max_rows"):
        vad.RingVad(65, device=dev)
    rv.close()
