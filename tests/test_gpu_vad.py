"""The row-mode voice-activity detector on the device (kk_vad.hip, mlx-audio_amd/vad.py) against tests/_vad_ref.py.

Energies: one wave's fixed order -- ceil(frame_len / 64) fmaf per lane, then six butterfly additions -- over non-negative terms, so the
relative error against the float64 sum is at most (ceil(frame_len / 64) + 7) 2^-24: one rounding per fmaf, one per addition, one to spare
for the second-order terms.  Derived, not measured; the observed maximum is printed.
Flags and status: clips of noise frames whose rms is one of {0, 0.003, 0.015, 0.06, 0.3} against the threshold 0.03, so every frame is a
factor of 2 or more away from the threshold (a factor of 4 in energy, against an error of 1e-5): the kernel's rule and the reference's float64
rule must agree on every frame.
Row mode: status and energies are bit-equal to the whole-clip `kk_op_vad`, whatever the slicing and the neighbours."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _vad_ref as V  # noqa: E402

from mlx_audio_amd import vad  # noqa: E402
from mlx_audio_amd._lib import KokoroHipError  # noqa: E402

pytestmark = pytest.mark.gpu

RATE = 1000  # frame_ms milliseconds are frame_ms samples


def _cfg(frame_len, threshold=0.03, hang=3):
    """A config whose frame is `frame_len` samples at RATE and whose hang is `hang` frames."""
    cfg = vad.VadConfig(frame_ms=frame_len, threshold=threshold, silence_ms=hang * frame_len)
    assert cfg.frame_len(RATE) == frame_len and cfg.hang_frames == hang
    return cfg


def _detect(x, cfg):
    """-> (status (classified, onset, last_speech, endpoint), energies of the classified frames as float32 numpy)"""
    o, s, e, start, stop, en = vad.detect(torch.from_numpy(np.ascontiguousarray(x)), cfg, RATE, energy=True)
    nf = x.shape[0] // cfg.frame_len(RATE)
    classified = e + 1 if e >= 0 else nf
    en = en.cpu().numpy()
    assert en.shape == (nf,) and not en[classified:].any()  # nothing behind an endpoint is classified
    return (classified, o, s, e), en[:classified], (start, stop)


# ---- energies -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", [1, 63, 64, 65, 100, 720, 4096])
def test_energy_against_the_float64_sum(fl):
    g = np.random.default_rng(700 + fl)
    nf = 9 if fl < 4096 else 5
    x = (0.3 * g.standard_normal(nf * fl + fl // 2)).astype(np.float32)  # (a partial last frame: never classified)
    x[:fl] *= 1e-3  # a quiet frame and a loud one
    x[fl : 2 * fl] *= 30
    status, en, _ = _detect(x, _cfg(fl, threshold=0.0))  # threshold 0: every frame is speech, no endpoint
    assert status == (nf, 0, nf - 1, -1)
    want = V.energies(x, fl)
    assert want.shape == (nf,) and (want > 0).all()
    rel = np.abs(en.astype(np.float64) - want) / want
    bound = (math.ceil(fl / 64) + 7) * 2.0 ** -24
    print(f"frame_len {fl}: max relative error {rel.max():.3e}, bound {bound:.3e}")
    assert rel.max() <= bound


# ---- flags and status ---------------------------------------------------------------------------------------------------------------------
LEVELS = [0, 0.003, 0.015, 0.06, 0.3]


@pytest.mark.parametrize("fl,hang,seed", [(720, 3, 1), (65, 2, 2), (100, 0, 3), (63, 5, 4), (720, 50, 5)])
def test_flags_and_status_equal_the_reference(fl, hang, seed):
    g = np.random.default_rng(seed)
    nf = 90 if hang < 50 else 140
    rms = g.choice(LEVELS, size=nf, p=[0.3, 0.15, 0.2, 0.2, 0.15]).tolist()
    if hang == 50:  # the default hang: a long pause that does not end the row, then one that does
        rms[:10] = [0.0, 0.003, 0.3, 0.06] + [0.06] * 6
        rms[10:60] = [0.0] * 50
        rms[60:62] = [0.06, 0.3]
        rms[62:] = [0.003] * (nf - 62)
    x = V.noise_clip(g, fl, rms)
    cfg = _cfg(fl, 0.03, hang)
    flags, want = V.machine(x, fl, 0.03, hang)
    status, en, sp = _detect(x, cfg)
    assert status == want
    got = (en >= cfg.thr2n(RATE)).tolist()  # the kernel's comparison on the kernel's energies: every frame, none excluded
    assert got == flags == [r >= 0.03 for r in rms[: len(flags)]]
    assert sp == (V.span(want, x.shape[0], fl, 0, None, hang) or (0, 0))
    if hang == 50:
        assert want == (113, 2, 61, 112)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def _layout(frames, fl=8):
    """frames: per frame 'S' (speech: constant 0.5), 0 (zeros), 'nan' or 'inf' (one such sample in a speech frame)"""
    x = np.zeros(len(frames) * fl, np.float32)
    for f, k in enumerate(frames):
        if k != 0:
            x[f * fl : (f + 1) * fl] = 0.5
        if k in ("nan", "inf"):
            x[f * fl + fl // 2] = float(k)
    return x


@pytest.mark.parametrize("name,frames,hang,want", [
    ("speech from frame 0", ["S", "S", 0, 0], 3, (4, 0, 1, -1)),
    ("silence only", [0] * 7, 3, (7, -1, -1, -1)),
    ("hang silent frames: the endpoint is missed by one frame", [0, "S", 0, 0, 0, "S", 0], 3, (7, 1, 5, -1)),
    ("hang + 1 silent frames end the row", [0, "S", 0, 0, 0, 0, "S", "S"], 3, (6, 1, 1, 5)),
    ("hang 0", ["S", 0, "S"], 0, (2, 0, 0, 1)),
    ("a NaN frame is silence, an inf frame is speech", ["S", "nan", "S", 0, 0, "inf", 0, 0, 0, 0, "S"], 2, (9, 0, 5, 8)),
    ("NaN frames count towards the endpoint", ["S", "nan", "nan", "S"], 1, (3, 0, 0, 2)),
])
def test_layouts(name, frames, hang, want):
    x = _layout(frames)
    status, en, _ = _detect(x, _cfg(8, 0.03, hang))
    assert status == want, name
    assert V.machine(x, 8, 0.03, hang)[1] == want  # (the reference restatement says the same)
    assert len(en) == want[0]


@pytest.mark.parametrize("hang,want", [(1029, (1100, 0, 1030, -1)), (1027, (1029, 0, 0, 1028)), (1022, (1024, 0, 0, 1023)), (1023, (1025, 0, 0, 1024))])
def test_1100_frames_cross_the_lds_batch(hang, want):
    frames = [0] * 1100
    frames[0] = frames[1030] = "S"
    x = _layout(frames)
    status, en, _ = _detect(x, _cfg(8, 0.03, hang))
    assert status == want
    assert V.machine(x, 8, 0.03, hang)[1] == want
    np.testing.assert_array_equal(en, V.energies(x, 8)[: want[0]].astype(np.float32))  # (8 samples of 0.25: exact)


# ---- row mode -----------------------------------------------------------------------------------------------------------------------------
ROWS = [dict(fl=720, thr=0.03, hang=9, start=0), dict(fl=65, thr=0.1, hang=1, start=2), dict(fl=100, thr=0.01, hang=0, start=5)]


def _row_clip(g, r, nf):
    lv = [0.0, r["thr"] / 10, r["thr"] / 2, r["thr"] * 2, r["thr"] * 10]
    rms = g.choice(lv, size=nf, p=[0.15, 0.1, 0.15, 0.3, 0.3]).tolist()
    rms[0] = 0.0
    x = V.noise_clip(g, r["fl"], rms)
    return np.concatenate([x, (0.2 * g.standard_normal(r["fl"] // 3)).astype(np.float32)])  # a partial last frame


def test_row_mode_is_bit_equal_to_the_whole_clip():
    g = np.random.default_rng(77)
    dev = torch.device("cuda")
    clips = [_row_clip(g, ROWS[0], 9), _row_clip(g, ROWS[1], 60), _row_clip(g, ROWS[2], 45)]
    W = max(c.shape[0] for c in clips) + 4
    buf = torch.full((4, W), float("nan"), dtype=torch.float32, device=dev)  # row 3 never gets a stream: it sits out with NaN in its buffer
    rv = vad.RowVad(4, device=dev)
    cfgs = [_cfg(r["fl"], r["thr"], r["hang"]) for r in ROWS]
    whole = [_detect(c, cfg) for c, cfg in zip(clips, cfgs)]
    assert any(w[0][3] >= 0 for w in whole) and any(w[0][3] < 0 for w in whole)  # a row that ends early and one that never does
    fed, got_e, ended_at = [0, 0, 0], [[], [], []], [None] * 3
    step = 0
    while any(fed[b] < clips[b].shape[0] for b in range(3)):
        before = rv.status.cpu().numpy().copy()
        for b, r in enumerate(ROWS):
            if step == r["start"]:
                rv.set_row(b, r["fl"], cfgs[b].thr2n(RATE), r["hang"])
            if step >= r["start"] and fed[b] < clips[b].shape[0]:
                sizes = [1, r["fl"] - 1, r["fl"], r["fl"] + 1, 1000]
                k = min(sizes[(step - r["start"]) % 5], clips[b].shape[0] - fed[b])
                buf[b, fed[b] : fed[b] + k] = torch.from_numpy(clips[b][fed[b] : fed[b] + k]).to(dev)  # what lies behind stays NaN
                fed[b] += k
        mirror = [st[1] if st is not None else 0 for st in rv._rows]
        e = rv.step(buf, fed + [0], energy=True).cpu().numpy()
        now = rv.status.cpu().numpy()
        for b, r in enumerate(ROWS):
            if step < r["start"]:
                assert now[b].tolist() == [0, -1, -1, -1]
                continue
            new = fed[b] // r["fl"] - mirror[b]
            got_e[b] += e[b, :new].tolist()
            if ended_at[b] is not None:  # a row past its endpoint is unchanged by later steps, and writes no energy
                assert now[b].tolist() == before[b].tolist() and not e[b].any()
            elif now[b][3] >= 0:
                ended_at[b] = step
        assert now[3].tolist() == [0, -1, -1, -1]
        step += 1
    final = rv.status.cpu().numpy()
    for b in range(3):
        status, en, _ = whole[b]
        assert tuple(final[b].tolist()) == status
        np.testing.assert_array_equal(np.array(got_e[b][: status[0]], np.float32).view(np.uint32), en.view(np.uint32))
    assert any(ended_at[b] is not None and fed[b] > (whole[b][0][3] + 2) * ROWS[b]["fl"] for b in range(3))  # steps did follow an endpoint
    # set_row restarts a row without touching the others
    keep = final.copy()
    clip = V.noise_clip(g, 80, [0, 0.2, 0.001, 0.3, 0.001])
    cfg = _cfg(80, 0.02, 1)
    rv.set_row(1, 80, cfg.thr2n(RATE), 1)
    now = rv.status.cpu().numpy()
    assert now[1].tolist() == [0, -1, -1, -1] and (now[[0, 2, 3]] == keep[[0, 2, 3]]).all()
    buf[1].fill_(float("nan"))
    buf[1, : clip.shape[0]] = torch.from_numpy(clip).to(dev)
    e = rv.step(buf, [fed[0], clip.shape[0], fed[2], 0], energy=True).cpu().numpy()
    status, en, _ = _detect(clip, cfg)
    now = rv.status.cpu().numpy()
    assert tuple(now[1].tolist()) == status and (now[[0, 2, 3]] == keep[[0, 2, 3]]).all()
    np.testing.assert_array_equal(e[1, : status[0]].view(np.uint32), en.view(np.uint32))
    rv.close()
    with pytest.raises(KokoroHipError, match="closed"):
        rv.step(buf, [0, 0, 0, 0])


def test_host_refusals_leave_everything_as_it_was():
    dev = torch.device("cuda")
    rv = vad.RowVad(2, device=dev)
    x = torch.zeros((2, 64), dtype=torch.float32, device=dev)
    x[0, 8:16] = 0.5
    rv.set_row(0, 8, 0.03 * 0.03 * 8, 1)
    rv.step(x, [24, 0])
    want = rv.status.cpu().numpy().copy()
    assert want.tolist() == [[3, 1, 1, -1], [0, -1, -1, -1]]

    def same():
        torch.cuda.synchronize()
        return (rv.status.cpu().numpy() == want).all()

    for row in (-1, 2):
        with pytest.raises(KokoroHipError, match="row"):
            rv.set_row(row, 8, 0.1, 1)
    for fl in (0, 4097, -8):
        with pytest.raises(KokoroHipError, match="frame_len"):
            rv.set_row(0, fl, 0.1, 1)
    with pytest.raises(KokoroHipError, match="hang_frames"):
        rv.set_row(0, 8, 0.1, -1)
    for thr in (-1.0, float("inf"), float("nan")):
        with pytest.raises(KokoroHipError, match="thr2n"):
            rv.set_row(0, 8, thr, 1)
    assert same()
    with pytest.raises(KokoroHipError, match="previous"):
        rv.step(x, [23, 0])
    with pytest.raises(KokoroHipError, match="previous"):
        rv.step(x, [-1, 0])
    with pytest.raises(KokoroHipError, match="in a row of 64"):
        rv.step(x, [65, 0])
    assert same()
    # an energy row too short for the step's new frames: 5 new frames, room for 4 (the wrapper sizes it itself, so through the library)
    e = torch.zeros((2, 4), dtype=torch.float32, device=dev)
    n = (C.c_int32 * 2)(64, 0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = rv.lib.kk_vad_step(rv._h, st, C.c_void_p(x.data_ptr()), 64, C.cast(n, C.c_void_p), C.c_void_p(rv.status.data_ptr()), C.c_void_p(e.data_ptr()), 4)
    assert rc != 0 and b"energy rows hold 4" in rv.lib.kk_last_error()
    assert same() and not e.any()
    # nothing was changed: the row goes on from frame 3 as if no refused call had been made
    en = rv.step(x, [64, 0], energy=True).cpu().numpy()
    assert rv.status.cpu().numpy().tolist() == [[4, 1, 1, 3], [0, -1, -1, -1]] and en.shape == (2, 5) and not en.any()
    with pytest.raises(ValueError):
        rv.step(x[:, ::2], [64, 0])  # not contiguous
    with pytest.raises(KokoroHipError, match="max_rows"):
        vad.RowVad(65, device=dev)
    rv.close()
