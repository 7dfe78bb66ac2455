"""The row-mode streaming Mimi ENCODER (Mimi.row_encoder on kk_mimi_stream_create_rows_encoder / kk_mimi_encode_step_rows): every row has its
own position and lifetime.  The contract is integer identity: a row that starts at any step, sits out any steps and is fed any step sizes
carries the codes of a fresh batch-1 `Mimi.encode_step` stream fed the same pcm in the same step sizes (array equality).  Against
MimiStreamOracle the `downsampled` activations meet the bar test_gpu_mimi.py sets for this path, rel_max < 2e-4; no code-agreement ratio is
asserted here (the batch-1 stream is pinned against the oracle there)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import mimi_oracle as M  # noqa: E402
import mlx_audio_amd.params as P  # noqa: E402
from _attn_ref import check_bits  # noqa: E402
from _util import err_stats, report  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_FRAMES = 48


def _setup(which, seed=5, encode=True):
    from mlx_audio_amd.mimi import Mimi, MimiConfig

    cfg = P.mimi_tiny_config() if which == "tiny" else P.mimi_config(32)
    w = P.mimi_synth_checkpoint(cfg, seed, encode=True) if encode else P.mimi_synth_checkpoint(cfg, seed)
    model = Mimi(MimiConfig.from_dict(cfg), w)
    spf = int(np.prod(cfg["ratios"])) * cfg["upsample_stride"]
    return cfg, w, model, spf


def _pcm(rng, frames, spf):
    return (rng.standard_normal(frames * spf) * 0.3).astype(np.float32)


def _solo(model, pcm, steps, spf, context=None):
    """A fresh batch-1 Mimi.encode_step stream over pcm [T * spf] in the given step sizes -> codes [nq, T]."""
    from mlx_audio_amd import _lib

    model.close_stream()
    with torch.cuda.device(model.device):
        st = model._open_stream("enc", True, 1, max(steps), 1, MAX_FRAMES, max(steps))
    if context is not None:
        _lib.check(model.lib.kk_mimi_stream_set_context(st["h"], context), "set_context")
    out, i = [], 0
    for F in steps:
        out.append(model.encode_step(torch.tensor(pcm[None, None, i * spf : (i + F) * spf]), max_chunk=max(steps)).cpu().numpy()[0])
        i += F
    assert i * spf == pcm.shape[0]
    model.close_stream()
    return np.concatenate(out, -1)


def _run(enc, model, schedule, pcm, fed=None, junk=np.nan, fetch=False):
    """schedule: [(F, rows active)]; pcm[row] [T * spf]: the row's stream, consumed in order.  Returns per row its code pieces, step sizes
    and (fetch) the `downsampled` rows of its steps.  Inactive rows' pcm entries are `junk`: the library may not depend on them."""
    B, spf = enc.max_batch, enc.spf
    fed = fed if fed is not None else {r: 0 for r in range(B)}
    codes = {r: [] for r in range(B)}
    steps = {r: [] for r in range(B)}
    down = {r: [] for r in range(B)}
    for F, rows in schedule:
        blk = np.full((B, 1, F * spf), junk, np.float32)
        for r in rows:
            blk[r, 0] = pcm[r][fed[r] * spf : (fed[r] + F) * spf]
        got = enc.step(torch.tensor(blk), [r in rows for r in range(B)]).cpu().numpy()
        assert got.shape == (B, model.cfg.nq, F)
        xd = model.debug_fetch("downsampled").cpu().numpy() if fetch else None
        for r in rows:
            assert (got[r] >= 0).all() and (got[r] < model.cfg.bins).all()
            codes[r].append(got[r])
            steps[r].append(F)
            if fetch:
                down[r].append(xd[r])
            fed[r] += F
    return codes, steps, fed, down


SCHEDULE = [(3, [0, 3]), (3, [0, 1, 3]), (3, [0, 1, 2, 3]), (2, [0, 2]), (3, [1, 3]), (1, [1]), (3, [3])]


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
def test_rows_started_at_different_steps_equal_their_solo_streams(which):
    """Four rows that start at different steps (row 2 while rows 0, 1 and 3 are mid-stream: what one `fresh` flag for all rows gets wrong in
    both directions), with NaN and then 1e30 in the inactive rows' pcm slots."""
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(41)
    total = {r: sum(F for F, rows in SCHEDULE if r in rows) for r in range(4)}
    pcm = {r: _pcm(rng, total[r], spf) for r in range(4)}
    want = None
    for junk in (np.nan, 1e30):
        enc = model.row_encoder(4, MAX_FRAMES, 3)
        codes, steps, fed, _ = _run(enc, model, SCHEDULE, pcm, junk=junk)
        assert steps == {0: [3, 3, 3, 2], 1: [3, 3, 3, 1], 2: [3, 2], 3: [3, 3, 3, 3, 3]}
        assert [enc.row_frames(r) for r in range(4)] == [total[r] for r in range(4)]
        if want is None:
            want = {r: _solo(model, pcm[r], steps[r], spf) for r in range(4)}  # (computed once, shared by both runs)
        for r in range(4):
            np.testing.assert_array_equal(np.concatenate(codes[r], -1), want[r], err_msg=f"row {r}, junk {junk}")
        if which == "tiny":  # the codes recorded before the stream-state kernels got their shared bodies
            check_bits("mimi_rows_encode/codes/tiny", *[np.concatenate(codes[r], -1).astype(np.int32) for r in range(4)])
        enc.close()


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
def test_active_rows_match_the_stream_oracle(which):
    """The `downsampled` rows of every active row and step against MimiStreamOracle.encode_step run per row with the same steps."""
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(42)
    total = {r: sum(F for F, rows in SCHEDULE if r in rows) for r in range(4)}
    pcm = {r: _pcm(rng, total[r], spf) for r in range(4)}
    enc = model.row_encoder(4, MAX_FRAMES, 3)
    codes, steps, fed, down = _run(enc, model, SCHEDULE, pcm, junk=np.nan, fetch=True)
    worst = 0.0
    for r in range(4):
        orc, i = M.MimiStreamOracle(w, cfg), 0
        for k, F in enumerate(steps[r]):
            _, inter = orc.encode_step(pcm[r][None, None, i * spf : (i + F) * spf], return_inter=True)
            e = err_stats(down[r][k], np.transpose(inter["downsampled"], (0, 2, 1))[0])
            print(f"row {r} step {k} F {F}: rel_max {e['rel_max']:.3e}")
            worst = max(worst, e["rel_max"])
            assert e["rel_max"] < 2e-4, (r, k, F, e)
            i += F
    report(f"mimi/rows_encode/{which}", worst_rel=worst)
    enc.close()


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
def test_an_inactive_row_is_inert(which):
    """Row 1 sits out two steps with non-finite pcm in its slot: its position, carried rows and K / V keep their bits, and its stream goes on as
    if nothing had happened.  The snapshot of an encoder stream holds sum(S * C) carried floats and the K / V of the ENCODER's layers."""
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(43)
    pcm = {0: _pcm(rng, 8, spf), 1: _pcm(rng, 7, spf)}
    enc = model.row_encoder(2, MAX_FRAMES, 2)
    c1, s1, fed, _ = _run(enc, model, [(2, [0, 1]), (2, [0, 1])], pcm)
    pos, snap = enc.snapshot(1)
    us, D = cfg["upsample_stride"], cfg["dim"]
    assert pos == 4 * us and np.abs(snap).max() > 0
    # carried rows (kk_mimi.hip stream_layout, encoder): init conv k - 1 x 1; per layer the residual block's k_r - 1 rows and the strided
    # conv's k - stride = ratio rows at the layer's width; last conv; resampler us rows of dim
    carried, ch = (cfg["ksize"] - 1) * 1, cfg["nfilters"]
    for ratio in reversed(cfg["ratios"]):
        carried += (cfg["residual_ksize"] - 1) * ch + ratio * ch
        ch *= 2
    carried += (cfg["last_ksize"] - 1) * ch + us * D
    assert snap.size == carried + 2 * cfg["num_layers"] * pos * D
    for junk in (np.nan, np.inf):
        c2, s2, fed, _ = _run(enc, model, [(2, [0])], pcm, fed=fed, junk=junk)
        c1[0] += c2[0]; s1[0] += s2[0]
        pos2, snap2 = enc.snapshot(1)
        assert pos2 == pos and enc.row_frames(1) == 4
        np.testing.assert_array_equal(snap2, snap)
    c3, s3, fed, _ = _run(enc, model, [(2, [1]), (1, [1])], pcm, fed=fed, junk=-1e30)
    c1[1] += c3[1]; s1[1] += s3[1]
    for r in (0, 1):
        np.testing.assert_array_equal(np.concatenate(c1[r], -1), _solo(model, pcm[r], s1[r], spf), err_msg=f"row {r}")
    enc.close()


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
@pytest.mark.parametrize("first", [1, 3])
def test_reset_row_restarts_one_row_and_touches_no_other(which, first):
    """The reset row's first step (F = 1 / F = 3) gets the resampler's edge fill from its NEW first row; rows 0 and 2 never notice."""
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(44)
    pcm = {r: _pcm(rng, 4 + first + 2, spf) for r in range(3)}
    enc = model.row_encoder(3, MAX_FRAMES, 3)
    ca, sa, fed, _ = _run(enc, model, [(2, [0, 1, 2]), (2, [0, 1, 2])], pcm)
    before = {r: enc.snapshot(r) for r in (0, 2)}
    enc.reset_row(1)
    for r in (0, 2):
        pos, snap = enc.snapshot(r)
        assert pos == before[r][0]
        np.testing.assert_array_equal(snap, before[r][1])
    pos1, snap1 = enc.snapshot(1)
    assert pos1 == 0 and enc.row_frames(1) == 0 and not snap1.any()
    new1 = _pcm(rng, first + 2, spf)
    pcm2 = {0: pcm[0], 1: np.concatenate([np.zeros(4 * spf, np.float32), new1]), 2: pcm[2]}  # (row 1's cursor stands at 4)
    cb, sb, fed, _ = _run(enc, model, [(first, [0, 1, 2]), (2, [0, 1, 2])], pcm2, fed=fed)
    for r in (0, 2):
        np.testing.assert_array_equal(np.concatenate(ca[r] + cb[r], -1), _solo(model, pcm[r], [2, 2, first, 2], spf), err_msg=f"row {r}")
    np.testing.assert_array_equal(np.concatenate(ca[1], -1), _solo(model, pcm[1][: 4 * spf], [2, 2], spf))
    np.testing.assert_array_equal(np.concatenate(cb[1], -1), _solo(model, new1, [first, 2], spf), err_msg="row 1 after its reset")
    enc.close()


def test_rows_with_different_key_windows():
    """Tiny codec, context 5 (odd: the window's edge falls inside a frame at upsample_stride 2): rows at positions below, at and above the
    context equal their solo streams with the same context."""
    cfg, w, model, spf = _setup("tiny")
    us = cfg["upsample_stride"]
    rng = np.random.default_rng(45)
    schedule = [(2, [0])] * 4 + [(2, [0, 1]), (1, [0, 1, 2]), (2, [0, 1, 2]), (2, [0, 1, 2])]
    total = {r: sum(F for F, rows in schedule if r in rows) for r in range(3)}
    pcm = {r: _pcm(rng, total[r], spf) for r in range(3)}
    enc = model.row_encoder(3, MAX_FRAMES, 2)
    enc.set_context(5)
    codes, steps, fed, _ = _run(enc, model, schedule, pcm)
    assert [enc.snapshot(r)[0] for r in range(3)] == [total[r] * us for r in range(3)]
    assert total[0] * us > 5 and any(sum(steps[1][:k]) * us < 5 < sum(steps[1][: k + 1]) * us for k in range(len(steps[1])))
    for r in range(3):
        got = np.concatenate(codes[r], -1)
        np.testing.assert_array_equal(got, _solo(model, pcm[r], steps[r], spf, context=5), err_msg=f"row {r}")
    assert (np.concatenate(codes[0], -1) != _solo(model, pcm[0], steps[0], spf)).any()  # (the short context is not vacuous)
    from mlx_audio_amd._lib import KokoroHipError

    with pytest.raises(KokoroHipError, match="fresh"):
        enc.set_context(8)  # only while every row is fresh
    enc.close()


def test_refusals_happen_on_the_host():
    """A row past max_frames, F = 0, F > max_chunk, a bad shape, the three cross-direction calls, 65 rows and a checkpoint without encoder
    parameters are refused before any launch; the stream is left as it was."""
    import ctypes as C

    from mlx_audio_amd._lib import KokoroHipError

    cfg, w, model, spf = _setup("tiny")
    rng = np.random.default_rng(46)
    enc = model.row_encoder(2, 4, 2)
    p2 = torch.tensor((rng.standard_normal((2, 1, 2 * spf)) * 0.3).astype(np.float32))
    with pytest.raises(KokoroHipError, match="frames per step"):
        enc.step(torch.zeros((2, 1, 3 * spf)), [True, True])
    with pytest.raises(ValueError):
        enc.step(torch.zeros((2, 1, 0)), [True, True])  # F = 0
    with pytest.raises(ValueError):
        enc.step(p2[:, :, : spf + 5], [True, True])  # a partial frame
    with pytest.raises(ValueError):
        enc.step(p2[:1], [True])
    with pytest.raises(ValueError):
        enc.step(p2, [True])
    for row in (-1, 2, 99):
        with pytest.raises(KokoroHipError, match="row out of range"):
            enc.reset_row(row)
        with pytest.raises(ValueError):
            enc.row_frames(row)
    # F = 0 at the library's own entry
    ws, out, act = enc._ws, torch.zeros((2, cfg["nq"], 2), dtype=torch.int32, device=model.device), (C.c_int32 * 2)(1, 1)
    pd = p2.to(model.device).reshape(2, -1).contiguous()
    args = (C.c_void_p(pd.data_ptr()), act, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(out.data_ptr()))
    assert model.lib.kk_mimi_encode_step_rows(enc._h, enc._stream(), 0, *args) != 0
    first = enc.step(p2, [True, False]).cpu().numpy()
    enc.step(p2, [True, False])
    assert [enc.row_frames(r) for r in (0, 1)] == [4, 0]
    with pytest.raises(KokoroHipError, match="would hold 6 frames"):
        enc.step(p2, [True, True])
    assert [enc.row_frames(r) for r in (0, 1)] == [4, 0] and enc.snapshot(0)[0] == 4 * cfg["upsample_stride"]
    # the three cross-direction calls
    dec = model.row_decoder(2, 4, 2)
    codes = torch.zeros((2, cfg["nq"], 2), dtype=torch.int32, device=model.device)
    pcm_out = torch.zeros((2, 2 * spf), dtype=torch.float32, device=model.device)
    rc = model.lib.kk_mimi_decode_step_rows(enc._h, enc._stream(), 2, C.c_void_p(codes.data_ptr()), act, C.c_void_p(ws.data_ptr()), ws.numel(),
                                            C.c_void_p(pcm_out.data_ptr()))
    assert rc != 0 and b"other direction" in model.lib.kk_last_error()
    rc = model.lib.kk_mimi_encode_step_rows(dec._h, enc._stream(), 2, C.c_void_p(pd.data_ptr()), act, C.c_void_p(dec._ws.data_ptr()), dec._ws.numel(),
                                            C.c_void_p(out.data_ptr()))
    assert rc != 0 and b"other direction" in model.lib.kk_last_error()
    rc = model.lib.kk_mimi_encode_step(enc._h, enc._stream(), 2, C.c_void_p(pd.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(out.data_ptr()))
    assert rc != 0 and b"row-mode" in model.lib.kk_last_error()
    assert [enc.row_frames(r) for r in (0, 1)] == [4, 0] and [dec.row_frames(r) for r in (0, 1)] == [0, 0]
    dec.close()
    # the full row rides along inactive while the other one runs; once reset it starts over with the same codes as its first stream
    enc.step(p2, [False, True])
    enc.reset_row(0)
    again = enc.step(p2, [True, False]).cpu().numpy()
    np.testing.assert_array_equal(again[0], first[0])
    with pytest.raises(KokoroHipError, match="64 rows"):
        model.row_encoder(65, 4, 2)
    with pytest.raises(KokoroHipError):
        model.row_encoder(2, 4, 5)  # max_chunk > max_frames
    enc.close()
    with pytest.raises(KokoroHipError, match="closed"):
        enc.step(p2, [True, False])
    _, _, plain, _ = _setup("tiny", encode=False)
    with pytest.raises(KokoroHipError, match="no encoder"):
        plain.row_encoder(2, 4, 2)
