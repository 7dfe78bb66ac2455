"""The row-mode streaming Mimi decoder (Mimi.row_decoder on kk_mimi_stream_create_rows / kk_mimi_decode_step_rows / kk_mimi_stream_reset_row):
every row has its own position and lifetime.  The contract is bit identity: a row that starts at any step, sits out any steps and is fed any
step sizes carries the pcm of a fresh batch-1 `Mimi.decode_step` stream fed the same codes in the same step sizes (array equality, no
tolerance); against MimiStreamOracle the bar is the one test_gpu_mimi.py uses, max_abs <= 1e-3 * max(1, ref_max)."""
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


def _setup(which, seed=5):
    from mlx_audio_amd.mimi import Mimi, MimiConfig

    cfg = P.mimi_tiny_config() if which == "tiny" else P.mimi_config(32)
    w = P.mimi_synth_checkpoint(cfg, seed)
    model = Mimi(MimiConfig.from_dict(cfg), w)
    spf = int(np.prod(cfg["ratios"])) * cfg["upsample_stride"]
    return cfg, w, model, spf


def _solo(model, codes, steps, context=None):
    """A fresh batch-1 Mimi.decode_step stream over codes [nq, T] in the given step sizes -> pcm [T * spf]."""
    from mlx_audio_amd import _lib

    model.close_stream()
    with torch.cuda.device(model.device):
        st = model._open_stream("dec", False, 1, max(steps), 1, MAX_FRAMES, max(steps))
    if context is not None:
        _lib.check(model.lib.kk_mimi_stream_set_context(st["h"], context), "set_context")
    out, i = [], 0
    for F in steps:
        out.append(model.decode_step(torch.tensor(codes[None, :, i : i + F]), max_chunk=max(steps)).cpu().numpy()[0, 0])
        i += F
    assert i == codes.shape[1]
    model.close_stream()
    return np.concatenate(out)


def _oracle(w, cfg, codes, steps, context=250):
    orc = M.MimiStreamOracle(w, cfg, context=context)
    out, i = [], 0
    for F in steps:
        out.append(orc.decode_step(codes[None, :, i : i + F])[0, 0])
        i += F
    return np.concatenate(out)


def _run(dec, cfg, schedule, codes, fed=None, junk=None):
    """schedule: [(F, rows active)]; codes[row] [nq, T]: the row's stream, consumed in order.  Returns per row its pcm pieces and step sizes.
    Inactive rows' code entries are `junk` (any int: the library may not depend on them)."""
    B, nq = dec.max_batch, cfg["nq"]
    fed = fed if fed is not None else {r: 0 for r in range(B)}
    pcm = {r: [] for r in range(B)}
    steps = {r: [] for r in range(B)}
    for F, rows in schedule:
        blk = np.full((B, nq, F), 0 if junk is None else junk, np.int64)
        for r in rows:
            blk[r] = codes[r][:, fed[r] : fed[r] + F]
        got = dec.step(torch.tensor(blk), [r in rows for r in range(B)]).cpu().numpy()
        assert got.shape == (B, 1, F * dec.spf) and np.isfinite(got).all()
        for r in rows:
            pcm[r].append(got[r, 0])
            steps[r].append(F)
            fed[r] += F
            assert dec.row_frames(r) >= F
    return pcm, steps, fed


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
def test_rows_started_at_different_steps_equal_their_solo_streams_and_the_oracle(which):
    """B = 4 rows that start at different steps, run different step sizes (N = 3 and tails of 2 and 1) and end at different steps."""
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(31)
    schedule = [(3, [0, 3]), (3, [0, 1, 3]), (3, [0, 1, 2, 3]), (2, [0, 2]), (3, [1, 3]), (1, [1]), (3, [3])]
    total = {r: sum(F for F, rows in schedule if r in rows) for r in range(4)}
    codes = {r: rng.integers(0, cfg["bins"], (cfg["nq"], total[r])) for r in range(4)}
    dec = model.row_decoder(4, MAX_FRAMES, 3)
    pcm, steps, fed = _run(dec, cfg, schedule, codes, junk=cfg["bins"] + 7)
    assert steps == {0: [3, 3, 3, 2], 1: [3, 3, 3, 1], 2: [3, 2], 3: [3, 3, 3, 3, 3]}
    assert [dec.row_frames(r) for r in range(4)] == [total[r] for r in range(4)]
    worst = 0.0
    for r in range(4):
        got = np.concatenate(pcm[r])
        np.testing.assert_array_equal(got, _solo(model, codes[r], steps[r]), err_msg=f"row {r}")
        e = err_stats(got, _oracle(w, cfg, codes[r], steps[r]))
        worst = max(worst, e["max_abs"] / max(1.0, e["ref_max"]))
        assert e["max_abs"] <= 1e-3 * max(1.0, e["ref_max"]), (r, e)
    report(f"mimi/rows/{which}", worst_rel=worst)
    if which == "tiny":  # the pcm bits recorded before the stream-state kernels got their shared bodies
        check_bits("mimi_rows/decode_pcm/tiny", *[np.concatenate(pcm[r]).astype(np.float32) for r in range(4)])
    dec.close()


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
def test_an_inactive_row_is_inert(which):
    """Row 1 sits out two steps with out-of-range codes in its slot: its carried state, its K / V below its position and its position keep
    their bits, and its stream goes on as if nothing had happened."""
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(32)
    codes = {0: rng.integers(0, cfg["bins"], (cfg["nq"], 8)), 1: rng.integers(0, cfg["bins"], (cfg["nq"], 7))}
    dec = model.row_decoder(2, MAX_FRAMES, 2)
    p1, s1, fed = _run(dec, cfg, [(2, [0, 1]), (2, [0, 1])], codes)
    pos, snap = dec.snapshot(1)
    assert pos == 4 * cfg["upsample_stride"] and snap.size > 0 and np.abs(snap).max() > 0
    for junk in (-5, 10 ** 6):
        p2, s2, fed = _run(dec, cfg, [(2, [0])], codes, fed=fed, junk=junk)
        p1[0] += p2[0]; s1[0] += s2[0]
        pos2, snap2 = dec.snapshot(1)
        assert pos2 == pos and dec.row_frames(1) == 4
        np.testing.assert_array_equal(snap2, snap)
    p3, s3, fed = _run(dec, cfg, [(2, [1]), (1, [1])], codes, fed=fed, junk=-1)
    p1[1] += p3[1]; s1[1] += s3[1]
    for r in (0, 1):
        np.testing.assert_array_equal(np.concatenate(p1[r]), _solo(model, codes[r], s1[r]), err_msg=f"row {r}")
    dec.close()


@pytest.mark.parametrize("which", ["tiny", "mimi_202407"])
def test_reset_row_restarts_one_row_and_touches_no_other(which):
    cfg, w, model, spf = _setup(which)
    rng = np.random.default_rng(33)
    codes = {r: rng.integers(0, cfg["bins"], (cfg["nq"], 8)) for r in range(3)}
    dec = model.row_decoder(3, MAX_FRAMES, 2)
    pa, sa, fed = _run(dec, cfg, [(2, [0, 1, 2]), (2, [0, 1, 2])], codes)
    before = {r: dec.snapshot(r) for r in (0, 2)}
    dec.reset_row(1)
    for r in (0, 2):
        pos, snap = dec.snapshot(r)
        assert pos == before[r][0]
        np.testing.assert_array_equal(snap, before[r][1])
    pos1, snap1 = dec.snapshot(1)
    assert pos1 == 0 and dec.row_frames(1) == 0 and not snap1.any()  # zero carried rows, no key below the position
    new1 = rng.integers(0, cfg["bins"], (cfg["nq"], 4))
    codes2 = {0: codes[0], 1: np.concatenate([np.zeros((cfg["nq"], 4), np.int64), new1], 1), 2: codes[2]}  # (row 1's cursor stands at 4)
    pb, sb, fed = _run(dec, cfg, [(2, [0, 1, 2]), (2, [0, 1, 2])], codes2, fed=fed)
    for r in (0, 2):
        np.testing.assert_array_equal(np.concatenate(pa[r] + pb[r]), _solo(model, codes[r], [2, 2, 2, 2]), err_msg=f"row {r}")
    np.testing.assert_array_equal(np.concatenate(pa[1]), _solo(model, codes[1][:, :4], [2, 2]))
    np.testing.assert_array_equal(np.concatenate(pb[1]), _solo(model, new1, [2, 2]), err_msg="row 1 after its reset")
    dec.close()


def test_rows_with_different_key_windows():
    """Tiny codec, context 6: row 0 has 20 positions behind it (its key range slides) when row 1 starts fresh beside it."""
    cfg, w, model, spf = _setup("tiny")
    rng = np.random.default_rng(34)
    codes = {0: rng.integers(0, cfg["bins"], (cfg["nq"], 16)), 1: rng.integers(0, cfg["bins"], (cfg["nq"], 6))}
    dec = model.row_decoder(2, MAX_FRAMES, 2)
    dec.set_context(6)
    schedule = [(2, [0])] * 5 + [(2, [0, 1])] * 3
    pcm, steps, fed = _run(dec, cfg, schedule, codes)
    assert dec.snapshot(0)[0] == 16 * cfg["upsample_stride"] > 6 and dec.snapshot(1)[0] == 6 * cfg["upsample_stride"]
    for r in (0, 1):
        got = np.concatenate(pcm[r])
        np.testing.assert_array_equal(got, _solo(model, codes[r], steps[r], context=6), err_msg=f"row {r}")
        e = err_stats(got, _oracle(w, cfg, codes[r], steps[r], context=6))
        assert e["max_abs"] <= 1e-3 * max(1.0, e["ref_max"]), (r, e)
        if r == 0:
            assert np.abs(got - _solo(model, codes[r], steps[r])).max() > 1e-4  # (the short context is not vacuous)
    from mlx_audio_amd._lib import KokoroHipError

    with pytest.raises(KokoroHipError, match="fresh"):
        dec.set_context(8)  # only while every row is fresh
    dec.close()


def test_refusals_happen_on_the_host():
    """A row past max_frames, F > max_chunk and a bad row index are refused before any launch; the stream is left as it was."""
    from mlx_audio_amd._lib import KokoroHipError

    cfg, w, model, spf = _setup("tiny")
    rng = np.random.default_rng(35)
    dec = model.row_decoder(2, 4, 2)
    c2 = torch.tensor(rng.integers(0, cfg["bins"], (2, cfg["nq"], 2)))
    with pytest.raises(KokoroHipError, match="frames per step"):
        dec.step(torch.tensor(rng.integers(0, cfg["bins"], (2, cfg["nq"], 3))), [True, True])
    with pytest.raises(ValueError):
        dec.step(c2[:1], [True])
    with pytest.raises(ValueError):
        dec.step(c2, [True])
    for row in (-1, 2, 99):
        with pytest.raises(KokoroHipError, match="row out of range"):
            dec.reset_row(row)
        with pytest.raises(ValueError):
            dec.row_frames(row)
    first = dec.step(c2, [True, False]).cpu().numpy()
    dec.step(c2, [True, False])
    assert [dec.row_frames(r) for r in (0, 1)] == [4, 0]
    with pytest.raises(KokoroHipError, match="would hold 6 frames"):
        dec.step(c2, [True, True])
    assert [dec.row_frames(r) for r in (0, 1)] == [4, 0] and dec.snapshot(0)[0] == 4 * cfg["upsample_stride"]
    # the full row rides along inactive while the other one runs; once reset it starts over with the same bits as its first stream
    dec.step(c2, [False, True])
    dec.reset_row(0)
    again = dec.step(c2, [True, False]).cpu().numpy()
    np.testing.assert_array_equal(again[0], first[0])
    from mlx_audio_amd.mimi import Mimi  # noqa: F401

    with pytest.raises(KokoroHipError):
        model.row_decoder(65, 4, 2)  # the active mask is one 64-bit word
    with pytest.raises(KokoroHipError):
        model.row_decoder(2, 4, 5)   # max_chunk > max_frames
    dec.close()
    with pytest.raises(KokoroHipError, match="closed"):
        dec.step(c2, [True, False])
