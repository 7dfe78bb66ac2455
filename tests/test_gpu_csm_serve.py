"""Continuous batching of CSM streams (csm_serve.CSMBatcher on kk_csm_admit / kk_csm_park_row / kk_csm_shift_caches): a stream admitted into a
running batch, into a reused row, beside parked rows, across a down-shift and an up-shift of the caches carries, bit for bit, the code frames
and the waveform of its own `generate_batch([prompt])` run.  No tolerance anywhere: every comparison is array equality."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import mlx_audio_amd.params as P  # noqa: E402

pytestmark = pytest.mark.gpu

TEMP, TOP_K, SEED = 0.8, 20, 1234


def _bf16(w):
    return {k: torch.tensor(np.asarray(v, np.float32)).to(torch.bfloat16).float().numpy() for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _loop(wdt):
    from mlx_audio_amd.mimi import Mimi, MimiConfig
    from mlx_audio_amd.sesame import Model

    ccfg = dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=4, max_seq_len=128)
    mcfg = P.mimi_tiny_config()
    cw = P.csm_synth_checkpoint(ccfg, 3)
    if wdt == "bfloat16":
        cw = _bf16(cw)
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 3, encode=True))
    return Model(ccfg, mimi=mimi, weights=cw, weight_dtype=wdt)


def _request(rng, speaker, n_ctx_text, n_audio, n_text, voice_match=False):
    """(context, text, speaker, voice_match): a context segment with `n_audio` frames of reference audio (0: text only) and a text."""
    from mlx_audio_amd.sesame import Segment

    audio = (0.3 * rng.standard_normal(1920 * n_audio)).astype(np.float32) if n_audio else None
    return dict(context=[Segment(speaker=speaker, text=rng.integers(0, 300, n_ctx_text).tolist(), audio=audio)],
                text=rng.integers(0, 300, n_text).tolist(), speaker=speaker, voice_match=voice_match)


def _sampler():
    from mlx_audio_amd.sesame import make_sampler

    return make_sampler(temp=TEMP, top_k=TOP_K)


def _solo(loop, req, frames, rng, seed, sid):
    prompt = loop.prompt_frames(req["context"], req["text"], req["speaker"], voice_match=req["voice_match"])
    if rng == "host":
        return loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=_sampler(), seed=seed)
    return loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=_sampler(), seed=SEED, rng="device", stream_ids=[sid])


def _check(loop, rng, reqs, frames, results, names=None):
    """every stream against its own batch-1 run: frames, codes, waveform"""
    for i, (req, f, fut) in enumerate(zip(reqs, frames, results)):
        got = fut.result(timeout=0)
        ref = _solo(loop, req, f, rng, 100 + i, 50 + i)
        tag = f"stream {names[i] if names else i}"
        assert got.frames == ref.frames[0], tag
        np.testing.assert_array_equal(got.codes.cpu().numpy(), ref.codes[0][:, : ref.frames[0]].cpu().numpy(), err_msg=tag)
        assert torch.equal(got.audio, ref.audio[0]), tag


def _submit(bat, rng, i, req, frames):
    return bat.submit(max_audio_length_ms=80 * frames, seed=(100 + i) if rng == "host" else None, stream_id=50 + i, **req)


@pytest.mark.parametrize("rng", ["host", "device"])
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_admit_into_a_running_batch_equals_solo_runs(wdt, rng):
    """A and B start together in a max_batch = 4 engine; C (another prompt length, with reference audio) is admitted after 5 frames."""
    loop = _loop(wdt)
    g = np.random.default_rng(5)
    reqs = [_request(g, 0, 5, 3, 4), _request(g, 1, 5, 1, 9, voice_match=True), _request(g, 2, 4, 5, 2)]
    frames = [14, 11, 9]
    bat = loop.serve(max_batch=4, rng=rng, sampler=_sampler(), seed=SEED)
    futs = [_submit(bat, rng, i, reqs[i], frames[i]) for i in (0, 1)]
    for _ in range(5):
        assert bat.step()
    pad, pos = loop.model.row_state()
    assert sum(p < 128 for p in pad) == 2
    futs.append(_submit(bat, rng, 2, reqs[2], frames[2]))
    bat.step()
    pad2, pos2 = loop.model.row_state()
    assert sum(p < 128 for p in pad2) == 3 and pos2 == pos + 1 and pad2[:2] == pad[:2]  # C sits in a third row; A and B did not move
    bat.run_until_idle()
    assert bat.stats["admissions"] == 3
    _check(loop, rng, reqs, frames, futs, "ABC")


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_row_reuse_nothing_of_the_previous_stream_leaks(wdt):
    """A ends early; D is admitted into A's row (on top of A's stale keys) while B runs on."""
    loop = _loop(wdt)
    g = np.random.default_rng(6)
    reqs = [_request(g, 0, 6, 4, 5), _request(g, 1, 5, 2, 3), _request(g, 2, 3, 2, 2)]  # A (the longest prompt), B, D
    frames = [6, 30, 12]
    bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED)
    futs = [_submit(bat, "device", i, reqs[i], frames[i]) for i in range(3)]
    bat.run_until_idle()
    a, b, d = (f.result(timeout=0) for f in futs)
    assert d.row == a.row != b.row
    _check(loop, "device", reqs, frames, futs, "ABD")


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_parked_rows_ride_along_harmlessly(wdt):
    """One live stream in a max_batch = 4 engine whose other rows were never used."""
    loop = _loop(wdt)
    g = np.random.default_rng(7)
    reqs, frames = [_request(g, 0, 5, 3, 4)], [12]
    bat = loop.serve(max_batch=4, rng="host", sampler=_sampler())
    futs = [_submit(bat, "host", 0, reqs[0], frames[0])]
    seen = []
    while bat.step():
        seen.append(bat._prev.cpu().numpy().copy())
    pad, _ = loop.model.row_state()
    assert pad == [128] * 4  # the stream's row is parked again
    seen = np.stack(seen)
    assert seen.shape[1:] == (4, 4) and seen.min() >= 0 and seen.max() < 64  # parked rows: codes in [0, V)
    _check(loop, "host", reqs, frames, futs)


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_shift_down_with_overlap_when_the_position_reaches_the_end(wdt):
    """A 40- and a 50-frame stream, then a 100-frame stream beside short ones: the session passes max_seq_len = 128 slots, so every live window is
    moved down while the long stream is longer than the move (source and destination overlap)."""
    loop = _loop(wdt)
    g = np.random.default_rng(8)
    reqs = [_request(g, 0, 5, 2, 4), _request(g, 1, 4, 3, 3), _request(g, 2, 5, 3, 4), _request(g, 3, 3, 1, 4), _request(g, 4, 3, 2, 3),
            _request(g, 5, 4, 1, 2)]
    frames = [40, 50, 100, 30, 30, 30]
    bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED)
    futs = [_submit(bat, "device", i, reqs[i], frames[i]) for i in range(6)]
    moves = []
    prev = loop.model.row_state()
    while bat.step() or bat._queue:
        now = loop.model.row_state()
        live = [b for b in range(2) if prev[0][b] < 128 and now[0][b] < 128]
        if now[1] < prev[1] and live:  # the position went DOWN under rows that were live before and after
            delta = prev[1] + 1 - now[1]  # (the round ran one frame after the shift)
            assert prev[1] == 128 and all(prev[0][b] - now[0][b] == delta for b in live) and min(now[0][b] for b in live) == 0
            moves.append((delta, max(prev[1] - prev[0][b] for b in live)))
        prev = now
    assert moves and any(delta < length for delta, length in moves), moves  # at least one overlapping move
    assert bat.stats["shifts_down"] >= len(moves)
    _check(loop, "device", reqs, frames, futs)


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_shift_up_for_a_prompt_longer_than_the_position(wdt):
    loop = _loop(wdt)
    g = np.random.default_rng(9)
    reqs = [_request(g, 0, 3, 0, 3), _request(g, 1, 6, 6, 6)]  # 6 frames of prompt; 6 + 7 + 6 = 19
    frames = [20, 10]
    bat = loop.serve(max_batch=2, rng="host", sampler=_sampler())
    futs = [_submit(bat, "host", 0, reqs[0], frames[0])]
    for _ in range(3):
        bat.step()
    pad, pos = loop.model.row_state()
    assert pos == 6 + 3 and pad[0] == 0 and bat.stats["shifts_up"] == 1  # (the first admission moved the bare position from 0 to 6)
    futs.append(_submit(bat, "host", 1, reqs[1], frames[1]))
    bat.step()
    pad2, pos2 = loop.model.row_state()
    assert bat.stats["shifts_up"] == 2 and pos2 == 19 + 1 and pad2 == [19 - 9, 0]  # A's window moved up by 19 - 9
    bat.run_until_idle()
    _check(loop, "host", reqs, frames, futs, "AB")


def test_real_head_geometry_admission_across_a_key_chunk_edge():
    """llama-1B / llama-100M head geometry on a short stack, bf16 weight mode, 256 cache slots: the backbone's single-token attention is
    attn_decode_kernel with key chunks of 128.  A stream admitted at a non-zero pad whose prompt plus frames cross the chunk edge."""
    from mlx_audio_amd.sesame import Model

    cfg = P.csm_config()
    cfg = dict(cfg, text_vocab_size=500, audio_vocab_size=1100, audio_num_codebooks=6, max_seq_len=256,
               backbone=dict(cfg["backbone"], num_layers=2, intermediate=1024), decoder=dict(cfg["decoder"], num_layers=2, intermediate=768))
    loop = Model(cfg, weights=_bf16(P.csm_synth_checkpoint(cfg, 2)), weight_dtype="bfloat16")
    g = np.random.default_rng(10)

    def prompt(n_text, n_audio):
        tok = np.zeros((n_text + n_audio, 7), np.int32)
        msk = np.zeros((n_text + n_audio, 7), np.float32)
        tok[:n_text, -1], msk[:n_text, -1] = g.integers(0, 500, n_text), 1
        tok[n_text:, :6], msk[n_text:, :6] = g.integers(0, 1100, (n_audio, 6)), 1
        return tok, msk

    prompts, frames = [prompt(20, 120), prompt(30, 90)], [40, 20]  # A: 140 + 40 frames; B: 120 keys of its own, crossing 128 after 8 frames
    bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, decode=False)
    futs = [bat.submit(None, None, prompt=prompts[0], max_audio_length_ms=80 * frames[0], stream_id=50)]
    for _ in range(7):
        bat.step()
    futs.append(bat.submit(None, None, prompt=prompts[1], max_audio_length_ms=80 * frames[1], stream_id=51))
    bat.step()
    pad, pos = loop.model.row_state()
    assert pos == 140 + 8 and pad == [0, 148 - 1 - 120]
    bat.run_until_idle()
    for i in range(2):
        got = futs[i].result(timeout=0)
        ref = loop.generate_batch([prompts[i]], max_audio_length_ms=80 * frames[i], sampler=_sampler(), seed=SEED, rng="device", stream_ids=[50 + i],
                                  decode=False)
        assert got.frames == ref.frames[0]
        np.testing.assert_array_equal(got.codes.cpu().numpy(), ref.codes[0][:, : ref.frames[0]].cpu().numpy())


def test_refusals_are_decided_on_the_host():
    """A live row, a row out of range, S > P without the shift, a shift that would push a window out of the cache, an admission without
    caches: the library returns its error (and Python raises ValueError) before any launch; the state is unchanged."""
    from mlx_audio_amd import _lib
    from mlx_audio_amd.csm import SesameModel

    ccfg = dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=4, max_seq_len=128)
    model = SesameModel(ccfg, P.csm_synth_checkpoint(ccfg, 3))
    lib, h = model.lib, model._h
    sp = _lib.KKCsmSampler(0.0, 0, 0.0, 0.0, 1, 0, 0)
    buf = torch.zeros(1 << 20, dtype=torch.int32, device="cuda")  # tokens / mask / workspace / codes stand-ins: no refused call launches
    ptr = ctypes.c_void_p(buf.data_ptr())

    def raw_admit(row, S):
        return lib.kk_csm_admit(h, None, row, S, ptr, ptr, ctypes.byref(sp), None, 0, ptr, buf.numel() * 4, ptr)

    assert raw_admit(0, 4) != 0 and b"kk_csm_setup_caches" in lib.kk_last_error()  # no caches
    assert lib.kk_csm_park_row(h, 0) != 0 and lib.kk_csm_shift_caches(h, None, 1, None, 0) != 0
    model.setup_caches(4)
    model.reset_caches_parked()
    tok, msk = np.zeros((5, 5), np.int32), np.zeros((5, 5), np.float32)
    msk[:, -1] = 1
    assert model.row_state() == ([128] * 4, 0)
    assert raw_admit(0, 5) != 0 and b"longer than the cache position" in lib.kk_last_error()  # S > P
    with pytest.raises(ValueError):
        model.admit(0, tok, msk)
    model.shift(5)  # nothing live: the bare position moves
    for row in (-1, 4):
        assert raw_admit(row, 5) != 0 and b"row out of range" in lib.kk_last_error()
        with pytest.raises(ValueError):
            model.admit(row, tok, msk)
        with pytest.raises(ValueError):
            model.park(row)
    codes = model.admit(1, tok, msk)
    assert codes.shape == (4,) and model.row_state() == ([128, 0, 128, 128], 5)
    assert raw_admit(1, 5) != 0 and b"the row is live" in lib.kk_last_error()
    with pytest.raises(ValueError):
        model.admit(1, tok, msk)
    for delta in (-1, 124, -6):  # the live window [0, 5) would leave [0, 128), or the position would
        assert lib.kk_csm_shift_caches(h, None, delta, None, 0) != 0 and b"leave the cache" in lib.kk_last_error()
        with pytest.raises(ValueError):
            model.shift(delta)
    assert model.row_state() == ([128, 0, 128, 128], 5)
    model.shift(123)
    assert model.row_state() == ([128, 123, 128, 128], 128)
    model.park(1)
    assert model.row_state() == ([128] * 4, 128)
    torch.cuda.synchronize()
