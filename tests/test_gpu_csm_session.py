"""Multi-turn sessions on the device (kk_csm_prefix_capture, `SesameModel.capture_prefix`, `CSMBatcher.session` / `submit(session=)`).
The capture is an exact copy of a live row's window -- of prompt positions (equal to kk_csm_prefix_create on the same frames) and of generated
positions (equal whatever row, slot, batch and poll cadence the stream had) --, a session's turns are bit for bit those of the same session run
alone, and a turn on captured K / V stays within the project's logit bar of the CPU oracle run on the whole conversation as one prompt."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402

import mlx_audio_amd.params as P  # noqa: E402
from _util import err_stats, report  # noqa: E402

pytestmark = pytest.mark.gpu

TEMP, TOP_K, SEED = 0.8, 20, 1234
MAX_POS = 128
N_CB, KVW, LAYERS = 4, 128, 2  # the tiny configuration: a slot is 32 16-byte columns


def _ccfg():
    return dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=N_CB, max_seq_len=MAX_POS)


def _bf16(w):
    return {k: torch.tensor(np.asarray(v, np.float32)).to(torch.bfloat16).float().numpy() for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _loop(wdt):
    from mlx_audio_amd.mimi import Mimi, MimiConfig
    from mlx_audio_amd.sesame import Model

    mcfg = P.mimi_tiny_config()
    cw = P.csm_synth_checkpoint(_ccfg(), 3)
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 3, encode=True))
    return Model(_ccfg(), mimi=mimi, weights=_bf16(cw) if wdt == "bfloat16" else cw, weight_dtype=wdt)


def _sampler():
    from mlx_audio_amd.sesame import make_sampler

    return make_sampler(temp=TEMP, top_k=TOP_K)


def _frames(g, n_text, n_audio, n_cb=N_CB, text_vocab=300, audio_vocab=64):
    tok = np.zeros((n_text + n_audio, n_cb + 1), np.int32)
    msk = np.zeros((n_text + n_audio, n_cb + 1), np.float32)
    tok[:n_text, -1], msk[:n_text, -1] = g.integers(0, text_vocab, n_text), 1
    tok[n_text:, :n_cb], msk[n_text:, :n_cb] = g.integers(1, audio_vocab, (n_audio, n_cb)), 1
    return tok, msk


def _drive(bat, fut):
    """Scheduling rounds until the request is resolved (a batch of one is idle right after: `step` then says so, which is no failure)."""
    for _ in range(600):
        if fut.done():
            return
        bat.step()
    raise AssertionError("the request did not finish")


def _step(model, prev):
    """One greedy frame for all rows of the batch (parked rows are fed zeros), through the captured graph."""
    B = prev.shape[0]
    curr = torch.zeros((B, 1, N_CB + 1), dtype=torch.int32, device="cuda")
    curr[:, 0, :N_CB] = prev
    mask = torch.zeros((B, 1, N_CB + 1), dtype=torch.float32, device="cuda")
    mask[:, 0, :N_CB] = 1
    return model.generate_frame(curr, mask).clone()


# ---- 1. the capture is an exact copy: prompt positions ---------------------------------------------------------------------------------------
def test_capture_of_prompt_positions_equals_prefix_create_and_disturbs_nothing():
    """L = 33 in row 2 of four, pad 7, another row live: 33 slots are 1 056 columns (a full workgroup and a partial one), 5 slots 160 (one
    partial workgroup).  Every layer, K and V.  Then the same after the window has moved."""
    from mlx_audio_amd.csm import SesameModel

    model = SesameModel(_ccfg(), P.csm_synth_checkpoint(_ccfg(), 3))
    g = np.random.default_rng(31)
    other, mine = _frames(g, 4, 2), _frames(g, 20, 13)
    want = model.make_prefix(*mine).save().view(LAYERS, 2, 33, KVW)
    assert bool((want[1].abs().sum(dim=(1, 2)) > 0).all()) and not torch.equal(want[0], want[1]) and not torch.equal(want[:, 0], want[:, 1])

    def run(capture):
        model.setup_caches(4)
        model.reset_caches_parked()
        model.set_graph_mode(True)
        model.shift(40)
        prev = torch.zeros((4, N_CB), dtype=torch.int32, device="cuda")
        prev[0], prev[2] = model.admit(0, *other), model.admit(2, *mine)
        assert model.row_state() == ([34, MAX_POS, 7, MAX_POS], 40)
        got, out = [], []
        if capture:
            got.append(model.capture_prefix(2, 33))
        for f in range(6):
            prev = _step(model, prev)
            out.append(prev.cpu().numpy())
            if capture and f == 3:  # between two replays of the captured frame step
                state = model.row_state()
                got += [model.capture_prefix(2, 33), model.capture_prefix(2, 5)]
                assert model.row_state() == state
        model.shift(-3)
        assert model.row_state() == ([31, MAX_POS, 4, MAX_POS], 43)
        if capture:
            got.append(model.capture_prefix(2, 33))
        out.append(_step(model, prev).cpu().numpy())
        return got, np.stack(out)

    _, plain = run(False)
    got, beside = run(True)
    first, mid, five, moved = got
    assert first.length == 33 and first.nbytes == 2 * LAYERS * 33 * KVW * 4 and five.nbytes == 2 * LAYERS * 5 * KVW * 4
    for name, p in (("at admission", first), ("between replays", mid), ("after the shift", moved)):
        assert torch.equal(p.save().view(LAYERS, 2, 33, KVW), want), name
    assert torch.equal(five.save().view(LAYERS, 2, 5, KVW), want[:, :, :5].contiguous())
    np.testing.assert_array_equal(beside, plain)  # both rows' codes, the replays behind the captures included
    codes = model.admit(1, *_frames(g, 2, 0), prefix=moved)  # and it is a Prefix like any other: 33 + 2 <= 44
    assert codes.shape == (N_CB,) and model.row_state()[0][1] == 44 - 35


# ---- 2. the capture is an exact copy: generated positions -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_capture_of_generated_positions_is_the_same_wherever_the_stream_ran(wdt):
    """Stream A (L = 7): in a busy batch of four (row 2, a non-zero pad, polls every 8 frames) captured at L + 6 when the row already holds
    L + 9 positions; alone (one row, pad 0) captured when it holds exactly L + 6."""
    loop = _loop(wdt)
    g = np.random.default_rng(32)
    a, others = _frames(g, 5, 2), [_frames(g, 6, 3), _frames(g, 3, 1)]

    def run(busy):
        bat = loop.serve(max_batch=4 if busy else 1, eos_check_interval=8 if busy else 1, rng="device", sampler=_sampler(), seed=SEED, decode=False,
                         stop_on_eos=False)
        if busy:
            for i, p in enumerate(others):
                bat.submit(None, None, prompt=p, max_audio_length_ms=80 * 40, stream_id=60 + i)
            for _ in range(3):
                bat.step()
        bat.submit(None, None, prompt=a, max_audio_length_ms=80 * 40, stream_id=50)
        s = None
        for _ in range(9 if busy else 6):
            bat.step()
            s = s or [x for x in bat._live() if x.stream_id == 50][0]
        pad, pos = loop.model.row_state()
        assert pos - pad[s.row] == 7 + (9 if busy else 6) and (s.row, pad[s.row] > 0) == ((2, True) if busy else (0, False))
        cap = loop.model.capture_prefix(s.row, 7 + 6)
        out = cap.save().clone()
        cap.close()
        bat.close()
        return out, torch.stack(s.codes[:7]).cpu()

    (solo, solo_codes), (busy, busy_codes) = run(False), run(True)
    assert torch.equal(solo_codes, busy_codes)
    assert solo.numel() == 2 * LAYERS * 13 * KVW and torch.equal(solo, busy)
    prompt_part = loop.model.make_prefix(*a).save().view(LAYERS, 2, 7, KVW)  # (the prompt's share is a prompt block's, as in test 1)
    assert torch.equal(solo.view(LAYERS, 2, 13, KVW)[:, :, :7].contiguous(), prompt_part)


# ---- 3. a session's turns equal the session alone -------------------------------------------------------------------------------------------
def _conversation(loop, rng, busy):
    """Three limit-ended turns with a heard turn (with audio) between the second and the third.  busy: a batch of four that also runs plain and
    prefix= requests and passes a down-shift between the turns; the second turn is streamed.  Else a batch of one."""
    from mlx_audio_amd.sesame import Segment

    g = np.random.default_rng(33)
    texts = [g.integers(0, 300, n).tolist() for n in (4, 3, 2)]
    heard = Segment(speaker=1, text=g.integers(0, 300, 3).tolist(), audio=(0.3 * g.standard_normal(1920 * 4)).astype(np.float32))
    ctx = [Segment(speaker=2, text=g.integers(0, 300, 4).tolist(), audio=(0.3 * g.standard_normal(1920 * 3)).astype(np.float32))]
    bat = loop.serve(max_batch=4 if busy else 1, eos_check_interval=8 if busy else 1, rng=rng, sampler=_sampler(), seed=SEED,
                     stream_chunk_frames=3 if busy else None, stream_max_frames=16)
    own = (lambda k: k) if rng == "host" else (lambda k: None)  # rng "device": every stream draws on the batcher's seed
    side, vp = [], None
    if busy:
        vp = loop.voice_prefix(ctx)
        side.append(bat.submit(None, None, prompt=_frames(g, 5, 1), max_audio_length_ms=80 * 30, seed=own(7), stream_id=80))
        for _ in range(2):
            bat.step()
    sess = bat.session(speaker=0)
    out, chunks = [], None
    for t, text in enumerate(texts):
        kw = dict(max_audio_length_ms=80 * 8, seed=own(100 + t), stream_id=50 + t)
        if busy:
            side.append(bat.submit(prefix=vp, text=g.integers(0, 300, 2).tolist(), speaker=2, max_audio_length_ms=80 * (5 + t), seed=own(8), stream_id=81 + t))
        if busy and t == 1:  # the stream that carries the batch past the end of the cache: live from P ~ 17 for 118 frames
            side.append(bat.submit(None, None, prompt=_frames(g, 4, 2), max_audio_length_ms=80 * 118, seed=own(9), stream_id=90))
        if t == 2:
            sess.hear(heard)
            if busy:
                while bat.stats["shifts_down"] == 0:
                    assert bat.step()
        if busy and t == 1:
            stream = sess.submit_stream(text, **kw)
            _drive(bat, stream.future)
            chunks, res = list(stream), stream.result(timeout=0)
        else:
            fut = sess.submit(text, **kw)
            _drive(bat, fut)
            res = fut.result(timeout=0)
        out.append(res)
    assert [t[2] for t in sess.turns] == [8, 8, 0, 8] and sess.length == sess.history[0].shape[0] == (4 + 9) + (3 + 9) + (3 + 5) + (2 + 9)
    assert bat.stats["session_admissions"] == 3 and bat.stats["captures"] == 3 and bat.stats["prefixed_admissions"] == 2 + (3 if busy else 0)
    bat.run_until_idle()
    for f in side:
        f.result(timeout=0)
    stats = dict(bat.stats)
    sess.close()
    bat.close()
    if vp is not None:
        vp.close()
    return out, chunks, stats


@pytest.mark.parametrize("wdt,rng", [("float32", "device"), ("float32", "host"), ("bfloat16", "device"), ("bfloat16", "host")])
def test_a_sessions_turns_equal_the_session_alone(wdt, rng):
    loop = _loop(wdt)
    solo, _, _ = _conversation(loop, rng, busy=False)
    got, chunks, stats = _conversation(loop, rng, busy=True)
    assert stats["shifts_down"] >= 1
    for t, (a, b) in enumerate(zip(solo, got)):
        assert a.frames == b.frames == 8, t
        np.testing.assert_array_equal(b.codes.cpu().numpy(), a.codes.cpu().numpy(), err_msg=f"turn {t + 1}")
    # the streamed turn against its submit form: the same frames, in chunks of 3, 3, 2 whose concatenation is the result's audio
    assert [(c.first_frame, c.frames, c.final) for c in chunks] == [(0, 3, False), (3, 3, False), (6, 2, True)]
    cat = torch.cat([c.audio for c in chunks])
    assert torch.equal(cat, got[1].audio) and cat.shape == solo[1].audio.shape
    assert torch.equal(got[0].audio, solo[0].audio) and torch.equal(got[2].audio, solo[2].audio)


# ---- 4. against the oracle --------------------------------------------------------------------------------------------------------------------
def test_a_turn_on_captured_kv_against_the_oracle_on_the_whole_conversation():
    """Greedy, float32 weights.  Turn 1 (4 frames, limit-ended) is captured; turn 2's prompt is the capture, then the last kept frame, the EOS frame
    and the new text.  The oracle takes the session's `history` plus that text as ONE prompt.  An admission does not publish its logits
    (kk_csm_debug_logits: "an admission leaves the live rows' debug logits alone"), so the first frame of turn 2 is checked through its codes
    and the logits are those of the frame behind it: the first single-token step whose attention reads every captured position.  The bar is
    that of tests/test_gpu_csm.py for frames on top of single-token K / V, rel_max < 2e-4.  The same whole prompt through the plain admission
    is measured beside it.  Codes are asserted where the oracle's gap between the picked and the next logit exceeds twice the bar; for this
    seed (chosen on the CPU with the oracle alone, smallest gap 1.2e-2 of the largest logit) that is every code book of both frames."""
    import csm_oracle as C
    from mlx_audio_amd.sesame import Model, make_sampler

    BAR = 2e-4
    cfg, w = _ccfg(), P.csm_synth_checkpoint(_ccfg(), 3)
    loop = Model(cfg, weights=w)
    g = np.random.default_rng(45)
    t1, t2 = g.integers(0, 300, 5).tolist(), g.integers(0, 300, 3).tolist()

    def first_two_frames(bat, **req):
        fut = bat.submit(max_audio_length_ms=80 * 5, **req)
        assert bat.step()  # the admission and one frame step
        s = bat._live()[0]
        torch.cuda.synchronize()
        lg = loop.model.debug_logits().cpu().numpy()[:, s.row]  # [n_cb, V] of the frame step
        codes = torch.stack(s.codes[:2]).cpu().numpy()
        bat.run_until_idle()
        fut.result(timeout=0)
        return lg, codes

    bat = loop.serve(max_batch=2, rng="host", sampler=make_sampler(temp=0.0), decode=False)
    sess = bat.session()
    f1 = sess.submit(t1, max_audio_length_ms=80 * 4)
    bat.run_until_idle()
    assert f1.result(timeout=0).frames == 4 and sess.n == 5 + 3 and sess.pending[0].shape[0] == 2
    text = loop._tokenize_text_segment(t2, 0)
    whole = np.concatenate([sess.history[0], text[0]]), np.concatenate([sess.history[1], text[1]])
    assert whole[0].shape[0] == 5 + 4 + 1 + 3
    lg_sess, codes_sess = first_two_frames(bat, session=sess, text=t2)
    assert bat.stats["session_admissions"] == 2 and bat.stats["prefixed_admissions"] == 1
    bat.close()
    bat = loop.serve(max_batch=2, rng="host", sampler=make_sampler(temp=0.0), decode=False)
    lg_plain, codes_plain = first_two_frames(bat, prompt=whole)
    bat.close()

    orc = C.CsmOracle(w, cfg)
    ref_codes, ref_lg, gaps = [], [], []
    tok, msk = whole[0][None].astype(np.int64), whole[1][None]
    for _ in range(2):
        trace = {}
        c = orc.generate_frame(tok, msk, temp=0.0, top_k=10, trace=trace)
        lg = np.stack([trace["c0_logits"]] + trace["ci_logits"], 0)[:, 0]
        top = np.sort(lg, axis=1)
        ref_codes.append(c[0]); ref_lg.append(lg); gaps.append((top[:, -1] - top[:, -2]) / np.abs(lg).max())
        tok, msk = np.zeros((1, 1, N_CB + 1), np.int64), np.zeros((1, 1, N_CB + 1), np.float32)
        tok[0, 0, :N_CB], msk[0, 0, :N_CB] = c[0], 1
    assert (np.stack(gaps) > 2 * BAR).all(), gaps  # a condition on the inputs: every code book qualifies
    e_sess, e_plain = err_stats(lg_sess, ref_lg[1]), err_stats(lg_plain, ref_lg[1])
    report("csm/session/turn2_frame2/logits_on_captured_kv", **e_sess)
    report("csm/session/turn2_frame2/logits_plain_admission", **e_plain)
    np.testing.assert_array_equal(codes_plain, np.stack(ref_codes))
    np.testing.assert_array_equal(codes_sess, np.stack(ref_codes))
    assert e_plain["rel_max"] < BAR, e_plain
    assert e_sess["rel_max"] < BAR, e_sess
    sess.close()


# ---- 5. the real head geometry ------------------------------------------------------------------------------------------------------------------
def test_real_head_geometry_session_whose_capture_crosses_a_key_chunk_edge():
    """8 kv heads x 64 on a short stack, bf16 weight mode, 256 slots: turn 1 is 110 prompt frames and 25 generated ones, its capture holds 134
    positions -- across the 128-key chunk edge of the single-token attention -- and turn 2 runs on it, beside a plain stream and alone."""
    from mlx_audio_amd.sesame import Model

    cfg = P.csm_config()
    cfg = dict(cfg, text_vocab_size=500, audio_vocab_size=1100, audio_num_codebooks=6, max_seq_len=256,
               backbone=dict(cfg["backbone"], num_layers=2, intermediate=1024), decoder=dict(cfg["decoder"], num_layers=2, intermediate=768))
    loop = Model(cfg, weights=_bf16(P.csm_synth_checkpoint(cfg, 2)), weight_dtype="bfloat16")

    def run(busy):
        g = np.random.default_rng(35)
        texts = [g.integers(0, 500, n).tolist() for n in (110, 4)]
        plain = _frames(g, 30, 10, n_cb=6, text_vocab=500, audio_vocab=1100)
        bat = loop.serve(max_batch=2 if busy else 1, eos_check_interval=8 if busy else 1, rng="device", sampler=_sampler(), seed=SEED, decode=False)
        if busy:
            side = bat.submit(None, None, prompt=plain, max_audio_length_ms=80 * 60, stream_id=60)
            for _ in range(3):
                bat.step()
        sess = bat.session()
        out = []
        for t, (text, frames) in enumerate(zip(texts, (25, 10))):
            fut = sess.submit(text, max_audio_length_ms=80 * frames, stream_id=50 + t)
            _drive(bat, fut)
            out.append(fut.result(timeout=0).codes.cpu().numpy())
            if t == 0:
                assert sess.n == 110 + 24 and sess.prefix.prefix.nbytes == 2 * 2 * 134 * 512 * 4
        bat.run_until_idle()
        if busy:
            side.result(timeout=0)
        sess.close()
        bat.close()
        return out

    solo, busy = run(False), run(True)
    assert [c.shape for c in solo] == [(6, 25), (6, 10)]
    for a, b in zip(solo, busy):
        np.testing.assert_array_equal(b, a)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_capture_refusals_are_decided_on_the_host():
    from mlx_audio_amd.csm import SesameModel

    model = SesameModel(_ccfg(), P.csm_synth_checkpoint(_ccfg(), 3))
    lib, h, out = model.lib, model._h, ctypes.c_void_p()

    def raw(row, n):
        return lib.kk_csm_prefix_capture(h, None, row, n, ctypes.byref(out))

    assert raw(0, 1) != 0 and b"kk_csm_setup_caches" in lib.kk_last_error()  # no caches
    model.setup_caches(3)
    model.reset_caches_parked()
    model.shift(9)
    g = np.random.default_rng(36)
    model.admit(1, *_frames(g, 4, 2))
    state = ([MAX_POS, 3, MAX_POS], 9)
    assert model.row_state() == state
    for row in (-1, 3):
        assert raw(row, 1) != 0 and b"row out of range" in lib.kk_last_error()
    assert raw(0, 1) != 0 and b"parked" in lib.kk_last_error()
    assert raw(1, 0) != 0 and b"at least 1" in lib.kk_last_error()
    assert raw(1, 7) != 0 and b"fewer than n" in lib.kk_last_error()  # the row holds 6
    for row, n in ((3, 1), (0, 1), (1, 0), (1, 7)):
        with pytest.raises(ValueError):
            model.capture_prefix(row, n)
    assert out.value is None and model.row_state() == state
    cap = model.capture_prefix(1, 6)
    assert cap.length == 6 and lib.kk_csm_prefix_length(cap._h) == 6
    cap.close()
    torch.cuda.synchronize()
