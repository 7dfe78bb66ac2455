"""Admissions prefilled on a side stream (kk_csm_admit_transfer, `SesameModel.admit_transfer`, `CSMBatcher(overlap_admission=True)`).
The transfer is an exact copy of a lane's window into a parked row of a running batch; a request served through a lane carries, bit for bit, the
codes and the waveform of its own `generate_batch([prompt])` run and of the same workload with the option off -- whichever lane and row it
used and however many frames passed between its prefill and its commit.  No tolerance anywhere: every comparison is array equality.

Two generators on one weight set are `share()`s of one model, and the rotary table -- `max_seq_len` long -- belongs to the weight set, so the two
sides of a transfer always agree on `max_seq_len`; their layer pitches differ through `max_batch` (1 in the lane, 3 in the batch).  A geometry
with kv_heads * head_dim % 4 != 0 is refused by kk_csm_create already, so that refusal of the transfer cannot be reached from here."""
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


@functools.lru_cache(maxsize=None)
def _generators():
    """One weight set, three generators: the batch (3 rows), its twin (3 rows, plain admissions) and the lane (1 row)."""
    from mlx_audio_amd.csm import SesameModel

    main = SesameModel(_ccfg(), P.csm_synth_checkpoint(_ccfg(), 3))
    twin, lane = main.share(), main.share()
    main.setup_caches(3), twin.setup_caches(3), lane.setup_caches(1)
    return main, twin, lane


def _sampler(**kw):
    from mlx_audio_amd.sesame import make_sampler

    return make_sampler(**(kw or dict(temp=TEMP, top_k=TOP_K)))


def _frames(g, n_text, n_audio, n_cb=N_CB, text_vocab=300, audio_vocab=64):
    tok = np.zeros((n_text + n_audio, n_cb + 1), np.int32)
    msk = np.zeros((n_text + n_audio, n_cb + 1), np.float32)
    tok[:n_text, -1], msk[:n_text, -1] = g.integers(0, text_vocab, n_text), 1
    tok[n_text:, :n_cb], msk[n_text:, :n_cb] = g.integers(1, audio_vocab, (n_audio, n_cb)), 1
    return tok, msk


def _step(model, prev):
    """One greedy frame for all rows of the batch, through the captured graph."""
    B = prev.shape[0]
    curr = torch.zeros((B, 1, N_CB + 1), dtype=torch.int32, device="cuda")
    curr[:, 0, :N_CB] = prev
    mask = torch.zeros((B, 1, N_CB + 1), dtype=torch.float32, device="cuda")
    mask[:, 0, :N_CB] = 1
    return model.generate_frame(curr, mask).clone()


def _drive(bat, fut):
    for _ in range(600):
        if fut.done():
            return
        bat.step()
    raise AssertionError("the request did not finish")


# ---- 1. the copy, exact ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_text,n_audio", [(1, 0), (3, 2), (20, 13)])
def test_the_transfer_is_an_exact_copy_and_disturbs_nothing(n_text, n_audio):
    """L = 1 (32 columns), 5 (160: one partial workgroup) and 33 (1 056: a full workgroup and a ragged one) from the lane's only row into row 2
    of three while rows 0 and 1 are live at other pads.  The twin takes the same three prompts through plain admissions.  Every layer, K and V,
    of all three rows; the position and the pads; the codes of the frame steps behind it; and all of it again after a down-shift."""
    main, twin, lane = _generators()
    g = np.random.default_rng(41)
    others, mine = [_frames(g, 4, 2), _frames(g, 7, 4)], _frames(g, n_text, n_audio)
    L = n_text + n_audio
    side = torch.cuda.Stream()
    for m in (main, twin):
        m.reset_caches_parked()
        m.set_graph_mode(True)
        m.shift(40)
    prev = [torch.zeros((3, N_CB), dtype=torch.int32, device="cuda") for _ in range(2)]
    for r in range(2):
        prev[0][r], prev[1][r] = main.admit(r, *others[r]), twin.admit(r, *others[r])
    for _ in range(2):  # the batch is running when the admission arrives
        prev = [_step(main, prev[0]), _step(twin, prev[1])]
    state = main.row_state()
    assert state == ([40 - 6, 40 - 11, MAX_POS], 42)
    with torch.cuda.stream(side):  # the lane's sequence per request, as the batcher's engine issues it
        lane.reset_caches_parked()
        lane.shift(L)
        first = lane.admit(0, *mine)
    assert lane.row_state() == ([0], L)
    main.admit_transfer(2, lane, 0, side)
    lane.park(0)
    prev[0][2], prev[1][2] = first, twin.admit(2, *mine)
    assert main.row_state() == ([34, 29, 42 - L], 42) == twin.row_state()
    assert torch.equal(prev[0], prev[1])

    def windows(m):
        """every position every row holds: kk_csm_prefix_capture + kk_csm_prefix_read"""
        pad, pos = m.row_state()
        out = []
        for r in range(3):
            cap = m.capture_prefix(r, pos - pad[r])
            out.append(cap.save().view(LAYERS, 2, pos - pad[r], KVW).clone())
            cap.close()
        return out

    got, want = windows(main), windows(twin)
    assert want[2].shape == (LAYERS, 2, L, KVW) and bool((want[2].abs().sum(dim=(2, 3)) > 0).all())
    for r in range(3):
        assert torch.equal(got[r], want[r]), f"row {r} behind the transfer"
    for f in range(3):  # the first frame steps behind the transfer
        prev = [_step(main, prev[0]), _step(twin, prev[1])]
        assert torch.equal(prev[0], prev[1]), f"frame {f} behind the transfer"
    down = min(29, 42 - L)  # the longest window goes to slot 0
    for m in (main, twin):
        m.shift(-down)
    assert main.row_state() == ([34 - down, 29 - down, 42 - L - down], 45 - down) == twin.row_state()
    got, want = windows(main), windows(twin)
    assert got[2].shape[2] == L + 3
    for r in range(3):
        assert torch.equal(got[r], want[r]), f"row {r} after the shift"
    prev = [_step(main, prev[0]), _step(twin, prev[1])]
    assert torch.equal(prev[0], prev[1])
    torch.cuda.synchronize()


# ---- 2. serving, bit for bit -------------------------------------------------------------------------------------------------------------------
def _request(rng, speaker, n_ctx_text, n_audio, n_text, voice_match=False):
    from mlx_audio_amd.sesame import Segment

    audio = (0.3 * rng.standard_normal(1920 * n_audio)).astype(np.float32) if n_audio else None
    return dict(context=[Segment(speaker=speaker, text=rng.integers(0, 300, n_ctx_text).tolist(), audio=audio)],
                text=rng.integers(0, 300, n_text).tolist(), speaker=speaker, voice_match=voice_match)


FRAMES = [30, 36, 66, 12, 10, 9, 30, 8]


def _workload():
    """Eight requests for two rows.  A's prompt (34 frames) sets the position; B's (41) is longer than the position when it is committed: an
    up-shift under a live row.  C runs 66 frames in one row -- through the end of the 128-slot cache -- while D .. G follow each other in the
    other row, each prefilled long before its row is free; H sits in the lane when the down-shift comes."""
    g = np.random.default_rng(42)
    return [_request(g, 0, 20, 3, 10), _request(g, 1, 24, 5, 12, voice_match=True), _request(g, 2, 5, 2, 4), _request(g, 3, 3, 1, 4),
            _request(g, 4, 6, 0, 3), _request(g, 5, 4, 1, 2), _request(g, 6, 3, 2, 5), _request(g, 7, 9, 3, 2)]


@functools.lru_cache(maxsize=None)
def _served(wdt, rng, lanes):
    """The workload through one batcher (lanes = 0: the option off); per request (codes, audio), the stats and what the run covered."""
    loop = _loop(wdt)
    reqs = _workload()
    kw = dict(overlap_admission=True, prefill_lanes=lanes) if lanes else {}
    bat = loop.serve(max_batch=2, rng=rng, sampler=_sampler(), seed=SEED, **kw)
    futs = [bat.submit(max_audio_length_ms=80 * f, seed=(100 + i) if rng == "host" else None, stream_id=50 + i, **r)
            for i, (r, f) in enumerate(zip(reqs, FRAMES))]
    began, seated, rows, down_under_prefill, joined_running = {}, {}, {}, False, False
    while True:
        down, live_before = bat.stats["shifts_down"], {s.stream_id for s in bat._live()}
        held = bool(lanes) and len(bat._inflight) > 0
        more = bat.step()
        for s in (bat._inflight if lanes else []):
            began.setdefault(s.stream_id, bat.stats["frames"])
        for s in bat._live():
            if s.stream_id not in seated:
                seated[s.stream_id], rows[s.stream_id] = bat.stats["frames"], s.row
                joined_running |= bool(live_before)
        down_under_prefill |= held and bat.stats["shifts_down"] > down
        if not (more or bat._queue or bat._inflight):
            break
    res = [f.result(timeout=0) for f in futs]
    stats = dict(bat.stats)
    bat.close()
    delays = [seated[i] - began[i] for i in began if i in seated]
    cover = dict(down_under_prefill=down_under_prefill, joined_running=joined_running, max_delay=max(delays) if delays else 0,
                 reused=len(set(rows.values())) < len(rows))
    return [(r.codes.cpu().numpy(), r.audio.cpu()) for r in res], stats, cover


@functools.lru_cache(maxsize=None)
def _solo(wdt, rng, i):
    loop = _loop(wdt)
    req = _workload()[i]
    prompt = loop.prompt_frames(req["context"], req["text"], req["speaker"], voice_match=req["voice_match"])
    how = dict(seed=100 + i) if rng == "host" else dict(seed=SEED, rng="device", stream_ids=[50 + i])
    ref = loop.generate_batch([prompt], max_audio_length_ms=80 * FRAMES[i], sampler=_sampler(), **how)
    return ref.codes[0][:, : ref.frames[0]].cpu().numpy(), ref.audio[0].cpu()


@pytest.mark.parametrize("rng", ["host", "device"])
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_served_through_a_lane_equals_the_solo_runs_and_the_option_off(wdt, rng):
    got, stats, cover = _served(wdt, rng, 1)
    off, off_stats, _ = _served(wdt, rng, 0)
    print("coverage", cover, {k: stats[k] for k in ("frames", "shifts_up", "shifts_down", "overlapped_admissions")})
    assert stats["overlapped_admissions"] == stats["admissions"] == len(FRAMES) and off_stats["overlapped_admissions"] == 0
    assert cover["joined_running"] and cover["reused"]           # admission into a running batch, row reuse
    assert cover["max_delay"] >= 3                               # a commit several frames behind its prefill
    assert stats["shifts_up"] >= 2 and stats["shifts_down"] >= 1  # (the bare move of the first admission, then) an up-shift at a commit
    assert cover["down_under_prefill"]                           # a down-shift while a request was held in the lane
    for i, ((codes, audio), (ocodes, oaudio)) in enumerate(zip(got, off)):
        scodes, saudio = _solo(wdt, rng, i)
        np.testing.assert_array_equal(codes, scodes, err_msg=f"request {i} against its solo run")
        np.testing.assert_array_equal(codes, ocodes, err_msg=f"request {i} against the option off")
        assert torch.equal(audio, saudio) and torch.equal(audio, oaudio), i


def test_two_lanes_give_the_results_of_one():
    one, _, _ = _served("float32", "device", 1)
    two, stats, _ = _served("float32", "device", 2)
    assert stats["overlapped_admissions"] == len(FRAMES)
    for i, ((c1, a1), (c2, a2)) in enumerate(zip(one, two)):
        np.testing.assert_array_equal(c2, c1, err_msg=f"request {i}")
        assert torch.equal(a2, a1), i


# ---- 3. the other request kinds ---------------------------------------------------------------------------------------------------------------
def _mixed(loop, overlap):
    """A plain request, two `prefix=` requests and a three-turn session (the second turn streamed, a heard turn before the third) in a batch of
    three rows; every result as (codes, audio), and the streamed turn's chunks."""
    from mlx_audio_amd.sesame import Segment

    g = np.random.default_rng(43)
    ctx = [Segment(speaker=2, text=g.integers(0, 300, 4).tolist(), audio=(0.3 * g.standard_normal(1920 * 3)).astype(np.float32))]
    heard = Segment(speaker=1, text=g.integers(0, 300, 3).tolist(), audio=(0.3 * g.standard_normal(1920 * 4)).astype(np.float32))
    texts = [g.integers(0, 300, n).tolist() for n in (4, 3, 2)]
    kw = dict(overlap_admission=True, prefill_lanes=1) if overlap else {}
    bat = loop.serve(max_batch=3, rng="device", sampler=_sampler(), seed=SEED, stream_chunk_frames=3, stream_max_frames=16, **kw)
    vp = loop.voice_prefix(ctx)
    side = [bat.submit(None, None, prompt=_frames(g, 5, 1), max_audio_length_ms=80 * 40, stream_id=80)]
    for _ in range(2):
        bat.step()
    sess = bat.session(speaker=0)
    out, chunks = [], None
    for t, text in enumerate(texts):
        side.append(bat.submit(prefix=vp, text=g.integers(0, 300, 2).tolist(), speaker=2, max_audio_length_ms=80 * (5 + t), stream_id=81 + t))
        if t == 2:
            sess.hear(heard)
        if t == 1:
            stream = sess.submit_stream(text, max_audio_length_ms=80 * 8, stream_id=51)
            _drive(bat, stream.future)
            chunks, res = list(stream), stream.result(timeout=0)
        else:
            fut = sess.submit(text, max_audio_length_ms=80 * 8, stream_id=50 + t)
            _drive(bat, fut)
            res = fut.result(timeout=0)
        out.append(res)
    bat.run_until_idle()
    out += [f.result(timeout=0) for f in side]
    stats = dict(bat.stats)
    assert [t[2] for t in sess.turns] == [8, 8, 0, 8]
    sess.close()
    bat.close()
    vp.close()
    return [(r.codes.cpu().numpy(), r.audio.cpu()) for r in out], chunks, stats


def test_prefix_session_and_streaming_requests_through_the_lane_equal_the_option_off():
    loop = _loop("float32")
    off, off_chunks, off_stats = _mixed(loop, False)
    got, chunks, stats = _mixed(loop, True)
    assert stats["overlapped_admissions"] == stats["admissions"] == 7 and off_stats["admissions"] == 7
    assert stats["session_admissions"] == 3 and stats["prefixed_admissions"] == off_stats["prefixed_admissions"] == 3 + 2 and stats["captures"] == 3
    for i, ((c, a), (oc, oa)) in enumerate(zip(got, off)):
        np.testing.assert_array_equal(c, oc, err_msg=f"result {i}")
        assert torch.equal(a, oa), i
    assert [(c.first_frame, c.frames, c.final) for c in chunks] == [(0, 3, False), (3, 3, False), (6, 2, True)]
    cat = torch.cat([c.audio for c in chunks]).cpu()
    assert torch.equal(cat, got[1][1]) and torch.equal(cat, torch.cat([c.audio for c in off_chunks]).cpu())


def test_row_samplers_and_a_seed_of_the_requests_own_through_the_lane():
    """Two samplers in one batch of two rows and three requests, the third with a seed of its own: each against its own
    `generate_batch([prompt], sampler=its own, seed=its own)` and against the option off."""
    loop = _loop("float32")
    g = np.random.default_rng(44)
    prompts = [_frames(g, 6, 2), _frames(g, 4, 1), _frames(g, 9, 3)]
    how = [(_sampler(temp=0.7, top_p=0.9, top_k=0), SEED), (_sampler(temp=0.0), SEED), (_sampler(temp=1.1, top_k=5), 77)]
    frames = [12, 9, 10]

    def run(overlap):
        kw = dict(overlap_admission=True) if overlap else {}
        bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, row_samplers=True, **kw)
        futs = [bat.submit(None, None, prompt=p, max_audio_length_ms=80 * f, sampler=sp, seed=sd, stream_id=60 + i)
                for i, (p, f, (sp, sd)) in enumerate(zip(prompts, frames, how))]
        bat.run_until_idle()
        out = [f.result(timeout=0) for f in futs]
        n = bat.stats["overlapped_admissions"]
        bat.close()
        return [(r.codes.cpu().numpy(), r.audio.cpu()) for r in out], n

    (got, n), (off, _) = run(True), run(False)
    assert n == 3
    for i, ((c, a), (oc, oa)) in enumerate(zip(got, off)):
        ref = loop.generate_batch([prompts[i]], max_audio_length_ms=80 * frames[i], sampler=how[i][0], seed=how[i][1], rng="device", stream_ids=[60 + i])
        np.testing.assert_array_equal(c, ref.codes[0][:, : ref.frames[0]].cpu().numpy(), err_msg=f"request {i} against its solo run")
        np.testing.assert_array_equal(c, oc, err_msg=f"request {i} against the option off")
        assert torch.equal(a, ref.audio[0].cpu()) and torch.equal(a, oa), i


# ---- 4. the real head geometry ---------------------------------------------------------------------------------------------------------------
def test_real_head_geometry_transfer_across_a_key_chunk_edge():
    """8 kv heads x 64 on a short stack, bf16 weight mode, 256 slots: the single-token attention is attn_decode_kernel with key chunks of 128.  B
    (120 keys of its own) is prefilled in the lane, transferred beside a running stream at a non-zero pad, and crosses the chunk edge after 8
    frames; a slot is 2 KiB here, so its transfer is 15 pieces of 16 KiB per layer and K / V."""
    from mlx_audio_amd.sesame import Model

    cfg = P.csm_config()
    cfg = dict(cfg, text_vocab_size=500, audio_vocab_size=1100, audio_num_codebooks=6, max_seq_len=256,
               backbone=dict(cfg["backbone"], num_layers=2, intermediate=1024), decoder=dict(cfg["decoder"], num_layers=2, intermediate=768))
    loop = Model(cfg, weights=_bf16(P.csm_synth_checkpoint(cfg, 2)), weight_dtype="bfloat16")
    g = np.random.default_rng(10)
    prompts = [_frames(g, 20, 120, n_cb=6, text_vocab=500, audio_vocab=1100), _frames(g, 30, 90, n_cb=6, text_vocab=500, audio_vocab=1100)]
    frames = [40, 20]
    bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED, decode=False, overlap_admission=True)
    futs = [bat.submit(None, None, prompt=prompts[0], max_audio_length_ms=80 * frames[0], stream_id=50)]
    for _ in range(7):
        bat.step()
    futs.append(bat.submit(None, None, prompt=prompts[1], max_audio_length_ms=80 * frames[1], stream_id=51))
    while not bat._rows[1]:
        assert bat.step()
    pad, pos = loop.model.row_state()
    assert pad[0] == 0 and pos - pad[1] == 120 + 1 and pad[1] > 0
    bat.run_until_idle()
    assert bat.stats["overlapped_admissions"] == 2
    for i in range(2):
        got = futs[i].result(timeout=0)
        ref = loop.generate_batch([prompts[i]], max_audio_length_ms=80 * frames[i], sampler=_sampler(), seed=SEED, rng="device", stream_ids=[50 + i],
                                  decode=False)
        assert got.frames == ref.frames[0] == frames[i]
        np.testing.assert_array_equal(got.codes.cpu().numpy(), ref.codes[0][:, : ref.frames[0]].cpu().numpy())
    bat.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_transfer_refusals_are_decided_on_the_host():
    from mlx_audio_amd.csm import SesameModel

    w = P.csm_synth_checkpoint(_ccfg(), 3)
    main = SesameModel(_ccfg(), w)
    lane, bare = main.share(), main.share()
    lib = main.lib

    def raw(m, row, src, src_row):
        return lib.kk_csm_admit_transfer(m._h, None, row, src._h, None, src_row)

    def refused(m, row, src, src_row, text):
        state = [x.row_state() for x in (main, lane) if x.caches_are_enabled()]
        assert raw(m, row, src, src_row) != 0 and text in lib.kk_last_error(), (text, lib.kk_last_error())
        assert [x.row_state() for x in (main, lane) if x.caches_are_enabled()] == state

    refused(main, 0, lane, 0, b"kk_csm_setup_caches")  # no caches on either side
    main.setup_caches(3)
    refused(main, 0, lane, 0, b"kk_csm_setup_caches")  # none in the source
    lane.setup_caches(1)
    refused(lane, 0, bare, 0, b"kk_csm_setup_caches")
    main.reset_caches_parked()
    main.shift(9)
    g = np.random.default_rng(46)
    main.admit(1, *_frames(g, 4, 2))
    lane.reset_caches_parked()
    assert main.row_state() == ([MAX_POS, 3, MAX_POS], 9) and lane.row_state() == ([MAX_POS], 0)
    refused(main, 0, main, 1, b"same generator")
    for row in (-1, 3):
        refused(main, row, lane, 0, b"row out of range")
    for row in (-1, 1):
        refused(main, 0, lane, row, b"source row out of range")
    refused(main, 0, lane, 0, b"the source row is parked")
    lane.reset_caches()  # the classic reset: the row is live and holds nothing
    refused(main, 0, lane, 0, b"holds no position")
    lane.reset_caches_parked()
    lane.shift(12)
    lane.admit(0, *_frames(g, 8, 4))
    assert lane.row_state() == ([0], 12)
    refused(main, 1, lane, 0, b"the row is live")
    refused(main, 0, lane, 0, b"kk_csm_shift_caches by 3 first")  # L = 12 > P = 9
    other = SesameModel(_ccfg(), w)  # the same numbers, another weight set
    other.setup_caches(1)
    other.reset_caches_parked()
    other.shift(5)
    other.admit(0, *_frames(g, 3, 2))
    refused(main, 0, other, 0, b"different weight sets")
    for args in ((0, main, 1), (3, lane, 0), (0, lane, 1), (1, lane, 0), (0, lane, 0), (0, other, 0)):
        with pytest.raises(ValueError):
            main.admit_transfer(*args)
    assert main.row_state() == ([MAX_POS, 3, MAX_POS], 9) and lane.row_state() == ([0], 12)
    main.shift(3)
    main.admit_transfer(0, lane, 0)  # and now it is legal
    assert main.row_state() == ([0, 6, MAX_POS], 12) and lane.row_state() == ([0], 12)
    torch.cuda.synchronize()
