"""Shared voice prefixes of CSM streams (kk_csm_prefix_create / kk_csm_admit_prefixed, `Model.voice_prefix`, `CSMBatcher.submit(prefix=)`,
`Model.generate(cache_context=True)`): a stream admitted on top of a prefix's K / V carries, bit for bit, the frames, codes and waveform of
`generate_batch([prompt_frames(context, text, voice_match=False)])` alone -- for every weight format, both RNGs, suffix blocks of 1, 2, 3 and 17
frames, wherever in a running batch it lands.  No tolerance anywhere: every comparison is array equality."""
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
MAX_POS = 128


def _bf16(w):
    return {k: torch.tensor(np.asarray(v, np.float32)).to(torch.bfloat16).float().numpy() for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _loop(wdt):
    """The tiny generator + codec; wdt "float32", "bfloat16", or "q8" (an 8-bit checkpoint that stays packed on the device)."""
    from mlx_audio_amd import quant
    from mlx_audio_amd.mimi import Mimi, MimiConfig
    from mlx_audio_amd.sesame import Model

    ccfg = dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=4, max_seq_len=MAX_POS)
    mcfg = P.mimi_tiny_config()
    cw = P.csm_synth_checkpoint(ccfg, 3)
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 3, encode=True))
    if wdt == "q8":
        qw = quant.quantize_checkpoint(cw, 64, 8, names=quant.csm_quantised_layer_names(cw, 64))
        loop = Model(dict(ccfg, quantization={"group_size": 64, "bits": 8}), mimi=mimi, weights=qw)
        assert loop.model.weight_format == "q8" and loop.model.weight_fallback is None
        return loop
    if wdt == "bfloat16":
        cw = _bf16(cw)
    return Model(ccfg, mimi=mimi, weights=cw, weight_dtype=wdt)


def _context(rng, speaker, n_text, n_audio):
    """One reference segment: n_text + n_audio + 1 (EOS) prompt frames (n_audio 0: text only, n_text frames)."""
    from mlx_audio_amd.sesame import Segment

    audio = (0.3 * rng.standard_normal(1920 * n_audio)).astype(np.float32) if n_audio else None
    return [Segment(speaker=speaker, text=rng.integers(0, 300, n_text).tolist(), audio=audio)]


def _plain(rng, speaker, n_ctx_text, n_audio, n_text):
    return dict(context=_context(rng, speaker, n_ctx_text, n_audio), text=rng.integers(0, 300, n_text).tolist(), speaker=speaker, voice_match=False)


def _sampler():
    from mlx_audio_amd.sesame import make_sampler

    return make_sampler(temp=TEMP, top_k=TOP_K)


def _solo(loop, req, frames, rng, seed, sid, decode=True):
    """The yardstick: the WHOLE prompt (context, then text) run alone."""
    prompt = req["prompt"] if "prompt" in req else loop.prompt_frames(req["context"], req["text"], req["speaker"], voice_match=False)
    if rng == "host":
        return loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=_sampler(), seed=seed, decode=decode)
    return loop.generate_batch([prompt], max_audio_length_ms=80 * frames, sampler=_sampler(), seed=SEED, rng="device", stream_ids=[sid], decode=decode)


def _submit(bat, rng, i, req, frames, vp=None):
    kw = dict(max_audio_length_ms=80 * frames, seed=(100 + i) if rng == "host" else None, stream_id=50 + i)
    if vp is not None:
        return bat.submit(prefix=vp, text=req["text"], speaker=req["speaker"], **kw)
    return bat.submit(**kw, **req)


def _check(loop, rng, reqs, frames, results, names=None, decode=True):
    for i, (req, f, fut) in enumerate(zip(reqs, frames, results)):
        got = fut.result(timeout=0)
        ref = _solo(loop, req, f, rng, 100 + i, 50 + i, decode)
        tag = f"stream {names[i] if names else i}"
        assert got.frames == ref.frames[0], tag
        np.testing.assert_array_equal(got.codes.cpu().numpy(), ref.codes[0][:, : ref.frames[0]].cpu().numpy(), err_msg=tag)
        if decode:
            assert torch.equal(got.audio, ref.audio[0]), tag


def _on(ctx, rng, speaker, n_text):
    """A request whose context is `ctx` (what a voice prefix of `ctx` stands for)."""
    return dict(context=ctx, text=rng.integers(0, 300, n_text).tolist(), speaker=speaker, voice_match=False)


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt,rng", [("float32", "host"), ("float32", "device"), ("bfloat16", "host"), ("bfloat16", "device"), ("q8", "device")])
def test_a_stream_on_a_prefix_equals_its_whole_prompt_run_alone(wdt, rng):
    """Suffix blocks of 1, 2, 3 and 17 frames (one and two rows are what the single-token kernels would take), each stream alone in the batch."""
    loop = _loop(wdt)
    g = np.random.default_rng(21)
    ctx = _context(g, 1, 5, 6)
    reqs = [_on(ctx, g, 1, s) for s in (1, 2, 3, 17)]
    frames = [9, 8, 10, 7]
    vp = loop.voice_prefix(ctx)
    assert vp.length == 5 + 6 + 1 and vp.prefix.nbytes == 2 * 2 * 12 * 128 * 4
    bat = loop.serve(max_batch=1, rng=rng, sampler=_sampler(), seed=SEED)
    futs = [_submit(bat, rng, i, reqs[i], frames[i], vp) for i in range(4)]
    bat.run_until_idle()
    assert bat.stats["prefixed_admissions"] == 4
    _check(loop, rng, reqs, frames, futs, ["S=1", "S=2", "S=3", "S=17"])
    vp.close()


# ---- placement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_admitted_on_a_prefix_into_a_running_batch(wdt):
    """Two plain streams run; after 5 frames a prefixed one (and a plain one behind it) join at a non-zero pad."""
    loop = _loop(wdt)
    g = np.random.default_rng(22)
    ctx = _context(g, 2, 4, 5)
    reqs = [_plain(g, 0, 5, 3, 4), _plain(g, 1, 6, 2, 3), _on(ctx, g, 2, 2), _plain(g, 3, 3, 1, 2)]
    frames = [14, 12, 9, 8]
    vp = loop.voice_prefix(ctx)
    bat = loop.serve(max_batch=4, rng="device", sampler=_sampler(), seed=SEED)
    futs = [_submit(bat, "device", i, reqs[i], frames[i]) for i in (0, 1)]
    for _ in range(5):
        assert bat.step()
    pad, pos = loop.model.row_state()
    futs += [_submit(bat, "device", 2, reqs[2], frames[2], vp), _submit(bat, "device", 3, reqs[3], frames[3])]
    bat.step()
    pad2, pos2 = loop.model.row_state()
    assert pos2 == pos + 1 and pad2[:2] == pad[:2] and pad2[2] == pos - (vp.length + 2) > 0  # the row's window holds prefix + suffix
    bat.run_until_idle()
    assert bat.stats["admissions"] == 4 and bat.stats["prefixed_admissions"] == 1
    _check(loop, "device", reqs, frames, futs, "ABCD")


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_admitted_on_a_prefix_into_a_reused_row_over_stale_keys(wdt):
    loop = _loop(wdt)
    g = np.random.default_rng(23)
    ctx = _context(g, 2, 3, 3)
    reqs = [_plain(g, 0, 6, 6, 6), _plain(g, 1, 5, 2, 3), _on(ctx, g, 2, 1)]  # A's prompt (19 frames) is longer than D's prefix + suffix (8)
    frames = [6, 30, 12]
    vp = loop.voice_prefix(ctx)
    bat = loop.serve(max_batch=2, rng="host", sampler=_sampler())
    futs = [_submit(bat, "host", 0, reqs[0], frames[0]), _submit(bat, "host", 1, reqs[1], frames[1]), _submit(bat, "host", 2, reqs[2], frames[2], vp)]
    bat.run_until_idle()
    a, b, d = (f.result(timeout=0) for f in futs)
    assert d.row == a.row != b.row
    _check(loop, "host", reqs, frames, futs, "ABD")


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_prefixed_rows_across_a_down_shift_and_an_up_shift(wdt):
    """A session that passes max_seq_len slots with prefixed rows live at the down-shift, and a prefixed request whose prefix + suffix is longer
    than the position (the live window moves up first)."""
    loop = _loop(wdt)
    g = np.random.default_rng(24)
    ctx = _context(g, 1, 4, 6)  # 11 frames
    vp = loop.voice_prefix(ctx)
    reqs = [_plain(g, 0, 3, 0, 3), _on(ctx, g, 1, 3), _on(ctx, g, 1, 2), _plain(g, 2, 4, 2, 3), _on(ctx, g, 1, 17), _on(ctx, g, 1, 1)]
    frames = [40, 50, 70, 30, 30, 30]
    use = [None, vp, vp, None, vp, vp]
    bat = loop.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED)
    futs = [_submit(bat, "device", 0, reqs[0], frames[0])]
    bat.step()
    assert loop.model.row_state() == ([0, MAX_POS], 7)
    futs.append(_submit(bat, "device", 1, reqs[1], frames[1], vp))  # 11 + 3 = 14 > P = 7: up by 7
    bat.step()
    assert bat.stats["shifts_up"] == 2 and loop.model.row_state() == ([7, 0], 15)
    futs += [_submit(bat, "device", i, reqs[i], frames[i], use[i]) for i in range(2, 6)]
    moved_prefixed = 0
    prev = loop.model.row_state()
    while bat.step() or bat._queue:
        now = loop.model.row_state()
        if now[1] < prev[1]:
            moved_prefixed += sum(1 for s in bat._live() if s.prefix is not None)
        prev = now
    assert bat.stats["shifts_down"] >= 1 and moved_prefixed >= 1 and bat.stats["prefixed_admissions"] == 4
    _check(loop, "device", reqs, frames, futs)


# ---- sharing -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_two_streams_share_one_prefix_object_which_stays_unchanged(wdt):
    loop = _loop(wdt)
    g = np.random.default_rng(25)
    ctx = _context(g, 3, 6, 4)
    reqs, frames = [_on(ctx, g, 3, 4), _on(ctx, g, 3, 7)], [15, 11]
    vp = loop.voice_prefix(ctx)
    before = vp.prefix.save().clone()
    assert before.numel() == 2 * 2 * vp.length * 128 and bool(before.abs().sum() > 0)
    bat = loop.serve(max_batch=2, rng="host", sampler=_sampler())
    futs = [_submit(bat, "host", i, reqs[i], frames[i], vp) for i in range(2)]
    bat.step()
    assert len(bat._live()) == 2  # both run at once, on the same object
    bat.run_until_idle()
    _check(loop, "host", reqs, frames, futs, "AB")
    assert torch.equal(vp.prefix.save(), before)


def test_a_prefix_serves_the_shares_of_its_model():
    loop = _loop("bfloat16")
    g = np.random.default_rng(26)
    ctx = _context(g, 0, 5, 3)
    req = _on(ctx, g, 0, 3)
    vp = loop.voice_prefix(ctx)
    other = loop.share()
    bat = other.serve(max_batch=2, rng="device", sampler=_sampler(), seed=SEED)
    fut = _submit(bat, "device", 0, req, 10, vp)
    bat.run_until_idle()
    _check(other, "device", [req], [10], [fut])


# ---- prefix_create beside live streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_prefix_create_while_streams_are_live_leaves_them_alone(wdt):
    loop = _loop(wdt)
    g = np.random.default_rng(27)
    ctx = _context(g, 1, 7, 6)
    reqs, frames = [_plain(g, 0, 5, 3, 4), _plain(g, 2, 4, 2, 6)], [16, 13]

    def run(with_prefix):
        bat = loop.serve(max_batch=3, rng="device", sampler=_sampler(), seed=SEED)
        futs = [_submit(bat, "device", i, reqs[i], frames[i]) for i in range(2)]
        for _ in range(4):
            bat.step()
        state = loop.model.row_state()
        if with_prefix:
            vp = loop.voice_prefix(ctx)  # Mimi.encode + the prefix block, between two replays of the captured frame step
            assert loop.model.row_state() == state
            bat.step()
            vp.close()
        bat.run_until_idle()
        return [f.result(timeout=0) for f in futs]

    plain, beside = run(False), run(True)
    for a, b in zip(plain, beside):
        assert a.frames == b.frames and torch.equal(a.codes, b.codes) and torch.equal(a.audio, b.audio)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_decided_on_the_host():
    """Live row, row out of range, n + S > P, a prefix of another weight set, a null and a destroyed prefix, a workspace too small: the library
    answers before any launch (the pointers handed over are stand-ins) and the state is unchanged."""
    from mlx_audio_amd import _lib
    from mlx_audio_amd.csm import SesameModel

    ccfg = dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=4, max_seq_len=MAX_POS)
    model = SesameModel(ccfg, P.csm_synth_checkpoint(ccfg, 3))
    stranger = SesameModel(ccfg, P.csm_synth_checkpoint(ccfg, 3))  # the same numbers, another weight set
    lib, h = model.lib, model._h
    sp = _lib.KKCsmSampler(0.0, 0, 0.0, 0.0, 1, 0, 0)
    buf = torch.zeros(1 << 20, dtype=torch.int32, device="cuda")
    ptr = ctypes.c_void_p(buf.data_ptr())
    tok, msk = np.zeros((6, 5), np.int32), np.zeros((6, 5), np.float32)
    msk[:, -1] = 1
    pre, foreign = model.make_prefix(tok, msk), stranger.make_prefix(tok, msk)
    assert pre.length == 6 and lib.kk_csm_prefix_length(pre._h) == 6 and pre.nbytes == 2 * 2 * 6 * 128 * 4

    def raw(row, prefix_h, S, ws_bytes=buf.numel() * 4):
        return lib.kk_csm_admit_prefixed(h, None, row, prefix_h, S, ptr, ptr, ctypes.byref(sp), None, 0, ptr, ws_bytes, ptr)

    def err():
        return lib.kk_last_error()

    assert raw(0, pre._h, 2) != 0 and b"kk_csm_setup_caches" in err()  # no caches
    model.setup_caches(3)
    model.reset_caches_parked()
    model.shift(7)
    state = ([MAX_POS] * 3, 7)
    assert raw(0, pre._h, 2) != 0 and b"longer than the cache position" in err()  # 6 + 2 > 7
    with pytest.raises(ValueError):
        model.admit(0, tok[:2], msk[:2], prefix=pre)
    for row in (-1, 3):
        assert raw(row, pre._h, 1) != 0 and b"row out of range" in err()
    with pytest.raises(ValueError):
        model.admit(3, tok[:1], msk[:1], prefix=pre)
    assert raw(0, foreign._h, 1) != 0 and b"another weight set" in err()
    with pytest.raises(ValueError):
        model.admit(0, tok[:1], msk[:1], prefix=foreign)
    assert raw(0, None, 1) != 0 and b"null or destroyed prefix" in err()
    assert raw(0, pre._h, 1, ws_bytes=64) != 0 and b"workspace too small" in err()
    assert lib.kk_csm_prefix_create(h, None, 6, ptr, ptr, ptr, 64, ctypes.byref(ctypes.c_void_p())) != 0 and b"workspace too small" in err()
    assert lib.kk_csm_prefix_create(h, None, MAX_POS, ptr, ptr, ptr, buf.numel() * 4, ctypes.byref(ctypes.c_void_p())) != 0
    assert model.row_state() == state
    codes = model.admit(1, tok[:1], msk[:1], prefix=pre)  # 6 + 1 = 7 = P
    assert codes.shape == (4,) and model.row_state() == ([MAX_POS, 0, MAX_POS], 7)
    assert raw(1, pre._h, 1) != 0 and b"the row is live" in err()
    with pytest.raises(ValueError):
        model.admit(1, tok[:1], msk[:1], prefix=pre)
    dead = ctypes.c_void_p(foreign._h.value)
    foreign.close()
    assert raw(0, dead, 1) != 0 and b"null or destroyed prefix" in err()
    assert lib.kk_csm_prefix_length(dead) == -1 and lib.kk_csm_prefix_bytes(dead) == 0
    with pytest.raises(ValueError):
        model.admit(0, tok[:1], msk[:1], prefix=foreign)
    assert model.row_state() == ([MAX_POS, 0, MAX_POS], 7)
    torch.cuda.synchronize()


# ---- Model.generate -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt,rng", [("float32", "host"), ("bfloat16", "device")])
def test_generate_with_cache_context_equals_generate_without(wdt, rng):
    loop = _loop(wdt)
    g = np.random.default_rng(28)
    ctx = _context(g, 1, 5, 6)
    lines = [g.integers(0, 300, n).tolist() for n in (4, 1, 9)]
    kw = dict(speaker=1, context=ctx, voice_match=False, sampler=_sampler(), max_audio_length_ms=80 * 10, seed=77, rng=rng)
    loop._seed_counter = 0
    ref = list(loop.generate(lines, **kw))
    loop._seed_counter = 0
    got = list(loop.generate(lines, cache_context=True, **kw))
    assert len(ref) == len(got) == 3
    for a, b in zip(ref, got):
        assert a.token_count == b.token_count and torch.equal(a.audio, b.audio)
    with pytest.raises(ValueError):
        next(loop.generate(lines, cache_context=True, **dict(kw, voice_match=True)))


# ---- the real head geometry ---------------------------------------------------------------------------------------------------------------------
def test_real_head_geometry_prefix_across_a_key_chunk_edge():
    """llama-1B / llama-100M head geometry (32 heads / 8 kv heads / hd 64) on a short stack, bf16 weight mode, 256 cache slots: the prefix is 120
    positions, the streams on it pass the 128-key chunk edge of attn_decode_kernel within their first frames -- one of them beside a plain
    stream, at a non-zero pad."""
    from mlx_audio_amd.sesame import Model, VoicePrefix

    cfg = P.csm_config()
    cfg = dict(cfg, text_vocab_size=500, audio_vocab_size=1100, audio_num_codebooks=6, max_seq_len=256,
               backbone=dict(cfg["backbone"], num_layers=2, intermediate=1024), decoder=dict(cfg["decoder"], num_layers=2, intermediate=768))
    loop = Model(cfg, weights=_bf16(P.csm_synth_checkpoint(cfg, 2)), weight_dtype="bfloat16")
    g = np.random.default_rng(29)

    def frames_of(n_text, n_audio):
        tok = np.zeros((n_text + n_audio, 7), np.int32)
        msk = np.zeros((n_text + n_audio, 7), np.float32)
        tok[:n_text, -1], msk[:n_text, -1] = g.integers(0, 500, n_text), 1
        tok[n_text:, :6], msk[n_text:, :6] = g.integers(0, 1100, (n_audio, 6)), 1
        return tok, msk

    ptok, pmsk = frames_of(20, 100)
    vp = VoicePrefix(prefix=loop.model.make_prefix(ptok, pmsk), tokens=ptok, mask=pmsk, length=120, root=loop.model.weights_root())
    assert vp.prefix.nbytes == 2 * 2 * 120 * 512 * 4
    texts = [g.integers(0, 500, n).tolist() for n in (5, 2)]
    plain = frames_of(30, 10)
    frames = [30, 20, 24]
    bat = loop.serve(max_batch=3, rng="device", sampler=_sampler(), seed=SEED, decode=False)
    futs = [bat.submit(None, None, prompt=plain, max_audio_length_ms=80 * frames[0], stream_id=50)]
    for _ in range(4):
        bat.step()
    futs.append(bat.submit(prefix=vp, text=texts[0], max_audio_length_ms=80 * frames[1], stream_id=51))  # 125 > P = 44: the plain window moves up
    bat.step()
    pad, pos = loop.model.row_state()
    assert pos == 126 and pad[:2] == [125 - 44 + 0, 0]
    futs.append(bat.submit(prefix=vp, text=texts[1], max_audio_length_ms=80 * frames[2], stream_id=52))  # 122 <= P: pad 4
    bat.step()
    assert loop.model.row_state()[0][2] == 126 - 122
    bat.run_until_idle()
    reqs = [dict(prompt=plain)] + [dict(prompt=(np.concatenate([ptok, t], 0), np.concatenate([pmsk, m], 0)))
                                   for t, m in (loop._tokenize_text_segment(x, 0) for x in texts)]
    _check(loop, "device", reqs, frames, futs, ["plain", "S=5", "S=2"], decode=False)
