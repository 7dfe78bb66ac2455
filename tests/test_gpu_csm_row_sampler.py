"""Per-row sampler settings (kk_op_csm_sample_rows, kk_csm_set_row_sampler, kk_csm_generate_frame_rows, generate_batch(sampler=[...])).  The
yardstick is the shipped launch-argument kernels: row b of a table-mode launch picks what kk_op_csm_sample_ex / kk_csm_generate_frame_ex pick
for that row alone with the entry's values as launch arguments.  Every comparison is array equality."""
import ctypes as CT
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import test_gpu_csm_sampler as SM  # noqa: E402  (VS, the logit rows and the B = 1 yardstick call)
import test_gpu_csm_serve as TS  # noqa: E402  (the tiny generator: vocab 64, 4 code books, max_seq_len 128)

pytestmark = pytest.mark.gpu

VS = sorted(set(SM.VS) | {2051})
TEMP = 0.8
# one setting per row: arg-max; select path (20, 64); full path (65, whole vocabulary, top-p, min-p with min_keep, top-k + top-p)
SETTINGS = [dict(temp=0.0, top_k=50), dict(temp=TEMP, top_k=20), dict(temp=TEMP, top_k=64), dict(temp=TEMP, top_k=65), dict(temp=TEMP, top_k=0),
            dict(temp=TEMP, top_k=0, top_p=0.9), dict(temp=TEMP, top_k=0, min_p=0.05, min_keep=3), dict(temp=TEMP, top_k=30, top_p=0.8)]
SEEDS = [11, 2**40 + 5, 7, 2**63 + 1, 99, 3, 12345678901234, 42]
SIDS = [5, 0, 77, 2**31 - 1, 9, 1, 300, 4]
POS = [0, 17, 3, 1000, 64, 2, 9, 31]


def _sample_rows(lg_dev, samplers, u=None, sid=None, pos=None):
    from mlx_audio_amd import _lib

    lib = _lib.load()
    B, V = lg_dev.shape
    arr = (_lib.KKCsmSampler * B)(*samplers)
    out = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    dev = lambda a, dt: None if a is None else torch.tensor(np.asarray(a), dtype=dt, device="cuda")  # noqa: E731
    ud, sd, pd = dev(u, torch.float32), dev(sid, torch.int32), dev(pos, torch.int32)
    ptr = lambda t: None if t is None else CT.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.kk_op_csm_sample_rows(CT.c_void_p(torch.cuda.current_stream().cuda_stream), B, V, CT.c_void_p(lg_dev.data_ptr()), arr, ptr(ud), ptr(sd), ptr(pd),
                                   CT.c_void_p(out.data_ptr()))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _solo_rows(d, samplers, u=None, sid=None, pos=None):
    """the yardstick: every row alone through kk_op_csm_sample_ex with its sampler as launch arguments"""
    one = lambda a, b: None if a is None else [a[b]]  # noqa: E731
    return np.array([SM._sample_ex(d[b : b + 1], samplers[b], one(u, b), one(sid, b), one(pos, b))[0] for b in range(d.shape[0])])


@pytest.mark.parametrize("V", VS)
def test_rows_equal_the_launch_argument_kernels_row_by_row(V):
    lg = SM._rows(V)
    B = lg.shape[0]
    assert B == len(SETTINGS)
    d = torch.tensor(lg, device="cuda")
    u = np.random.default_rng(V).uniform(size=B).astype(np.float32)
    host = [SM._sampler(**s) for s in SETTINGS]
    want = _solo_rows(d, host, u)
    got = _sample_rows(d, host, u)
    np.testing.assert_array_equal(got, want, err_msg="injected uniforms")
    assert got.min() >= 0 and got.max() < V
    # the device generator: a seed, a stream id and a position of its own per row
    devs = [SM._sampler(**s, seed=SEEDS[b], device_rng=True) for b, s in enumerate(SETTINGS)]
    want_d = _solo_rows(d, devs, None, SIDS, POS)
    np.testing.assert_array_equal(_sample_rows(d, devs, None, SIDS, POS), want_d, err_msg="device rng")
    # slot independence: the same rows in reversed order
    r = slice(None, None, -1)
    dr = torch.tensor(lg[r].copy(), device="cuda")
    np.testing.assert_array_equal(_sample_rows(dr, host[r], u[r].copy()), want[r], err_msg="reversed, injected uniforms")
    np.testing.assert_array_equal(_sample_rows(dr, devs[r], None, SIDS[r], POS[r]), want_d[r], err_msg="reversed, device rng")
    # no uniform source: every row is arg-max, whatever its entry says
    np.testing.assert_array_equal(_sample_rows(d, host), _solo_rows(d, host), err_msg="no uniforms")


@pytest.mark.parametrize("V", [1100, 4000])
def test_wall_fallback_beside_a_full_row_and_a_nan_row(V):
    """A select-type row whose top 100 logits are exactly equal (more than 64 candidates: the round-based fallback) shares the launch with a
    full-vocabulary row, a NaN row and an arg-max row."""
    rng = np.random.default_rng(V + 1)
    lg = rng.standard_normal((4, V)).astype(np.float32)
    lg[0, rng.choice(V, 100, replace=False)] = 7.5
    lg[2, :] = np.nan
    d = torch.tensor(lg, device="cuda")
    host = [SM._sampler(0.9, 50), SM._sampler(0.9, 0, top_p=0.9), SM._sampler(0.9, 50), SM._sampler(0.0, 50)]
    for u0 in (0.03, 0.5, 0.97):
        u = np.array([u0, 1.0 - u0, u0, u0], np.float32)
        got = _sample_rows(d, host, u)
        np.testing.assert_array_equal(got, _solo_rows(d, host, u), err_msg=f"u {u0}")
        assert got.min() >= 0 and got.max() < V
    both = [SM._sampler(0.9, 50), SM._sampler(0.9, 0, top_p=0.9), SM._sampler(0.9, 0, min_p=0.1), SM._sampler(0.9, 50)]
    lg[3] = lg[0]
    d = torch.tensor(lg, device="cuda")
    u = np.array([0.6, 0.6, 0.6, 0.2], np.float32)
    np.testing.assert_array_equal(_sample_rows(d, both, u), _solo_rows(d, both, u))  # a NaN row on the full path, two walls in one launch


def test_refusals_of_the_op():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    d = torch.zeros((2, 67), device="cuda")
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = CT.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in ([SM._sampler(0.5, 5), SM._sampler(-1.0, 5)], [SM._sampler(0.5, 5), SM._sampler(0.5, 5, top_p=1.5)],
                [SM._sampler(0.5, 5, device_rng=True), SM._sampler(0.5, 5)]):
        arr = (_lib.KKCsmSampler * 2)(*bad)
        assert lib.kk_op_csm_sample_rows(st, 2, 67, CT.c_void_p(d.data_ptr()), arr, None, None, None, CT.c_void_p(out.data_ptr())) != 0


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------------
B, NCB, VOCAB, S0 = 3, 4, 64, 5


def _mk(temp, top_k=0, top_p=0.0, min_p=0.0):
    from mlx_audio_amd.sesame import make_sampler

    return make_sampler(temp=temp, top_k=top_k, top_p=top_p, min_p=min_p)


def _prompt_block(seed):
    g = np.random.default_rng(seed)
    tok = np.zeros((B, S0, NCB + 1), np.int32)
    msk = np.zeros((B, S0, NCB + 1), np.float32)
    tok[:, :, -1], msk[:, :, -1] = g.integers(0, 300, (B, S0)), 1
    return tok, msk


def _run(csm, frames, graph, how, change=None, logits=False):
    """The prompt block, then `frames` single-token frames; `how(i)` = the keywords of frame i's generate_frame call.  `change` = (i, fn): fn()
    runs in front of frame i.  Returns codes [frames + 1, B, n_cb] (and the frames' logits [frames + 1, n_cb, B, V])."""
    tok, msk = _prompt_block(3)
    csm.set_graph_mode(graph)
    curr, cmask = tok, msk
    out, lgs = [], []
    for i in range(frames + 1):
        if change is not None and change[0] == i:
            change[1]()
        c = csm.generate_frame(curr, cmask, **how(i)).clone()
        out.append(c.cpu().numpy())
        if logits:
            lgs.append(csm.debug_logits().cpu().numpy())
        curr = torch.zeros((B, 1, NCB + 1), dtype=torch.int32, device=csm.device)
        curr[:, 0, :NCB] = c
        cmask = torch.zeros((B, 1, NCB + 1), dtype=torch.float32, device=csm.device)
        cmask[:, 0, :NCB] = 1
    return (np.stack(out), np.stack(lgs)) if logits else np.stack(out)


def _uniforms(n):
    return np.random.default_rng(77).uniform(size=(n, B, NCB)).astype(np.float32)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_one_sampler_in_every_row_equals_the_launch_argument_frame(wdt, graph):
    csm = TS._loop(wdt).model
    frames = 7  # (graph mode: the third single-token frame and every later one is a replay)
    U = _uniforms(frames + 1)
    for sp in (_mk(0.8, 20), _mk(1.1, 0, top_p=0.9)):
        csm.setup_caches(B)
        want = _run(csm, frames, graph, lambda i: dict(sampler=sp, uniforms=U[i]))
        csm.reset_caches()
        for b in range(B):
            csm.set_row_sampler(b, sp)
        got = _run(csm, frames, graph, lambda i: dict(sampler="rows", uniforms=U[i]))
        np.testing.assert_array_equal(got, want)
        # the device generator: one seed in every entry = the launch's seed word
        csm.reset_caches()
        want = _run(csm, frames, graph, lambda i: dict(sampler=sp, seed=2**33 + 9, stream_ids=[4, 9, 2]))
        csm.reset_caches()
        for b in range(B):
            csm.set_row_sampler(b, sp, seed=2**33 + 9)
        got = _run(csm, frames, graph, lambda i: dict(sampler="rows", device_rng=True, stream_ids=[4, 9, 2]))
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_a_row_changes_its_sampler_between_two_replays(wdt):
    csm = TS._loop(wdt).model
    frames, at = 8, 5  # frames 1 .. 8 are single-token frames; the change lands in front of frame 5, after replays 3 and 4
    U = _uniforms(frames + 1)
    rows = [_mk(0.0, 50), _mk(0.8, 20), _mk(1.1, 0, top_p=0.9)]
    other = _mk(0.9, 0, min_p=0.05)

    def start():
        csm.setup_caches(B)
        for b in range(B):
            csm.set_row_sampler(b, rows[b])

    how = lambda i: dict(sampler="rows", uniforms=U[i])  # noqa: E731
    start()
    base = _run(csm, frames, True, how)
    start()
    got, lgs = _run(csm, frames, True, how, change=(at, lambda: csm.set_row_sampler(1, other)), logits=True)
    np.testing.assert_array_equal(got[:at], base[:at])
    np.testing.assert_array_equal(got[:, [0, 2]], base[:, [0, 2]])  # the other rows: as without the change
    sp = SM._sampler(other.temp, other.top_k, other.top_p, other.min_p, other.min_tokens_to_keep)
    old = SM._sampler(rows[1].temp, rows[1].top_k)
    differs = False
    for i in range(at, frames + 1):
        for cb in range(NCB):
            lg = torch.tensor(lgs[i, cb, 1:2], device="cuda")
            assert got[i, 1, cb] == SM._sample_ex(lg, sp, [U[i, 1, cb]])[0], (i, cb)
            differs = differs or got[i, 1, cb] != SM._sample_ex(lg, old, [U[i, 1, cb]])[0]
    assert differs  # (the new entry is what was read: somewhere the old one would have picked another code)


@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_a_zeroed_table_is_argmax(wdt):
    csm = TS._loop(wdt).model
    U = _uniforms(4)
    csm.setup_caches(B)  # zeroes the table
    want = _run(csm, 3, False, lambda i: dict(temperature=0.0, uniforms=U[i]))
    csm.setup_caches(B)
    got = _run(csm, 3, False, lambda i: dict(sampler="rows", uniforms=U[i]))
    np.testing.assert_array_equal(got, want)
    assert got.min() >= 0 and got.max() < VOCAB
    with pytest.raises(ValueError):
        csm.set_row_sampler(B, _mk(0.5, 5))
    with pytest.raises(ValueError):
        csm.set_row_sampler(0, type("S", (), dict(temp=-1.0, top_k=5))())


@pytest.mark.parametrize("rng", ["host", "device"])
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
def test_generate_batch_with_a_sampler_per_prompt_equals_the_solo_runs(wdt, rng):
    loop = TS._loop(wdt)
    g = np.random.default_rng(12)
    reqs = [TS._request(g, 0, 4, 0, 3), TS._request(g, 1, 5, 2, 4), TS._request(g, 2, 3, 1, 2)]  # ragged prompts
    prompts = [loop.prompt_frames(r["context"], r["text"], r["speaker"], voice_match=r["voice_match"]) for r in reqs]
    samplers = [_mk(0.0, 50), _mk(0.8, 20), _mk(1.1, 0, top_p=0.9)]
    seeds, sids = [5, 600, 2**40 + 7], [50, 51, 52]
    kw = dict(max_audio_length_ms=80 * 10, decode=False, rng=rng)
    got = loop.generate_batch(prompts, sampler=samplers, seed=seeds, stream_ids=sids if rng == "device" else None, **kw)
    for i in range(3):
        ref = loop.generate_batch([prompts[i]], sampler=samplers[i], seed=seeds[i], stream_ids=[sids[i]] if rng == "device" else None, **kw)
        n = ref.frames[0]
        assert got.frames[i] == n, i
        np.testing.assert_array_equal(got.codes[i][:, :n].cpu().numpy(), ref.codes[0][:, :n].cpu().numpy(), err_msg=f"item {i}")
