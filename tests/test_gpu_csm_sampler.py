"""The CSM sampler on the device (kk_op_csm_sample_ex, kk_op_csm_uniforms, generate_frame(sampler=...), rng="device") against the float64
restatement of its rule and the integer restatement of its RNG in tests/_sampler_ref.py."""
import ctypes as CT
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _sampler_ref as R  # noqa: E402
import mlx_audio_amd.params as P  # noqa: E402

pytestmark = pytest.mark.gpu

VS = [67, 1100, 2051, 4000]
U_TOP = np.float32(1.0) - np.float32(2.0**-24)  # the largest float below 1


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _rows(V):
    """The rows of test_csm_sampler_matches_oracle_incl_tie_walls, a peaked row (scale 6) and a flat one."""
    rng = np.random.default_rng(V)
    rows = [rng.standard_normal(V) * 3, np.round(rng.standard_normal(V) * 2) / 2, np.zeros(V), np.round(rng.standard_normal(V)),
            np.where(rng.uniform(size=V) < 0.5, -np.inf, rng.standard_normal(V)), -np.abs(rng.standard_normal(V)) * 50,
            rng.standard_normal(V) * 6, rng.standard_normal(V) * 0.05]
    return np.stack(rows).astype(np.float32)


def _sampler(temp, top_k=0, top_p=0.0, min_p=0.0, min_keep=1, seed=0, device_rng=False):
    from mlx_audio_amd import _lib

    return _lib.KKCsmSampler(float(temp), int(top_k), float(top_p), float(min_p), int(min_keep), int(seed), 1 if device_rng else 0)


def _sample_ex(lg_dev, sp, u=None, sid=None, pos=None):
    from mlx_audio_amd import _lib

    lib = _lib.load()
    B, V = lg_dev.shape
    out = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    dev = lambda a, dt: None if a is None else torch.tensor(np.asarray(a), dtype=dt, device="cuda")  # noqa: E731
    ud, sd, pd = dev(u, torch.float32), dev(sid, torch.int32), dev(pos, torch.int32)
    ptr = lambda t: None if t is None else CT.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.kk_op_csm_sample_ex(CT.c_void_p(torch.cuda.current_stream().cuda_stream), B, V, CT.c_void_p(lg_dev.data_ptr()), CT.byref(sp), ptr(ud),
                                 ptr(sd), ptr(pd), CT.c_void_p(out.data_ptr()))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _uniforms(B, ncb, seed, sid=None, pos=None):
    from mlx_audio_amd import _lib

    lib = _lib.load()
    out = torch.zeros((B, ncb), dtype=torch.float32, device="cuda")
    sd = None if sid is None else torch.tensor(np.asarray(sid), dtype=torch.int32, device="cuda")
    pd = None if pos is None else torch.tensor(np.asarray(pos), dtype=torch.int32, device="cuda")
    rc = lib.kk_op_csm_uniforms(CT.c_void_p(torch.cuda.current_stream().cuda_stream), B, ncb, CT.c_uint64(seed),
                                None if sd is None else CT.c_void_p(sd.data_ptr()), None if pd is None else CT.c_void_p(pd.data_ptr()),
                                CT.c_void_p(out.data_ptr()))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V", VS)
def test_default_path_did_not_move(V):
    """Filters off, top_k in 1..64, injected uniforms: kk_op_csm_sample_ex gives kk_op_csm_sample's picks bit for bit."""
    from mlx_audio_amd import _lib

    lib = _lib.load()
    lg = _rows(V)
    B = lg.shape[0]
    d = torch.tensor(lg, device="cuda")
    rng = np.random.default_rng(_seed("default", V))
    for temp, top_k in ((0.9, 5), (0.9, 50), (0.7, 64), (0.0, 50)):
        for _ in range(4):
            u = rng.uniform(size=B).astype(np.float32)
            ud = torch.tensor(u, device="cuda")
            old = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            rc = lib.kk_op_csm_sample(CT.c_void_p(torch.cuda.current_stream().cuda_stream), B, V, CT.c_void_p(d.data_ptr()), temp, top_k,
                                      CT.c_void_p(ud.data_ptr()), CT.c_void_p(old.data_ptr()))
            assert rc == 0, lib.kk_last_error()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_sample_ex(d, _sampler(temp, top_k), u), old.cpu().numpy(), err_msg=f"temp {temp} top_k {top_k}")


def _clear_top_p(before, top_p, margin):
    """The value nearest to top_p with no cumulative within `margin` of it (None: the row has none within +-0.05)."""
    for k in range(0, 500):
        for s in (+1, -1):
            t = top_p + s * k * 1e-4
            if 0.0 < t < 1.0 and np.abs(before - t).min() > margin:
                return t
    return None


def _clear_min_p(ratio, min_p):
    """The value nearest to min_p such that no p / p_max lies within a relative 1e-4 of it."""
    for k in range(0, 2000):
        for s in (+1, -1):
            t = min_p * (1.0 + s * k * 3e-4)
            if 0.0 < t <= 1.0 and np.abs(ratio / t - 1.0).min() > 1e-4:
                return t
    return None


CASES = [dict(top_k=0), dict(top_k=200), dict(top_k="V"),
         dict(top_k=0, top_p=0.5), dict(top_k=200, top_p=0.8), dict(top_k="V", top_p=0.95),
         dict(top_k=0, min_p=0.02), dict(top_k=200, min_p=0.1), dict(top_k="V", min_p=0.02),
         dict(top_k=0, top_p=0.95, min_p=0.02), dict(top_k=200, top_p=0.8, min_p=0.1), dict(top_k="V", top_p=0.5, min_p=0.1),
         dict(top_k=50, top_p=0.8, min_p=0.02), dict(top_k=50, top_p=0.5), dict(top_k=50, min_p=0.1),
         dict(top_k=0, min_p=0.9, min_keep=3)]


@pytest.mark.parametrize("V", VS)
def test_exact_picks_with_constructed_inputs(V):
    """One row per launch, so that every row gets thresholds of its own.  A parallel float32 sum of n positive terms is within (n - 1) 2^-24
    of the exact one (2.4e-4 at n = 4000), hence the margins: the target sits at the midpoint of a kept token's CDF interval and only intervals
    at least 1e-3 wide are used (the first token, the last kept one, up to 8 others); top_p moves to the nearest value with no cumulative
    within 5e-4, min_p to the nearest with no p / p_max within a relative 1e-4.  On the all-equal row every weight is exactly 1 and float32
    sums of ones are exact, so its top_p only has to keep a quarter of a step (0.25 / V) away from a cumulative.  Where a row offers no such
    top_p at all (the flat row at large V: steps of 1 / V < 5e-4), or no interval that wide, the pick of a target in the first half of the
    kept set must be a member of the kept set.  u = the largest float below 1: the last kept token where its interval is that wide, and
    always a member of the kept set."""
    lg = _rows(V)
    exact = loose = 0
    for b in range(lg.shape[0]):
        d = torch.tensor(lg[b : b + 1], device="cuda")
        order, p, dist = R.sorted_row(lg[b])
        before = np.concatenate([[0.0], np.cumsum(p)[:-1]])
        all_equal = bool(np.ptp(lg[b]) == 0)
        for case in CASES:
            temp = 0.9 if case.get("top_p", 0) != 0.5 else 0.7
            kw = dict(top_k=V if case["top_k"] == "V" else case["top_k"], top_p=case.get("top_p", 0.0), min_p=case.get("min_p", 0.0),
                      min_keep=case.get("min_keep", 1))
            cut_ok = True
            if kw["top_p"]:
                t = _clear_top_p(before, kw["top_p"], 0.25 / V if all_equal else 5e-4)
                cut_ok = t is not None
                kw["top_p"] = t if cut_ok else kw["top_p"]
            if kw["min_p"]:
                t = _clear_min_p(p / p[0], kw["min_p"])
                if t is None:  # (a ratio of exactly 1 everywhere: the all-equal row keeps everything for every min_p <= 1)
                    assert all_equal
                else:
                    kw["min_p"] = t
            n = R.kept(lg[b], **kw)[0]
            if case.get("min_keep") and b in (0, 6):  # (the random rows: this min_p alone keeps fewer than the three tokens asked for)
                assert R.kept(lg[b], **dict(kw, min_keep=1))[0] < 3 == n, (b, kw)
            keptset = set(order[:n].tolist())
            sp = _sampler(temp, kw["top_k"], kw["top_p"], kw["min_p"], kw["min_keep"])
            c = np.concatenate([[0.0], R.cdf(dist, n, temp)])
            wide = [j for j in range(n) if c[j + 1] - c[j] >= 1e-3]
            if cut_ok and wide:
                others = [j for j in wide if j not in (0, n - 1)]
                sel = sorted(set([j for j in (0, n - 1) if j in wide] + [others[i] for i in np.linspace(0, len(others) - 1, min(8, len(others))).astype(int)]))
                for j in sel:
                    got = int(_sample_ex(d, sp, [np.float32(0.5 * (c[j] + c[j + 1]))])[0])
                    assert got == order[j], (V, b, kw, j, got, int(order[j]))
                    exact += 1
            else:
                j = max(0, n // 2 - 1)
                got = int(_sample_ex(d, sp, [np.float32(0.5 * (c[j] + c[j + 1]) * 0.5)])[0])
                assert got in keptset, (V, b, kw, got)
                loose += 1
            if cut_ok:
                got = int(_sample_ex(d, sp, [U_TOP])[0])
                assert got in keptset, (V, b, kw, got)
                if (n - 1) in wide:
                    assert got == order[n - 1], (V, b, kw, got, int(order[n - 1]))
    print(f"V {V}: {exact} exact picks, {loose} membership-only cases")
    assert exact >= 8 * len(CASES)


@pytest.mark.parametrize("V", VS)
def test_tie_walls_straddling_a_cut_and_nan_rows(V):
    """A cut inside a tie keeps the lower indices: on the all-equal row and the quantised rows, top_k alone (a count: exact) at a temperature
    that keeps the kept tokens' intervals wide; every kept token of the tie is reachable and no other.  A row with NaNs gives codes in
    [0, V) on every path."""
    lg = _rows(V)
    for b, top_k, temp in ((2, 200, 1.0), (2, 65, 0.5), (1, 100, 4.0), (3, 150, 4.0)):
        order = R.sorted_row(lg[b])[0]
        ks = [k for k in range(min(top_k, V - 1), 64, -1) if lg[b][order[k - 1]] == lg[b][order[k]]]  # the nearest cut inside a tie, above the one-wave path's 64
        if not ks:
            assert V == 67 and b != 2  # (66 sorted values of a small quantised row may end in singletons; the all-equal row always has a wall)
            continue
        top_k = ks[0]
        d = torch.tensor(lg[b : b + 1], device="cuda")
        n, order, p, dist = R.kept(lg[b], top_k=top_k)
        assert n == top_k and lg[b][order[n - 1]] == lg[b][order[n]]
        c = np.concatenate([[0.0], R.cdf(dist, n, temp)])
        sp = _sampler(temp, top_k)
        tail = [j for j in range(max(0, n - 6), n) if c[j + 1] - c[j] >= 1e-3]
        assert tail, (V, b)
        for j in tail:
            assert int(_sample_ex(d, sp, [np.float32(0.5 * (c[j] + c[j + 1]))])[0]) == order[j]
        assert int(_sample_ex(d, sp, [U_TOP])[0]) == order[n - 1]
    rng = np.random.default_rng(_seed("nan", V))
    odd = lg.copy()
    odd[:, rng.integers(0, V, V // 3)] = np.nan
    odd[0, :] = np.nan
    odd[1, : V // 2] = -np.inf
    odd[2, 0] = np.inf
    d = torch.tensor(odd, device="cuda")
    for sp in (_sampler(0.9, 50), _sampler(0.9, 0), _sampler(0.9, 200, 0.9, 0.05), _sampler(0.9, 50, 0.9), _sampler(0.0, 50), _sampler(0.9, 0, 0.5, 0.0, 4)):
        for u in (0.0, 0.3, float(U_TOP)):
            got = _sample_ex(d, sp, np.full(odd.shape[0], u, np.float32))
            assert ((got >= 0) & (got < V)).all(), got


@pytest.mark.parametrize("V", VS)
def test_same_inputs_same_codes_in_every_run_and_slot(V):
    lg = _rows(V)
    B = lg.shape[0]
    rng = np.random.default_rng(_seed("det", V))
    d = torch.tensor(lg, device="cuda")
    for sp in (_sampler(0.9, 0, 0.95, 0.01), _sampler(0.8, 200), _sampler(1.1, 50, 0.9)):
        u = rng.uniform(size=B).astype(np.float32)
        first = _sample_ex(d, sp, u)
        for _ in range(19):
            np.testing.assert_array_equal(_sample_ex(d, sp, u), first)
        for shift in (1, 3, 5):  # the same rows in other batch slots
            perm = np.roll(np.arange(B), shift)
            np.testing.assert_array_equal(_sample_ex(torch.tensor(lg[perm], device="cuda"), sp, u[perm]), first[perm])
        for b in (0, B - 1):  # and alone
            np.testing.assert_array_equal(_sample_ex(torch.tensor(lg[b : b + 1], device="cuda"), sp, u[b : b + 1]), first[b : b + 1])


def test_device_uniforms_equal_the_philox_restatement_bit_for_bit():
    for seed in (0, 1, _seed("u"), 2**64 - 1, 2**63 + 12345):
        sid, pos = [0, 7, 3, 11, 2**31 - 1, 5], [0, 1, 77, 2047, 300, 2**20]
        got = _uniforms(6, 32, seed, sid, pos)
        want = np.array([[R.device_uniform(seed, s, p, cb) for cb in range(32)] for s, p in zip(sid, pos)], np.float32)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert ((got > 0) & (got < 1)).all()
    np.testing.assert_array_equal(_uniforms(3, 4, 9), np.array([[R.device_uniform(9, b, 0, cb) for cb in range(4)] for b in range(3)], np.float32))
    # the sampling kernels draw exactly these: device RNG == injection of the reported uniform (both kernels)
    lg = _rows(1100)
    d = torch.tensor(lg, device="cuda")
    B = lg.shape[0]
    sid, pos = list(range(10, 10 + B)), list(range(100, 100 + B))
    u0 = _uniforms(B, 1, 42, sid, pos)[:, 0]
    for temp, top_k, top_p in ((0.9, 50, 0.0), (0.9, 0, 0.95)):
        a = _sample_ex(d, _sampler(temp, top_k, top_p, seed=42, device_rng=True), None, sid, pos)
        np.testing.assert_array_equal(a, _sample_ex(d, _sampler(temp, top_k, top_p), u0))
        assert not np.array_equal(a, _sample_ex(d, _sampler(temp, top_k, top_p, seed=43, device_rng=True), None, sid, pos))


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------------
def _prompt(cfg, rng, B, n_text, n_audio):
    n = cfg["audio_num_codebooks"]
    S = n_text + n_audio
    tok = np.zeros((B, S, n + 1), np.int64)
    msk = np.zeros((B, S, n + 1), np.float32)
    tok[:, :n_text, -1] = rng.integers(0, cfg["text_vocab_size"], (B, n_text))
    msk[:, :n_text, -1] = 1
    tok[:, n_text:, :n] = rng.integers(0, cfg["audio_vocab_size"], (B, n_audio, n))
    msk[:, n_text:, :n] = 1
    return tok, msk


def _run_frames(model, tok, msk, us, graph, logits=False, **kw):
    """Prompt block + len(us) single-token frames; returns codes [1 + F][B][n] (and the logits of every frame)."""
    B, n = tok.shape[0], tok.shape[2] - 1
    model.reset_caches()
    model.set_graph_mode(graph)
    codes = [model.generate_frame(torch.tensor(tok), torch.tensor(msk), uniforms=torch.tensor(us[0]), **kw).clone()]
    lgs = [model.debug_logits().clone()] if logits else []
    for i in range(1, len(us)):
        t_in = torch.zeros((B, 1, n + 1), dtype=torch.int32, device="cuda")
        t_in[:, 0, :n] = codes[-1]
        m_in = torch.zeros((B, 1, n + 1), dtype=torch.float32, device="cuda")
        m_in[:, 0, :n] = 1
        codes.append(model.generate_frame(t_in, m_in, uniforms=torch.tensor(us[i]), **kw).clone())
        if logits:
            lgs.append(model.debug_logits().clone())
    torch.cuda.synchronize()
    out = torch.stack(codes).cpu().numpy()
    return (out, torch.stack(lgs).cpu().numpy()) if logits else out


def _bf16(w):
    return {k: torch.tensor(np.asarray(v, np.float32)).to(torch.bfloat16).float().numpy() for k, v in w.items()}


@pytest.mark.parametrize("size", ["tiny", "tiny300", "full_width"])
def test_generate_frame_with_default_sampler_equals_temperature_top_k_call(size):
    """generate_frame(sampler=Sampler(0.9, 50)) with injected uniforms == the temperature=0.9, top_k=50 call bit for bit, eager and graph
    replay; on the full-width short stack (V = 2051, 32 code books, bf16 weights) also a full-vocabulary top-p run whose codes are in range."""
    from mlx_audio_amd.csm import SesameModel
    from mlx_audio_amd.sesame import Sampler

    if size == "full_width":
        cfg = P.csm_config()
        cfg = dict(cfg, backbone=dict(cfg["backbone"], num_layers=2), decoder=dict(cfg["decoder"], num_layers=1), max_seq_len=64)
        model = SesameModel(cfg, _bf16(P.csm_synth_checkpoint(cfg, 0)), weight_dtype="bfloat16")
    else:
        cfg = P.csm_tiny_config() if size == "tiny" else dict(P.csm_tiny_config(), audio_vocab_size=300)
        model = SesameModel(cfg, P.csm_synth_checkpoint(cfg, 2))
    B, n, V = 3, cfg["audio_num_codebooks"], cfg["audio_vocab_size"]
    rng = np.random.default_rng(_seed("default-frame", size))
    model.setup_caches(B)
    tok, msk = _prompt(cfg, rng, B, 6, 3)
    us = rng.uniform(size=(5, B, n)).astype(np.float32)
    want = _run_frames(model, tok, msk, us, False, temperature=0.9, top_k=50)
    np.testing.assert_array_equal(_run_frames(model, tok, msk, us, False, sampler=Sampler(0.9, 50)), want)
    for _ in range(3):  # eager, capture, replay
        got = _run_frames(model, tok, msk, us, True, sampler=Sampler(0.9, 50))
    np.testing.assert_array_equal(got, want)
    if size == "full_width":
        for graph in (False, True, True, True):
            c = _run_frames(model, tok, msk, us, graph, sampler=Sampler(0.9, 0, top_p=0.9, min_p=0.02))
            assert ((c >= 0) & (c < V)).all()
        assert not np.array_equal(c, want)  # (another sampler: other codes; the graph cache keys on every sampler field)


def _admissible_share(logits, codes, us, sampler, V):
    """Every code against the float64 rule with thresholds and target moved by +-d, d = V 2^-24; returns (violations, share of ambiguous picks)."""
    d = V * 2.0**-24
    bad, ambiguous, total = [], 0, 0
    F, n, B = logits.shape[0], logits.shape[1], logits.shape[2]
    for f in range(F):
        for i in range(n):
            for b in range(B):
                ok = R.admissible(logits[f, i, b], sampler.temp, us[f, b, i], d, top_k=sampler.top_k, top_p=sampler.top_p, min_p=sampler.min_p,
                                  min_keep=sampler.min_tokens_to_keep)
                total += 1
                ambiguous += len(ok) > 1
                if int(codes[f, b, i]) not in ok:
                    bad.append((f, i, b, int(codes[f, b, i]), sorted(ok)))
    return bad, ambiguous / total


def test_full_vocabulary_sampler_in_the_frame_loop_against_debug_logits():
    """V = 300 tiny configuration, Sampler(0.9, 0, top_p=0.9, min_p=0.02), injected uniforms, eager and graph replay: every code is checked after
    the fact against debug_logits() of its own frame -- it must be in the set of codes the float64 rule admits when the cut thresholds and
    the target each move by +-d, d = V 2^-24 = 1.8e-5 (the worst-case relative error of a float32 sum of V positive terms in any order).
    A pick whose set has more than one member shows nothing; their share is capped at 5 % (the targets that can be ambiguous cover at
    most 2 d per kept boundary, <= 2 V d = 1.1 % of the uniforms).  On the CPU, with CsmOracle's logits for this seed driven by the float64
    rule (3 streams, prompt block + 11 frames, 4 code books = 144 picks; kept sets of 1 to 46 tokens), 0 of the 144 picks are ambiguous."""
    from mlx_audio_amd.csm import SesameModel
    from mlx_audio_amd.sesame import Sampler

    cfg = dict(P.csm_tiny_config(), audio_vocab_size=300)
    model = SesameModel(cfg, P.csm_synth_checkpoint(cfg, 2))
    B, n, V = 3, cfg["audio_num_codebooks"], 300
    rng = np.random.default_rng(_seed("admissible", V))
    model.setup_caches(B)
    tok, msk = _prompt(cfg, rng, B, 6, 3)
    us = rng.uniform(size=(12, B, n)).astype(np.float32)
    sampler = Sampler(0.9, 0, top_p=0.9, min_p=0.02)
    for graph in (False, True, True, True):
        codes, logits = _run_frames(model, tok, msk, us, graph, logits=True, sampler=sampler)
        bad, share = _admissible_share(logits, codes, us, sampler, V)
        print(f"graph {graph}: {len(bad)} inadmissible codes, ambiguous share {share:.4f}")
        assert not bad, bad[:5]
        assert share <= 0.05, share
    kept_sizes = [R.kept(logits[f, i, b], top_p=0.9, min_p=0.02)[0] for f in range(12) for i in range(n) for b in range(B)]
    assert min(kept_sizes) < V  # the filters did cut


def _ragged_loop(wdt="float32"):
    from mlx_audio_amd.mimi import Mimi, MimiConfig
    from mlx_audio_amd.sesame import Model, Segment

    ccfg = dict(P.csm_tiny_config(), audio_vocab_size=64, audio_num_codebooks=4, max_seq_len=128)
    mcfg = P.mimi_tiny_config()
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 3, encode=True))
    loop = Model(ccfg, mimi=mimi, weights=P.csm_synth_checkpoint(ccfg, 3), weight_dtype=wdt)
    rng = np.random.default_rng(19)
    ctxs, texts = [], []
    for b, (na, nt) in enumerate(((3, 4), (1, 9), (5, 2))):
        audio = (0.3 * rng.standard_normal(1920 * na)).astype(np.float32)
        ctxs.append([Segment(speaker=b, text=rng.integers(0, 300, 5).tolist(), audio=audio)])
        texts.append(rng.integers(0, 300, nt).tolist())
    prompts = [loop.prompt_frames(ctxs[b], texts[b], b, voice_match=(b == 1)) for b in range(3)]
    assert len({p[0].shape[0] for p in prompts}) > 1
    return loop, prompts, ctxs, texts


@pytest.mark.parametrize("sampler_kw", [dict(temp=0.8, top_k=20), dict(temp=0.8, top_k=0, top_p=0.9)])
def test_device_rng_makes_a_stream_independent_of_its_batch(sampler_kw):
    """generate_batch(rng="device", seed, stream_ids=[7, 3, 11]) on ragged prompts == three B = 1 runs with stream ids [7], [3], [11], bit
    for bit, with no uniforms callback and graph replay on; another seed gives other codes; and the codes are those of injecting the
    uniforms kk_op_csm_uniforms reports for (seed, stream id, the stream's own position, code book)."""
    from mlx_audio_amd.sesame import make_sampler

    loop, prompts, _, _ = _ragged_loop()
    n, F = 4, 7
    seed = _seed("device-rng")
    sids = [7, 3, 11]
    kw = dict(max_audio_length_ms=80 * F, sampler=make_sampler(**sampler_kw), stop_on_eos=False)
    both = loop.generate_batch(prompts, rng="device", seed=seed, stream_ids=sids, **kw)
    assert both.frames == [F] * 3
    for b in range(3):
        one = loop.generate_batch([prompts[b]], rng="device", seed=seed, stream_ids=[sids[b]], **kw)
        np.testing.assert_array_equal(both.codes[b].cpu().numpy(), one.codes[0].cpu().numpy())
        assert torch.equal(both.audio[b], one.audio[0])
    again = loop.generate_batch(prompts, rng="device", seed=seed, stream_ids=sids, **kw)
    np.testing.assert_array_equal(again.codes.cpu().numpy(), both.codes.cpu().numpy())
    other = loop.generate_batch(prompts, rng="device", seed=seed + 1, stream_ids=sids, **kw)
    assert not np.array_equal(other.codes.cpu().numpy(), both.codes.cpu().numpy())
    moved = loop.generate_batch(prompts[::-1], rng="device", seed=seed, stream_ids=sids[::-1], **kw)  # the same streams in other slots
    np.testing.assert_array_equal(moved.codes.cpu().numpy()[::-1], both.codes.cpu().numpy())
    # frame i of stream b is generated at the stream's own position len(prompt b) + i
    lens = [p[0].shape[0] for p in prompts]
    host = loop.generate_batch(prompts, uniforms=lambda i: _uniforms(3, n, seed, sids, [L + i for L in lens]), **kw)
    np.testing.assert_array_equal(host.codes.cpu().numpy(), both.codes.cpu().numpy())


def test_model_generate_with_top_p_sampler_and_device_rng_yields_audio():
    from mlx_audio_amd.sesame import make_sampler

    loop, _, ctxs, texts = _ragged_loop()
    kw = dict(context=ctxs[0], voice_match=False, max_audio_length_ms=80 * 5, sampler=make_sampler(0.8, top_p=0.95, top_k=0), rng="device", seed=1,
              stop_on_eos=False)
    res = list(loop.generate(texts[0], **kw))
    assert len(res) == 1 and res[0].token_count == 5 and res[0].samples == 5 * 1920 and bool(torch.isfinite(res[0].audio).all())
    parts = list(loop.generate(texts[0], stream=True, streaming_interval=0.16, **kw))
    assert [p.token_count for p in parts] == [2, 2, 1] and sum(p.samples for p in parts) == res[0].samples
