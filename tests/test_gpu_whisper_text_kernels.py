"""The decode-step kernels of the Whisper text side (csrc/kk_whisper_text_kernels.hip) on their own, through the raw kk_op_* entries: one-query
attention over a bf16 K/V store, the skinny-M Linear on bf16 weights, the embedding and the token pick, each against a float64 / numpy reference with
a bound derived from the arithmetic, and each for the project's invariant: a row's bits do not depend on the rows beside it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_text_ref as T  # noqa: E402
from _whisper_ref import bf16_round  # noqa: E402

from mlx_audio_amd import _lib, whisper  # noqa: E402

EPS = 2.0 ** -23


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
def _attn(q, kv, k_off, v_off, items, T_rows, ld, item, ln, heads):
    import torch

    lib = _lib.load()
    R = q.shape[0]
    out = torch.full((R, heads * 64), float("nan"), dtype=torch.float32, device="cuda")
    nb = lib.kk_op_whisper_attn_rows_scratch_bytes(R, heads, T_rows)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    rc = lib.kk_op_whisper_attn_rows(_st(), R, heads, _p(q), _p(kv), k_off, v_off, items, T_rows, ld, _p(item), _p(ln), _p(out), _p(scratch), nb)
    return rc, out


@pytest.mark.parametrize("T_rows", [64, 448, 1500])
def test_attention_rows_against_float64(T_rows):
    """R = 5 rows over 3 items, heads = 2, len in {1, 63, 65, T_rows - 1, T_rows} mixed in one call (capped at T_rows), K | V interleaved in one store with
    channel offsets, everything a row may not read NaN when it runs alone, and a NaN row behind the store.  Bound per element: (len + 64 + 8) 2^-23 max|v| of the (item,
    head): the probabilities are exp2 of an fp32 score (a 64-term dot: its rounding moves every probability by a relative 64 ulp at most, scores being
    O(1)), their sum and the P V sum are fp32 sums of len terms with weights that sum to 1, plus a few ulp for v_exp_f32 and the merge of the splits."""
    import torch

    heads, items, ld, k_off, v_off = 2, 3, 2 * 128 + 8, 8, 8 + 128
    g = np.random.default_rng(T_rows)
    lens = [min(x, T_rows) for x in (1, 63, 65, T_rows - 1, T_rows)]
    item = [0, 2, 1, 2, 0]
    q = g.standard_normal((5, heads * 64)).astype(np.float32)
    kv = bf16_round(g.standard_normal((items, T_rows, ld)).astype(np.float32))
    flat = np.concatenate([kv.reshape(-1, ld), np.full((1, ld), np.nan, np.float32)])  # one NaN row behind the last item's T_rows rows
    dev = torch.from_numpy(flat).cuda().bfloat16()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    outs = []
    for r in range(5):  # every row alone, with everything it may not read NaN: the other items, and its own item behind len[r]
        one = torch.full_like(dev, float("nan"))
        lo = item[r] * T_rows
        one[lo: lo + lens[r]] = dev[lo: lo + lens[r]]
        rc, o = _attn(torch.from_numpy(q[r:r + 1]).cuda(), one, k_off, v_off, items, T_rows, ld, i32([item[r]]), i32([lens[r]]), heads)
        assert rc == 0
        outs.append(o.cpu().numpy()[0])
    rc, got = _attn(torch.from_numpy(q).cuda(), dev, k_off, v_off, items, T_rows, ld, i32(item), i32(lens), heads)
    assert rc == 0
    got = got.cpu().numpy()
    worst = 0.0
    for r in range(5):
        assert np.isfinite(outs[r]).all()
        assert np.array_equal(got[r], outs[r]), f"row {r}: bits differ between R = 5 and R = 1"
        for h in range(heads):
            k = kv[item[r], : lens[r], k_off + 64 * h: k_off + 64 * h + 64]
            v = kv[item[r], : lens[r], v_off + 64 * h: v_off + 64 * h + 64]
            ref = T.attn_row(q[r, 64 * h: 64 * h + 64], k, v)
            bound = (lens[r] + 64 + 8) * EPS * float(np.abs(v).max())
            err = float(np.abs(got[r, 64 * h: 64 * h + 64] - ref).max())
            worst = max(worst, err / bound)
            assert err <= bound, (r, h, err, bound)
    print(f"T_rows {T_rows}: worst measured / bound = {worst:.3f}")


def test_attention_rows_refuses_bad_row_tables():
    import torch

    kv = torch.zeros((2, 64, 128), dtype=torch.bfloat16, device="cuda")
    q = torch.zeros((1, 64), dtype=torch.float32, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    lib = _lib.load()
    for item, ln, word in (([0], [0], b"len[0] = 0"), ([0], [65], b"len[0] = 65"), ([2], [1], b"item[0] = 2")):
        rc, _ = _attn(q, kv, 0, 64, 2, 64, 128, i32(item), i32(ln), 1)
        assert rc != 0 and word in lib.kk_last_error(), lib.kk_last_error()
    rc, _ = _attn(q, kv, 0, 96, 2, 64, 128, i32([0]), i32([1]), 1)  # the values would run past the row
    assert rc != 0


# ---- linear ---------------------------------------------------------------------------------------------------------------------------------
def _linear(x, w, bias, act, res, M, N, K, want_f32=True, store=None):
    import torch

    lib = _lib.load()
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda") if want_f32 else None
    ob, ldb, rows, nrows = (None, 0, None, 0) if store is None else store
    rc = lib.kk_op_whisper_linear_rows(_st(), M, N, K, _p(x), x.shape[1], _p(w), _p(bias), act, _p(res), N, _p(out), N, _p(ob), ldb, _p(rows), nrows)
    return rc, out


@pytest.fixture(scope="module")
def lin_data():
    import torch

    data = {}
    for K, N in ((128, 384), (512, 128), (128, 51866), (1280, 200)):
        g = np.random.default_rng(K * 7 + N)
        w = bf16_round((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
        x = g.standard_normal((16, K)).astype(np.float32)
        bias = (0.5 * g.standard_normal(N)).astype(np.float32)
        res = g.standard_normal((16, N)).astype(np.float32)
        xb = bf16_round(x).astype(np.float64)
        acc = xb @ w.astype(np.float64).T  # float64 on x rounded as the kernel rounds it
        mag = np.abs(xb) @ np.abs(w.astype(np.float64)).T
        data[(K, N)] = dict(w=w, x=x, bias=bias, res=res, acc=acc, mag=mag, wd=torch.from_numpy(w).cuda().bfloat16(), xd=torch.from_numpy(x).cuda(),
                            bd=torch.from_numpy(bias).cuda(), rd=torch.from_numpy(res).cuda())
    return data


@pytest.mark.parametrize("K,N", [(128, 384), (512, 128), (128, 51866), (1280, 200)])
def test_linear_rows_against_float64(lin_data, K, N):
    """M in {1, 3, 16}; plain, bias, bias + GELU, bias + residual, bias + GELU + residual.  Bound: (K + 4) 2^-23 (sum_k |x_k w_k| + |bias| + |res|): the matrix
    core's fp32 accumulation of K exact bf16 products in an order of its own, the sixteen waves' partial sums, bias and residual.  The same bound is kept for
    GELU, whose slope is below 1.13 and whose erff adds a few ulp of a value no larger than the sum.  Row 1 of M = 3 equals that row at M = 1 bit for bit."""
    d = lin_data[(K, N)]
    worst = 0.0
    for M in (1, 3, 16):
        for use_bias, act, use_res in ((0, 0, 0), (1, 0, 0), (1, 2, 0), (1, 0, 1), (1, 2, 1)):
            rc, out = _linear(d["xd"][:M].contiguous(), d["wd"], d["bd"] if use_bias else None, act, d["rd"][:M].contiguous() if use_res else None, M, N, K)
            assert rc == 0
            ref = d["acc"][:M] + (d["bias"].astype(np.float64) if use_bias else 0.0)
            if act:
                ref = ref * 0.5 * (1.0 + _erf(ref / np.sqrt(2.0)))
            if use_res:
                ref = ref + d["res"][:M]
            bound = (K + 4) * EPS * (d["mag"][:M] + (np.abs(d["bias"]) if use_bias else 0.0) + (np.abs(d["res"][:M]) if use_res else 0.0))
            err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (M, use_bias, act, use_res, float((err / bound).max()))
    print(f"K {K} N {N}: worst measured / bound = {worst:.3f}")
    x1 = d["xd"][1:2].contiguous()
    _, alone = _linear(x1, d["wd"], d["bd"], 2, None, 1, N, K)
    _, three = _linear(d["xd"][:3].contiguous(), d["wd"], d["bd"], 2, None, 3, N, K)
    assert np.array_equal(alone.cpu().numpy()[0], three.cpu().numpy()[1])


def _erf(a):
    import torch

    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def test_linear_rows_bf16_strided_store(lin_data):
    """the result rounded to bf16 into caller-given rows of a wider store, at a channel offset (how the step's K and V reach the cache); a row index
    outside the store is skipped; rows that are not named stay untouched.  Bound: the fp32 bound plus half a bf16 ulp of the value."""
    import torch

    K, N, M = 512, 128, 3
    d = lin_data[(K, N)]
    store = torch.full((10, 2 * N + 8), -7.0, dtype=torch.bfloat16, device="cuda")
    rows = torch.tensor([7, 2, 99], dtype=torch.int32, device="cuda")
    rc, out = _linear(d["xd"][:M].contiguous(), d["wd"], d["bd"], 0, None, M, N, K, store=(store[:, N:], 2 * N + 8, rows, 10))
    assert rc == 0
    rc, _ = _linear(d["xd"][:M].contiguous(), d["wd"], d["bd"], 0, None, M, N, K, want_f32=False, store=(store[:, N:], 2 * N + 8, rows, 10))
    assert rc == 0
    s = store.float().cpu().numpy()
    ref = d["acc"][:M] + d["bias"]
    f32 = out.cpu().numpy()
    for m, row in ((0, 7), (1, 2)):
        got = s[row, N: 2 * N]
        assert np.array_equal(got, bf16_round(f32[m]))  # the stored value is the fp32 result, rounded to nearest even
        bound = (K + 4) * EPS * (d["mag"][m] + np.abs(d["bias"])) + np.abs(ref[m]) * 2.0 ** -8
        assert (np.abs(got - ref[m]) <= bound).all()
    untouched = np.ones_like(s, bool)
    untouched[7, N: 2 * N] = untouched[2, N: 2 * N] = False
    assert (s[untouched] == -7.0).all()


def test_linear_rows_refuses_17_rows():
    import torch

    x = torch.zeros((17, 32), dtype=torch.float32, device="cuda")
    w = torch.zeros((16, 32), dtype=torch.bfloat16, device="cuda")
    rc, _ = _linear(x, w, None, 0, None, 17, 16, 32)
    assert rc != 0 and b"M <= 16" in _lib.load().kk_last_error()


# ---- embed ----------------------------------------------------------------------------------------------------------------------------------
def test_embed_is_exact_and_clamps_bad_ids():
    import torch

    lib = _lib.load()
    V, D, ctx = 1000, 384, 48
    g = np.random.default_rng(5)
    table = bf16_round(g.standard_normal((V, D)).astype(np.float32))
    pos = g.standard_normal((ctx, D)).astype(np.float32)
    tok = np.array([0, 999, 17, 1000, -3, 2 ** 31 - 1, 5], np.int32)
    at = np.array([0, 47, 3, 1, 2, 48, -1], np.int32)
    out = torch.full((len(tok), D), float("nan"), dtype=torch.float32, device="cuda")
    td, pd, tokd, atd = torch.from_numpy(table).cuda().bfloat16(), torch.from_numpy(pos).cuda(), torch.from_numpy(tok).cuda(), torch.from_numpy(at).cuda()
    rc = lib.kk_op_whisper_embed(_st(), len(tok), D, _p(tokd), _p(atd), _p(td), V, _p(pd), ctx, _p(out))
    assert rc == 0
    want = table[np.clip(tok, 0, V - 1)] + pos[np.clip(at, 0, ctx - 1)]  # fp32 sum of an exact bf16 widening and the fp32 position
    assert np.array_equal(out.cpu().numpy(), want)


# ---- pick -----------------------------------------------------------------------------------------------------------------------------------
def _script(tok, V, g, mi):
    """Per step, the B = 4 rows' logits: random N(0, 2) with the winner the script wants pushed 40 above the rest.  Row 0 walks the timestamp
    grammar (first position -> timestamp, text, closing pair, text, eot, then frozen); row 1 has the timestamps' total probability decide (a flat
    boost of all timestamps, no single one above the best text token); row 2 tries to break every rule (the pushed token is one the filters must
    mask); row 3 ends at once."""
    tb, eot = tok.timestamp_begin, tok.eot
    steps = []
    plan0 = [tb + 3, 1000, tb + 9, tb + 9, 2000, eot, 3000, 4000]
    plan2 = [220, tb + 2, tok.no_timestamps, tb + 1, 1500, tok.sot, tb + 1400, 1234]  # blank at first; then forbidden choices
    plan3 = [tb + (60 if mi is None else mi), eot, 777, tb + 5, 9, 9, 9, 9]
    for s in range(8):
        x = (2.0 * g.standard_normal((4, V))).astype(np.float32)
        x[0, plan0[s]] += 40.0
        x[1, tb:] += np.float32(6.0 if s % 2 == 0 else -6.0)  # even steps: the timestamps' mass wins; odd: the best text token wins
        x[2, plan2[s]] += 40.0
        x[3, plan3[s]] += 40.0
        steps.append(x)
    return steps


@pytest.mark.parametrize("n_vocab,mi", [(51865, 50), (51866, None)])
def test_pick_follows_the_numpy_restatement(n_vocab, mi):
    """A scripted sequence of 8 steps, B = 4: tokens exactly equal to filter_logits + GreedyRow (the logits' top-2 gap after filtering is asserted to be far
    above fp32 round-off), sum_logprob within 1e-5 per step, an ended row emits eot with its sum frozen, the not-ended counter exact after every step."""
    import torch

    lib = _lib.load()
    tok = whisper.special_tokens(T.dims(128, 2, 1, n_vocab, 100))
    g = np.random.default_rng(n_vocab)
    P = T.pick_params(tok, n_vocab, max_initial_timestamp_index=mi)
    sup = (tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm, tok.no_speech, 1500)
    from mlx_audio_amd.whisper_decoding import suppress_bitmask

    B, cap = 4, 16
    params = torch.from_numpy(np.array([P[k] for k in ("n_vocab", "eot", "blank", "no_timestamps", "timestamp_begin", "max_initial_timestamp_index",
                                                        "without_timestamps", "suppress_blank")], np.int32)).cuda()
    bits = torch.from_numpy(suppress_bitmask(n_vocab, sup).view(np.int32)).cuda()
    state = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    tokens = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
    nxt = torch.zeros(B, dtype=torch.int32, device="cuda")
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.kk_op_whisper_pick_reset(_st(), B, _p(state), _p(left)) == 0
    assert int(left.item()) == B
    rows = [T.GreedyRow(tok.eot) for _ in range(B)]
    seen_mass = set()
    for s, x in enumerate(_script(tok, n_vocab, g, mi)):
        xd = torch.from_numpy(x).cuda()
        assert lib.kk_op_whisper_pick(_st(), B, _p(xd), n_vocab, _p(params), _p(bits), _p(state), _p(tokens), cap, _p(nxt), _p(left)) == 0
        for b in range(B):
            f = T.filter_logits(x[b], rows[b].sampled, P, suppress=sup)
            top = np.sort(f[np.isfinite(f)])[-2:]
            assert top[1] - top[0] > 1e-3, "the script's logits must not tie"
            if b == 1:
                seen_mass.add(bool(np.isneginf(f[: tok.timestamp_begin]).all()))
            rows[b].update(f)
        got = nxt.cpu().numpy()
        assert [int(t) for t in got] == [r.sampled[-1] for r in rows], (s, got, [r.sampled[-1] for r in rows])
        assert int(left.item()) == sum(not r.ended for r in rows)
    st = state.cpu().numpy()
    sums = st[:, 5].copy().view(np.float32)
    tk = tokens.cpu().numpy()
    for b in range(B):
        assert list(tk[b, :8]) == rows[b].sampled and (tk[b, 8:] == -1).all()
        assert abs(float(sums[b]) - rows[b].sum_logprob) <= 1e-5 * 8, (b, sums[b], rows[b].sum_logprob)
        assert st[b, 4] == 8 and st[b, 3] == int(rows[b].ended)
    assert seen_mass == {True, False}  # the probability-mass rule fell on both sides
    assert rows[0].sampled[5:] == [tok.eot] * 3 and rows[3].sampled[1:] == [tok.eot] * 7  # ended rows emit eot
    assert rows[2].sampled[0] != 220 and tok.no_timestamps not in rows[2].sampled and tok.sot not in rows[2].sampled and 1500 not in rows[2].sampled
    assert rows[3].sampled[0] == tok.timestamp_begin + (60 if mi is None else mi)


def test_pick_without_timestamps_and_ties():
    """without_timestamps: only blank and suppress apply; equal maxima resolve to the lowest index; a row's choice does not depend on the rows beside it"""
    import torch

    lib = _lib.load()
    V = 51865
    tok = whisper.special_tokens(T.dims(128, 2, 1, V, 100))
    P = T.pick_params(tok, V, without_timestamps=True)
    params = torch.from_numpy(np.array([P[k] for k in ("n_vocab", "eot", "blank", "no_timestamps", "timestamp_begin", "max_initial_timestamp_index",
                                                        "without_timestamps", "suppress_blank")], np.int32)).cuda()
    g = np.random.default_rng(9)
    x = g.standard_normal((3, V)).astype(np.float32)
    x[0, [220, 4000, 51000]] = 9.0  # the blank is masked at the first position; of the tie, the lower index wins
    x[1, [tok.eot, 300]] = [9.0, 8.0]
    x[2, 51864] = 9.0  # the last id of the vocabulary
    res = {}
    for sel in ([0, 1, 2], [1], [2, 0]):
        B = len(sel)
        state = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
        tokens = torch.zeros((B, 4), dtype=torch.int32, device="cuda")
        nxt = torch.zeros(B, dtype=torch.int32, device="cuda")
        left = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.kk_op_whisper_pick_reset(_st(), B, _p(state), _p(left)) == 0
        xd = torch.from_numpy(np.ascontiguousarray(x[sel])).cuda()
        assert lib.kk_op_whisper_pick(_st(), B, _p(xd), V, _p(params), None, _p(state), _p(tokens), 4, _p(nxt), _p(left)) == 0
        st = state.cpu().numpy()
        for j, b in enumerate(sel):
            res.setdefault(b, []).append((int(nxt[j].item()), int(st[j, 5])))  # token and the BITS of sum_logprob
    assert res[0][0][0] == 4000 and res[1][0][0] == 300 and res[2][0][0] == 51864
    assert all(len(set(v)) == 1 for v in res.values())
