"""The beam-search kernels of the Whisper text side (csrc/kk_whisper_text_kernels.hip) on their own, through the raw entries: the top-(K + 1) of a row
against numpy, the select of a window against the restatement (tests/_whisper_beam_ref.py) with the owner tables against parent pointers followed on
the host, the owned attention against the direct one on gathered keys bit for bit, and the refusals.  tests/test_whisper_beam_cpu.py shows that every
decision compared here is decided by at least 1e-3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_beam_ref as BR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import _lib  # noqa: E402
from mlx_audio_amd.whisper_decoding import suppress_bitmask  # noqa: E402

KEYS = ("n_vocab", "eot", "blank", "no_timestamps", "timestamp_begin", "max_initial_timestamp_index", "without_timestamps", "suppress_blank")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _state_rows(histories, tb, sums=None):
    """kk_whisper_pick_state rows of the given sampled histories, as int32 [B][8]"""
    st = np.zeros((len(histories), 8), np.int32)
    for b, h in enumerate(histories):
        seen = [t for t in h if t >= tb]
        st[b, :5] = [h[-1] if h else -1, h[-2] if len(h) > 1 else -1, seen[-1] if seen else -1, 0, len(h)]
        st[b, 5:6] = np.array([0.0 if sums is None else sums[b]], np.float32).view(np.int32)
    return st


@pytest.mark.parametrize("n_vocab", BR.TOPK_VOCABS)
def test_topk_against_numpy(n_vocab):
    """K = 5, ten rows (timestamps on and off, first position and later, a bitmask, planted equal logits, three unmasked tokens, everything masked), the rows
    that share parameters and bitmask in one launch: the tokens equal numpy's on the float64 filters, equal logits by the lower id, never a masked token, -1
    in the unused slots; log-probabilities within 2e-5; and the first offer is the greedy pick's token with its log-probability's bits."""
    import torch

    lib = _lib.load()
    K, C1 = BR.TOPK_K, BR.TOPK_K + 1
    P, rows = BR.topk_case(n_vocab)
    groups = {}
    for r in rows:
        groups.setdefault((r[1], r[3]), []).append(r)
    assert max(len(g) for g in groups.values()) >= 4  # more than one workgroup in a launch
    for (ts, sup), grp in groups.items():
        p, B = P[ts], len(grp)
        params = torch.from_numpy(np.array([p[k] for k in KEYS], np.int32)).cuda()
        bits = torch.from_numpy(suppress_bitmask(n_vocab, sup).view(np.int32)).cuda() if sup else None
        x = torch.from_numpy(np.stack([r[4] for r in grp])).cuda()
        state = torch.from_numpy(_state_rows([r[2] for r in grp], p["timestamp_begin"], sums=[-1.5] * B)).cuda()
        ct = torch.full((B, C1), 7, dtype=torch.int32, device="cuda")
        cl = torch.zeros((B, C1), dtype=torch.float32, device="cuda")
        before = state.clone()
        assert lib.kk_op_whisper_beam_topk(_st(), B, K, _p(x), n_vocab, _p(params), _p(bits), _p(state), _p(ct), _p(cl)) == 0, lib.kk_last_error()
        got_t, got_l = ct.cpu().numpy(), cl.cpu().numpy()
        assert torch.equal(state, before)  # the state is only read
        # the greedy pick on the same rows
        tokens = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
        nxt, left = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((1,), B, dtype=torch.int32, device="cuda")
        assert lib.kk_op_whisper_pick(_st(), B, _p(x), n_vocab, _p(params), _p(bits), _p(state), _p(tokens), 8, _p(nxt), _p(left)) == 0
        greedy_t, greedy_l = nxt.cpu().numpy(), state.cpu().numpy()[:, 6].copy().view(np.float32)
        for b, (name, _, sampled, _, xr) in enumerate(grp):
            f = T.filter_logits(xr, sampled, p, suppress=sup)
            want, _ = BR.top_offers(f, C1, p["eot"])
            n = len(want)
            assert list(got_t[b, :n]) == [t for t, _ in want] and (got_t[b, n:] == -1).all(), (name, got_t[b], want)
            assert np.abs(got_l[b, :n] - np.array([lp for _, lp in want])).max() <= 2e-5, (name, got_l[b], want)
            assert np.isneginf(got_l[b, n:]).all()
            assert all(np.isfinite(f[t]) for t in got_t[b, :n] if np.isfinite(f).any())  # never a masked token
            assert got_t[b, 0] == greedy_t[b] and got_l[b, 0].view(np.uint32) == greedy_l[b].view(np.uint32), (name, got_t[b, 0], greedy_t[b])
            if "planted" in name:
                assert got_t[b, 0] < got_t[b, 1] and got_l[b, 0] == got_l[b, 1] and got_t[b, 2] < got_t[b, 3] and got_l[b, 2] == got_l[b, 3]
            if "three unmasked" in name:
                assert n == 3 and sorted(got_t[b, :3]) == [5, 9, 300]
            if "everything masked" in name:
                assert n == 1 and got_t[b, 0] == p["eot"] and got_l[b, 0] == 0.0
    # a dead row (sum -inf) offers nothing, whatever its logits
    dead = torch.from_numpy(_state_rows([[15]], 50364, sums=[-np.inf])).cuda()
    p = P[False]
    params = torch.from_numpy(np.array([p[k] for k in KEYS], np.int32)).cuda()
    x = torch.from_numpy(rows[1][4][None]).cuda()
    ct = torch.full((1, C1), 7, dtype=torch.int32, device="cuda")
    cl = torch.zeros((1, C1), dtype=torch.float32, device="cuda")
    assert lib.kk_op_whisper_beam_topk(_st(), 1, K, _p(x), n_vocab, _p(params), None, _p(dead), _p(ct), _p(cl)) == 0
    assert (ct.cpu().numpy() == -1).all()


class Beam:
    """the device buffers of kk_whisper_beam_bufs for n_audio windows of K rows, and the pick state, token stores and next[] beside them"""

    def __init__(self, n_audio, K, maxc, n_ctx, cap, eot, tb):
        import torch

        self.lib, self.n_audio, self.K, self.maxc, self.n_ctx, self.cap = _lib.load(), n_audio, K, maxc, n_ctx, cap
        B = self.B = n_audio * K
        i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")  # noqa: E731
        self.cand_token, self.cand_logprob = i32(B, K + 1), torch.zeros((B, K + 1), dtype=torch.float32, device="cuda")
        self.owner = [i32(B, n_ctx), i32(B, n_ctx)]
        self.parent, self.fin_score = i32(B), torch.zeros((n_audio, maxc), dtype=torch.float32, device="cuda")
        self.fin_length, self.fin_tokens, self.fin_count = i32(n_audio, maxc), i32(n_audio, maxc, cap), i32(n_audio)
        self.complete, self.not_complete = i32(n_audio), i32(1)
        self.state, self.tokens, self.next, left = torch.zeros((B, 8), dtype=torch.int32, device="cuda"), i32(B, cap), i32(B), i32(1)
        self.params = torch.from_numpy(np.array([1000, eot, 220, 349, tb, -1, 0, 1], np.int32)).cuda()
        b = self.bufs = _lib.KKWhisperBeamBufs(n_audio=n_audio, beam_size=K, max_candidates=maxc, n_ctx=n_ctx, cap=cap)
        for name in ("cand_token", "cand_logprob", "parent", "fin_score", "fin_length", "fin_tokens", "fin_count", "complete", "not_complete"):
            setattr(b, name, getattr(self, name).data_ptr())
        b.owner[0], b.owner[1] = self.owner[0].data_ptr(), self.owner[1].data_ptr()
        assert self.lib.kk_op_whisper_pick_reset(_st(), B, _p(self.state), _p(left)) == 0
        assert self.lib.kk_op_whisper_beam_reset(_st(), C.byref(b)) == 0, self.lib.kk_last_error()
        self.flip = 0

    def select(self, offers, pos):
        """offers[row] = [(token, logprob)] -> one select at `pos`"""
        import torch

        ct, cl = np.full((self.B, self.K + 1), -1, np.int32), np.full((self.B, self.K + 1), -np.inf, np.float32)
        for r, o in enumerate(offers):
            for i, (t, lp) in enumerate(o):
                ct[r, i], cl[r, i] = t, lp
        self.cand_token.copy_(torch.from_numpy(ct))
        self.cand_logprob.copy_(torch.from_numpy(cl))
        rc = self.lib.kk_op_whisper_beam_select(_st(), C.byref(self.bufs), self.flip, pos, _p(self.params), _p(self.state), _p(self.tokens), _p(self.next))
        assert rc == 0, self.lib.kk_last_error()
        self.flip ^= 1


@pytest.mark.parametrize("K", BR.SELECT_KS)
def test_select_against_the_restatement_and_owner_tables_against_parent_pointers(K):
    """2 windows, 5 chained steps of seeded offers (eot at several ranks; a window that completes and keeps stepping; rows that offer one token or none, so
    slots die and are filled again): after EVERY step the parents, tokens, sums, derived pick states, finished stores, complete flags and the counter equal
    the restatement's, the owner table equals the one built by following the parent pointers on the host, and every live prefix and every finished
    sequence reads back through it."""
    S0, n_ctx, cap, eot, tb = 5, 16, 12, BR.SELECT_EOT, 350
    maxc = BR.SELECT_MAXC[K]
    dev = Beam(2, K, maxc, n_ctx, cap, eot, tb)
    wins = [BR.BeamWindow(K, maxc, eot) for _ in range(2)]
    B = 2 * K
    own = np.repeat(np.arange(B)[:, None], n_ctx, axis=1)
    assert np.array_equal(dev.owner[0].cpu().numpy(), own) and int(dev.not_complete.item()) == 2
    for s, step in enumerate(BR.select_script(K)):
        pos = S0 + s
        dev.select([o for w in range(2) for o in step[w]], pos)  # a dead row's offers are uploaded all the same: select must not read them
        for w in range(2):
            wins[w].update_offers([o if wins[w].live(j) else [] for j, o in enumerate(step[w])])
        parent, nxt, st = dev.parent.cpu().numpy(), dev.next.cpu().numpy(), dev.state.cpu().numpy()
        sums, tokens = st[:, 5].copy().view(np.float32), dev.tokens.cpu().numpy()
        new = np.repeat(np.arange(B)[:, None], n_ctx, axis=1)
        for w in range(2):
            for k in range(K):
                r, pj = w * K + k, wins[w].parents[-1][k]
                assert parent[r] == (w * K + pj if pj >= 0 else -1), (s, r)
                assert nxt[r] == wins[w].prefix[k][-1] and st[r, 4] == s + 1 and st[r, 0] == nxt[r] and st[r, 3] == 0
                if pj < 0:
                    assert np.isneginf(sums[r]) and nxt[r] == eot
                    continue
                assert abs(sums[r] - wins[w].sums[k]) <= 1e-5, (s, r, sums[r], wins[w].sums[k])
                pre = wins[w].prefix[k]
                seen = [t for t in pre if t >= tb]
                assert st[r, 1] == (pre[-2] if len(pre) > 1 else -1) and st[r, 2] == (seen[-1] if seen else -1), (s, r, st[r], pre)  # the PARENT's history
                new[r, :pos] = own[w * K + pj, :pos]
        own = new
        assert np.array_equal(dev.owner[dev.flip].cpu().numpy(), own), f"owner table after step {s}"
        for w in range(2):
            for k in range(K):
                if wins[w].live(k):
                    got = [int(tokens[own[w * K + k, S0 + i], i]) for i in range(s + 1)]
                    assert got == wins[w].prefix[k], (s, w, k, got, wins[w].prefix[k])
        fc, fs, fl, ft = dev.fin_count.cpu().numpy(), dev.fin_score.cpu().numpy(), dev.fin_length.cpu().numpy(), dev.fin_tokens.cpu().numpy()
        for w in range(2):
            assert fc[w] == len(wins[w].finished) and int(dev.complete[w].item()) == int(wins[w].complete), (s, w, fc[w], len(wins[w].finished))
            for f, (toks, score) in enumerate(wins[w].finished):
                assert fl[w, f] == len(toks) and list(ft[w, f, : len(toks)]) == toks and abs(fs[w, f] - score) <= 1e-5, (s, w, f)
        assert int(dev.not_complete.item()) == sum(not w.complete for w in wins)
    assert min(min(w.margins) for w in wins) >= BR.MARGIN
    assert (np.array(own) != np.arange(B)[:, None])[:, : S0 + BR.SELECT_STEPS - 1].any() or K == 1  # the tables did move away from the identity


@pytest.mark.parametrize("heads", [2, 6])
def test_owned_attention_is_bit_equal_to_the_direct_one_on_gathered_keys(heads):
    """T_rows 448, five rows of lengths 1, 127, 128, 129 and 300 (they straddle the 128-key split), the keys of every row scattered over 4 items by a random
    owner table: the output equals, bit for bit, kk_op_whisper_attn_rows on a store that holds each row's keys gathered into one item."""
    import torch

    lib = _lib.load()
    T_rows, items, D = 448, 4, heads * 64
    lens = [1, 127, 128, 129, 300]
    R, ld = len(lens), 2 * D
    g = torch.Generator().manual_seed(heads)
    kv = torch.randn((items, T_rows, ld), generator=g).to(torch.bfloat16).cuda()
    q = torch.randn((R, D), generator=g).cuda()
    owner = torch.randint(0, items, (R, T_rows), generator=g, dtype=torch.int32).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    gathered = kv[owner.long(), torch.arange(T_rows, device="cuda")[None, :].expand(R, T_rows)].contiguous()  # [R][T_rows][ld]: row r's keys in item r
    item = torch.arange(R, dtype=torch.int32).cuda()
    nb = lib.kk_op_whisper_attn_rows_scratch_bytes(R, heads, T_rows)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    a = torch.full((R, D), float("nan"), dtype=torch.float32, device="cuda")
    b = torch.full((R, D), float("nan"), dtype=torch.float32, device="cuda")
    assert lib.kk_op_whisper_attn_rows_owned(_st(), R, heads, _p(q), _p(kv), 0, D, items, T_rows, ld, _p(owner), _p(ln), _p(a), _p(scratch), nb) == 0, lib.kk_last_error()
    assert lib.kk_op_whisper_attn_rows(_st(), R, heads, _p(q), _p(gathered), 0, D, R, T_rows, ld, _p(item), _p(ln), _p(b), _p(scratch), nb) == 0, lib.kk_last_error()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(b).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    k64, v64 = gathered[2, :128, :64].float().cpu().numpy(), gathered[2, :128, D:D + 64].float().cpu().numpy()  # and both are the attention: row 2, head 0
    assert np.abs(a[2, :64] - T.attn_row(q[2, :64].cpu().numpy(), k64, v64)).max() < 1e-4


def test_the_beam_entries_refuse_bad_arguments_before_anything_is_launched():
    import torch

    lib = _lib.load()
    dev = Beam(1, 2, 2, 8, 8, 500, 350)
    before = [t.clone() for t in (dev.state, dev.tokens, dev.next, dev.owner[0], dev.owner[1], dev.fin_count, dev.not_complete)]

    def bufs(**kw):
        b = _lib.KKWhisperBeamBufs.from_buffer_copy(dev.bufs)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    for kw, flip, pos, word in ((dict(beam_size=0), 0, 4, b"beam_size"), (dict(beam_size=9), 0, 4, b"beam_size"), (dict(max_candidates=17), 0, 4, b"max_candidates"),
                                (dict(n_ctx=0), 0, 4, b"n_ctx"), (dict(fin_tokens=None), 0, 4, b"null buffer"), ({}, 2, 4, b"flip"), ({}, 0, 9, b"pos = 9"), ({}, 0, -1, b"pos = -1")):
        rc = lib.kk_op_whisper_beam_select(_st(), C.byref(bufs(**kw)), flip, pos, _p(dev.params), _p(dev.state), _p(dev.tokens), _p(dev.next))
        assert rc != 0 and word in lib.kk_last_error(), (kw, lib.kk_last_error())
    assert lib.kk_op_whisper_beam_select(_st(), C.byref(dev.bufs), 0, 4, _p(dev.params), None, _p(dev.tokens), _p(dev.next)) != 0
    x = torch.zeros((2, 1000), dtype=torch.float32, device="cuda")
    for k in (0, 9):
        assert lib.kk_op_whisper_beam_topk(_st(), 2, k, _p(x), 1000, _p(dev.params), None, _p(dev.state), _p(dev.cand_token), _p(dev.cand_logprob)) != 0
    assert lib.kk_op_whisper_beam_topk(_st(), 0, 2, _p(x), 1000, _p(dev.params), None, _p(dev.state), _p(dev.cand_token), _p(dev.cand_logprob)) != 0
    torch.cuda.synchronize()
    after = (dev.state, dev.tokens, dev.next, dev.owner[0], dev.owner[1], dev.fin_count, dev.not_complete)
    assert all(torch.equal(a, b) for a, b in zip(before, after))  # nothing was launched
    # the owned attention reads its table back: an owner outside the items is refused, one beyond the row's length is never read
    heads, T_rows, D = 2, 64, 128
    kv = torch.zeros((2, T_rows, 2 * D), dtype=torch.bfloat16, device="cuda")
    q, out = torch.zeros((1, D), device="cuda"), torch.zeros((1, D), device="cuda")
    nb = lib.kk_op_whisper_attn_rows_scratch_bytes(1, heads, T_rows)
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ln = torch.tensor([10], dtype=torch.int32).cuda()
    own = torch.zeros((1, T_rows), dtype=torch.int32, device="cuda")
    own[0, 10] = 99
    assert lib.kk_op_whisper_attn_rows_owned(_st(), 1, heads, _p(q), _p(kv), 0, D, 2, T_rows, 2 * D, _p(own), _p(ln), _p(out), _p(scratch), nb) == 0
    own[0, 9] = 2
    assert lib.kk_op_whisper_attn_rows_owned(_st(), 1, heads, _p(q), _p(kv), 0, D, 2, T_rows, 2 * D, _p(own), _p(ln), _p(out), _p(scratch), nb) != 0
    assert b"owner[0][9] = 2 is outside [0, 2)" in lib.kk_last_error()
    assert lib.kk_op_whisper_attn_rows_owned(_st(), 1, heads, _p(q), _p(kv), 0, D, 2, T_rows, 2 * D, _p(own), _p(ln), _p(out), _p(scratch), nb - 1) != 0
    assert b"scratch too small" in lib.kk_last_error()
