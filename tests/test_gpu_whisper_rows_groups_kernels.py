"""Groups of row mode at the level of the C ABI (kk_whisper_text_rows_groups_bind, _admit_group, _group_read, _group_release, _group_offers;
csrc/kk_whisper_text.hip): G rows on the leader's cross K/V against window mode's grouped state, the per-row top-k of the round's one pick
launch against kk_op_whisper_beam_topk, the per-group select against the restatement of tests/_whisper_beam_ref.py for two groups at different
positions, a beam row's step through its owner row against a plain row that holds the same prefix, and the refusals.  Both state buffers are 0xFF
in every byte before they are opened (NaN as bf16 and fp32, -1 as int32): whatever a round reads, an admission has written."""
import ctypes as C
import math
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
from test_gpu_whisper_rows_kernels import Rows, _p, _params, _runtime, _solo, _st  # noqa: E402

from mlx_audio_amd import _lib, whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

PLAIN, BEAM = _lib.WHISPER_GROUP_PLAIN, _lib.WHISPER_GROUP_BEAM
FIN = 2 * _lib.WHISPER_MAX_GROUP


class Groups(Rows):
    """Rows with the groups buffer bound behind rows_open; the workspace is sized after the bind (it then holds the round's owner table)"""

    def __init__(self, rt, max_rows, ws_rows=512, bind=True):
        import torch

        super().__init__(rt, max_rows, ws_rows)
        n = self.lib.kk_whisper_text_rows_groups_state_bytes(self.h, max_rows)
        assert n > 0
        self.gstate = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
        if bind:
            assert self.lib.kk_whisper_text_rows_groups_bind(self.h, _st(), _p(self.gstate), n) == 0, self.lib.kk_last_error()
            self.ws = torch.empty(self.lib.kk_whisper_text_rows_workspace_bytes(self.h, ws_rows, max_rows), dtype=torch.uint8, device="cuda")

    def admit_group_rc(self, rows, kind, feats, tokens, params, bits=None, maxc=1):
        import torch

        f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
        t = np.ascontiguousarray(np.asarray(tokens, np.int32))
        r = np.ascontiguousarray(np.asarray(rows, np.int32))
        return self.lib.kk_whisper_text_rows_admit_group(self.h, _st(), r.ctypes.data_as(C.c_void_p), len(r), kind, _p(f), t.ctypes.data_as(C.c_void_p), len(t),
                                                         C.byref(params), None if bits is None else bits.ctypes.data_as(C.c_void_p), maxc, _p(self.ws), self.ws.numel())

    def admit_group(self, *a, **kw):
        assert self.admit_group_rc(*a, **kw) == 0, self.lib.kk_last_error()

    def set_token(self, row, index, token):
        import torch

        t = torch.tensor([token], dtype=torch.int32, device="cuda")
        assert self.lib.kk_whisper_text_rows_set_token(self.h, _st(), row, index, _p(t)) == 0, self.lib.kk_last_error()
        torch.cuda.synchronize()

    def group_read(self, leader, G):
        """-> (finished [(tokens, score)], live [(tokens, sum)] by slot, kept (2, V))"""
        import torch

        cap = self.d.n_text_ctx
        fc, fs, fl = np.zeros(1, np.int32), np.zeros(FIN, np.float32), np.zeros(FIN, np.int32)
        ft, lt = np.zeros((FIN, cap), np.int32), np.zeros((G, cap), np.int32)
        ls, ll = np.zeros(G, np.float32), np.zeros(G, np.int32)
        kept = torch.empty((2, self.d.n_vocab), dtype=torch.float32, device="cuda")
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = self.lib.kk_whisper_text_rows_group_read(self.h, _st(), leader, cap, p(fc), p(fs), p(fl), p(ft), p(lt), p(ls), p(ll), _p(kept))
        assert rc == 0, self.lib.kk_last_error()
        fin = [([int(t) for t in ft[f, : fl[f]]], float(fs[f])) for f in range(fc[0])]
        live = [([int(t) for t in lt[k, : ll[k]]], float(ls[k])) for k in range(G)]
        return fin, live, kept.cpu().numpy()

    def offers(self, row, n):
        t, lp = np.zeros(n, np.int32), np.zeros(n, np.float32)
        assert self.lib.kk_whisper_text_rows_group_offers(self.h, _st(), row, t.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p)) == 0, self.lib.kk_last_error()
        return t, lp

    def release(self, leader):
        return self.lib.kk_whisper_text_rows_group_release(self.h, leader)


@pytest.mark.parametrize("name", ["a", "b"])
def test_a_group_reads_its_leaders_cross_slice_with_the_bits_of_window_modes_groups(name):
    """A plain group on rows 5, 0, 3 (leader 5: the only row whose cross slices are written) next to the single row 2 on another window: a 4-token
    prefill and 3 steps with different tokens per row.  Every row's logits are the bits of window mode's set_audio_groups(1 window, 3 rows) forward of the
    same tokens; shape b's 1500 audio positions take the multi-split cross-attention."""
    import torch

    d, rt = _runtime(name)
    g = np.random.default_rng(31)
    feats = T.features(d, 2, 12)
    grp, n = (5, 0, 3), 7
    toks = {r: g.integers(0, d.n_vocab, n) for r in grp + (2,)}
    _, params = _params(d)
    rows = Groups(rt, 6)
    rows.admit_group(grp, PLAIN, feats[0], toks[5], params)
    for r in (0, 3):  # the admission gives every row the leader's tokens: the others get their own on the device
        for i in range(n):
            rows.set_token(r, i, int(toks[r][i]))
    rows.admit(2, feats[1], toks[2], params)
    order = (0, 2, 5, 3)
    got = [rows.forward([(r, 0, 4, 0) for r in order], [4 * i + 3 for i in range(4)])]
    for s in range(4, n):
        got.append(rows.forward([(r, s, 1, s) for r in order], [0, 1, 2, 3]))
    rt.set_audio_groups(torch.from_numpy(np.ascontiguousarray(feats[:1])).cuda(), 3)
    tt = torch.from_numpy(np.stack([toks[r] for r in grp]).astype(np.int32)).cuda()
    ref = [rt.forward(tt[:, :4].contiguous(), False).cpu().numpy()]
    for s in range(4, n):
        ref.append(rt.forward(tt[:, s:s + 1].contiguous(), False).cpu().numpy())
    solo = _solo(rt, feats[1], toks[2])
    for k in range(len(got)):
        assert np.isfinite(got[k]).all()
        for j, r in enumerate(order):
            want = solo[3 + k] if r == 2 else ref[k][grp.index(r)]
            assert np.array_equal(got[k][j].view(np.uint32), want.view(np.uint32)), (name, k, r)
    assert not np.array_equal(got[0][0], got[0][2])  # the rows of the group did carry different tokens


KEYS = ("n_vocab", "eot", "blank", "no_timestamps", "timestamp_begin", "max_initial_timestamp_index", "without_timestamps", "suppress_blank")


def test_per_row_topk_greedy_and_sampled_rows_in_one_pick_launch():
    """Three beam groups of 5 rows with three parameter sets on the first-position rows of _whisper_beam_ref.topk_case (timestamps with an initial limit,
    no timestamps, a bitmask that leaves eot and the blank, which the first position then masks too), a greedy row and a sampled row, all in ONE
    rows_pick: every beam row's 6 offers are the bits of kk_op_whisper_beam_topk on the same logits, parameters and a fresh state; the greedy row's and
    the sampled row's token and state are the bits of kk_op_whisper_pick / kk_op_whisper_pick_sampled."""
    import torch

    d, rt = _runtime("a")
    lib, V, K = rt._lib, d.n_vocab, BR.TOPK_K
    tok = whisper.special_tokens(d)
    P, cases = BR.topk_case(V)
    pick = [c for c in cases if c[0] in ("first, timestamps", "first, no timestamps", "everything masked at the first position but eot and the blank")]
    assert len(pick) == 3
    rows = Groups(rt, 17)
    feats = T.features(d, 1, 2)[0]
    layout = [(10, 1, 12, 3, 14), (0, 11, 2, 13, 4), (5, 15, 6, 16, 7)]  # interleaved physical rows
    sets = []
    for (name, ts, hist, sup, x), grp in zip(pick, layout):
        assert hist == []
        params = _lib.KKWhisperPickParams(**P[ts])
        bits = WD.suppress_bitmask(V, sup) if sup else None
        rows.admit_group(grp, BEAM, feats, [tok.sot], params, bits, maxc=K)
        sets.append((name, P[ts], bits, x, grp))
    Pg, params_g = _params(d, without_timestamps=True)
    rows.admit(8, feats, [tok.sot], params_g)
    rows.admit(9, feats, [tok.sot], params_g)
    seed, stream, temp = 1234, 77, 0.7
    assert lib.kk_whisper_text_rows_set_draw(rows.h, _st(), 9, C.c_float(temp), seed, stream) == 0, lib.kk_last_error()
    order = [r for *_, grp in sets for r in grp] + [8, 9]
    assert rows.forward_rc([(r, 0, 1, 0) for r in order], list(range(17))) == 0, lib.kk_last_error()
    xg = (2.0 * np.random.default_rng(8).standard_normal((2, V))).astype(np.float32)
    script = np.concatenate([np.repeat(x[None], 5, axis=0) for *_, x, _ in sets] + [xg]).astype(np.float32)
    rows.logits.copy_(torch.from_numpy(script).cuda())
    assert rows.pick_rc(order) == 0, lib.kk_last_error()

    def fresh():
        state, left = torch.zeros((1, 8), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.kk_op_whisper_pick_reset(_st(), 1, _p(state), _p(left)) == 0
        return state, left

    for name, p, bits, x, grp in sets:
        pd = torch.from_numpy(np.array([p[k] for k in KEYS], np.int32)).cuda()
        bd = None if bits is None else torch.from_numpy(bits.view(np.int32)).cuda()
        state, _ = fresh()
        ct, cl = torch.full((1, K + 1), 7, dtype=torch.int32, device="cuda"), torch.zeros((1, K + 1), dtype=torch.float32, device="cuda")
        xd = torch.from_numpy(np.ascontiguousarray(x[None])).cuda()
        assert lib.kk_op_whisper_beam_topk(_st(), 1, K, _p(xd), V, _p(pd), _p(bd), _p(state), _p(ct), _p(cl)) == 0, lib.kk_last_error()
        want_t, want_l = ct.cpu().numpy()[0], cl.cpu().numpy()[0]
        assert want_t[0] >= 0
        for r in grp:
            t, lp = rows.offers(r, K + 1)
            assert np.array_equal(t, want_t) and np.array_equal(lp.view(np.uint32), want_l.view(np.uint32)), (name, r, t, want_t)
    pd = torch.from_numpy(np.array([Pg[k] for k in KEYS], np.int32)).cuda()
    for j, r in enumerate((8, 9)):
        state, left = fresh()
        tokens, nxt = torch.full((1, d.n_text_ctx), -1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        xd = torch.from_numpy(np.ascontiguousarray(xg[j:j + 1])).cuda()
        if r == 8:
            assert lib.kk_op_whisper_pick(_st(), 1, _p(xd), V, _p(pd), None, _p(state), _p(tokens), d.n_text_ctx, _p(nxt), _p(left)) == 0
        else:
            sid = torch.tensor([stream], dtype=torch.int32, device="cuda")
            assert lib.kk_op_whisper_pick_sampled(_st(), 1, _p(xd), V, _p(pd), None, C.c_float(temp), seed, _p(sid), _p(state), _p(tokens), d.n_text_ctx, _p(nxt),
                                                  _p(left)) == 0, lib.kk_last_error()
        toks, st, _ = rows.read(r)
        assert np.array_equal(np.frombuffer(bytes(st), np.int32), state.cpu().numpy()[0]), r
        assert toks[0] == int(tokens[0, 0].item())
    assert rows.read(8)[0][0] == int(np.argmax(xg[0]))


def _norm(offers, eot, real_eot):
    """what a row offers when its logits are the script's log-probabilities at the script's tokens and -inf elsewhere: the same tokens on the row's own
    log-sum-exp; a row without a token has everything masked and offers (eot, 0) alone (kk_op_whisper_beam_topk)"""
    if not offers:
        return [(real_eot, 0.0)]
    x = np.array([lp for _, lp in offers], np.float64)
    lse = x.max() + math.log(np.exp(x - x.max()).sum())
    return [(real_eot if t == eot else t, float(lp - lse)) for (t, _), lp in zip(offers, x)]


def test_two_beam_groups_at_different_positions_against_the_restatement_after_every_step():
    """Group A (K = 3, rows 7, 2, 9, 4 initial tokens, window 1 of select_script(3): it completes and keeps stepping, slots die and are filled again) and
    group B (K = 8, rows 0, 8, 1, 10, 3, 11, 5, 4, 6 initial tokens, patience 1.5, window 0 of select_script(8)), B admitted two rounds after A: five chained
    steps each, the scripted offers entering as logits (the script's log-probability at the script's tokens, -inf elsewhere) so that the round's own pick
    launch makes them.  After EVERY step, per group: the live prefixes by SLOT read through the owner table equal the restatement's prefixes -- which
    follow the parent pointers on the host --, the sums, the finished stores and the complete flag, which the poll reads from the rows' ended flags.
    Sums: 1e-5, the window-mode test's bound; the script's decision margin must then be ten times that."""
    import torch

    d, rt = _runtime("a")
    lib, V = rt._lib, d.n_vocab
    tok = whisper.special_tokens(d)
    _, params = _params(d, without_timestamps=True, suppress_blank=False)
    rows = Groups(rt, 12)
    feats = T.features(d, 2, 4)
    g = np.random.default_rng(2)
    groups = {"A": dict(K=3, rows=(7, 2, 9), n=4, w=1, start=0, feats=feats[0]), "B": dict(K=8, rows=(0, 8, 1, 10, 3, 11, 5, 4), n=6, w=0, start=2, feats=feats[1])}
    for e in groups.values():
        e["script"] = [step[e["w"]] for step in BR.select_script(e["K"])]
        e["win"] = BR.BeamWindow(e["K"], BR.SELECT_MAXC[e["K"]], tok.eot)
        e["init"] = g.integers(0, 400, e["n"])
    for rnd in range(2 + BR.SELECT_STEPS):
        active = [(k, e, rnd - e["start"]) for k, e in groups.items() if 0 <= rnd - e["start"] < BR.SELECT_STEPS]
        items, out, at = [], [], 0
        for k, e, s in active:
            if s == 0:
                rows.admit_group(e["rows"], BEAM, e["feats"], e["init"], params, maxc=BR.SELECT_MAXC[e["K"]])
            for r in e["rows"]:
                items.append((r, 0, e["n"], 0) if s == 0 else (r, e["n"] + s - 1, 1, -1))
                at += items[-1][2]
                out.append(at - 1)
        assert rows.forward_rc(items, out) == 0, lib.kk_last_error()
        x = np.full((len(out), V), -np.inf, np.float32)
        j = 0
        for k, e, s in active:
            for slot in range(e["K"]):
                for t, lp in e["script"][s][slot]:
                    x[j, tok.eot if t == BR.SELECT_EOT else t] = lp
                j += 1
        rows.logits.copy_(torch.from_numpy(x).cuda())
        assert rows.pick_rc([it[0] for it in items]) == 0, lib.kk_last_error()
        flags = rows.flags()
        for k, e, s in active:
            win, K = e["win"], e["K"]
            win.update_offers([_norm(o, BR.SELECT_EOT, tok.eot) if win.live(j) else [] for j, o in enumerate(e["script"][s])])
            fin, live, _ = rows.group_read(e["rows"][0], K)
            for slot in range(K):
                if not win.live(slot):
                    assert np.isneginf(live[slot][1]), (k, s, slot)
                    continue
                assert live[slot][0] == win.prefix[slot], (k, s, slot, live[slot][0], win.prefix[slot])
                assert abs(live[slot][1] - win.sums[slot]) <= 1e-5, (k, s, slot)
            assert len(fin) == len(win.finished), (k, s, len(fin), len(win.finished))
            for (gt, gs), (wt, ws) in zip(fin, win.finished):
                assert gt == wt and abs(gs - ws) <= 1e-5, (k, s)
            assert [flags[r] for r in e["rows"]] == [int(win.complete)] * K, (k, s, flags)
    A, B = groups["A"]["win"], groups["B"]["win"]
    assert min(A.margins + B.margins) >= 1e-4
    assert A.complete and any(-1 in p for p in A.parents) and not B.complete and len(B.finished) >= 1
    assert any(p != list(range(len(p))) for p in B.parents[1:])  # the prefixes did move between slots


@pytest.mark.parametrize("n", [1, 127, 298])
def test_a_beam_rows_step_reads_its_prefix_through_the_owner_table(n):
    """A beam group of 2 on rows 3 and 1 behind `n` initial tokens.  Pick 1 gives slot 0 the prefix [a] and slot 1 [b] (one parent); pick 2 is scripted so
    that the slots SWAP parents: slot 0 continues [b] -- whose key at position n lies in row 1 -- and slot 1 continues [a].  The step after each pick
    gives every row the logits, bit for bit, of a plain window-mode row fed that slot's whole prefix: n + 1 keys (none foreign yet), then n + 2 keys, the
    one at position n read from the other row -- 3, 129 and 300 keys, across the 128-key split.  (A step follows a prefill, so a step on one key does not
    exist; kk_op_whisper_attn_rows_owned is tested on one key by test_gpu_whisper_beam_kernels.)"""
    import torch

    d, rt = _runtime("a")
    lib, V = rt._lib, d.n_vocab
    tok = whisper.special_tokens(d)
    _, params = _params(d, without_timestamps=True, suppress_blank=False)
    rows = Groups(rt, 4, ws_rows=2 * n + 2)
    feats = T.features(d, 1, 6)[0]
    init = np.random.default_rng(n).integers(0, d.n_vocab, n)
    grp = (3, 1)
    rows.admit_group(grp, BEAM, feats, init, params, maxc=2)
    win = BR.BeamWindow(2, 2, tok.eot)
    a, b, c, dd = 1000, 2000, 3000, 4000
    scripts = [[[(a, 0.0), (b, -0.2), (5, -5.0)], [(6, 0.0)]], [[(dd, 0.0), (7, -1.0), (8, -2.0)], [(c, 10.0), (9, 0.0), (10, -1.0)]]]
    assert rows.forward_rc([(r, 0, n, 0) for r in grp], [n - 1, 2 * n - 1]) == 0, lib.kk_last_error()
    for s, script in enumerate(scripts):
        x = np.full((2, V), -np.inf, np.float32)
        for j in range(2):
            for t, lp in script[j]:
                x[j, t] = lp
        rows.logits.copy_(torch.from_numpy(x).cuda())
        assert rows.pick_rc(grp) == 0, lib.kk_last_error()
        win.update_offers([_norm(o, -1, tok.eot) for o in script])
        got = rows.forward([(r, n + s, 1, -1) for r in grp], [0, 1])
        for slot in range(2):
            want = _solo(rt, feats, list(init) + win.prefix[slot], all_positions=False)
            assert np.array_equal(got[slot].view(np.uint32), want.view(np.uint32)), (n, s, slot)
    assert win.prefix == [[b, c], [a, dd]] and win.parents == [[0, 0], [1, 0]] and min(win.margins) > 1e-3
    _, live, _ = rows.group_read(3, 2)
    assert [t for t, _ in live] == win.prefix


@pytest.mark.parametrize("draw", [None, (0.7, 1234, 77)])
def test_a_plain_group_of_one_is_a_single_row(draw):
    """With the groups buffer bound, row 0 admitted by rows_admit and row 1 as the plain group (1,) carry the same window, initial tokens and pick
    parameters (and, in the second case, the same draw): a prefill that keeps the sot position in slot 1, a pick, two steps with their picks.  The two
    rows' logits are bit-equal in every round and are the request's window-mode bits; rows_read(0) and rows_group_read(1) give the same tokens, count,
    sum and kept rows."""
    d, rt = _runtime("a")
    lib = rt._lib
    tok = whisper.special_tokens(d)
    _, params = _params(d, without_timestamps=True)
    feats = T.features(d, 1, 5)[0]
    init = [tok.sot, 11, 12]
    rows = Groups(rt, 2)
    rows.admit(0, feats, init, params)
    rows.admit_group((1,), PLAIN, feats, init, params)
    if draw is not None:
        for r in (0, 1):
            assert lib.kk_whisper_text_rows_set_draw(rows.h, _st(), r, C.c_float(draw[0]), draw[1], draw[2]) == 0, lib.kk_last_error()
    got = [rows.forward([(0, 0, 3, 0, 0, 1), (1, 0, 3, 0, 0, 1)], [0, 2, 3, 5])]
    assert rows.pick_rc([0, 1]) == 0, lib.kk_last_error()
    for s in range(2):
        got.append(rows.forward([(0, 3 + s, 1, -1), (1, 3 + s, 1, -1)], [0, 1]))
        assert rows.pick_rc([0, 1]) == 0, lib.kk_last_error()
    toks, st, kept = rows.read(0)
    fin, live, gkept = rows.group_read(1, 1)
    assert fin == [] and st.count == 3 and live[0] == ([int(t) for t in toks[:3]], float(st.sum_logprob))
    assert np.array_equal(kept.view(np.uint32), gkept.view(np.uint32))
    solo = _solo(rt, feats, init + [int(t) for t in toks[:2]])
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    assert same(got[0][0], solo[0]) and same(got[0][2], solo[0]) and same(kept[1], solo[0])  # the sot position
    for k, (a, b) in enumerate([(got[0][1], got[0][3]), (got[1][0], got[1][1]), (got[2][0], got[2][1])]):  # the prefill's last position, then the steps
        assert np.isfinite(a).all() and same(a, solo[2 + k]) and same(b, solo[2 + k]), (draw, k)


def test_group_refusals_are_error_returns_and_a_valid_round_follows():
    import torch

    d, rt = _runtime("a")
    lib = rt._lib
    tok = whisper.special_tokens(d)
    _, params = _params(d, without_timestamps=True)
    feats = T.features(d, 1, 3)[0]
    init = [tok.sot, 11, 12]
    unbound = Groups(rt, 6, bind=False)
    assert unbound.admit_group_rc((0, 1), BEAM, feats, init, params, maxc=2) != 0 and b"groups are not bound" in lib.kk_last_error()
    assert unbound.release(0) != 0 and b"groups are not bound" in lib.kk_last_error()
    assert lib.kk_whisper_text_rows_groups_bind(unbound.h, _st(), _p(unbound.gstate), 64) != 0 and b"too small" in lib.kk_last_error()
    rows = Groups(rt, 6)
    guard = [rows.state.clone(), rows.gstate.clone()]
    for args, kw, word in ((((0, 1, 0), BEAM), dict(maxc=3), b"listed twice"), (((0, 6), BEAM), dict(maxc=2), b"outside [0, max_rows"),
                           (((), BEAM), dict(maxc=2), b"a group of 0 rows"), ((tuple(range(6)) + (0, 1, 2), PLAIN), {}, b"a group of 9 rows"),
                           (((0, 1), BEAM), dict(maxc=0), b"max_candidates = 0"), (((0, 1), BEAM), dict(maxc=17), b"max_candidates = 17"),
                           (((0, 1), 2), dict(maxc=2), b"neither plain")):
        assert rows.admit_group_rc(args[0], args[1], feats, init, params, **kw) != 0, args
        assert word in lib.kk_last_error(), (args, lib.kk_last_error())
    torch.cuda.synchronize()
    assert torch.equal(rows.state, guard[0]) and torch.equal(rows.gstate, guard[1])  # nothing was launched, nothing uploaded
    rows.admit_group((4, 1), BEAM, feats, init, params, maxc=2)
    rows.admit_group((2, 5), PLAIN, feats, init, params)
    rows.admit(0, feats, init, params)
    assert rows.admit_group_rc((3, 1), BEAM, feats, init, params, maxc=2) != 0 and b"row 1 is already in the group led by row 4" in lib.kk_last_error()
    f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    t = np.asarray(init, np.int32)
    assert lib.kk_whisper_text_rows_admit(rows.h, _st(), 1, _p(f), t.ctypes.data_as(C.c_void_p), 3, C.byref(params), None, _p(rows.ws), rows.ws.numel()) != 0
    assert b"belongs to the group led by row 4" in lib.kk_last_error()
    guard = [rows.state.clone(), rows.gstate.clone()]
    cases = [([(4, 0, 3, 0), (1, 0, 2, 0), (0, 0, 3, 0)], b"leader 4 at 0 + 3"),       # positions disagree
             ([(1, 0, 3, 0), (0, 0, 3, 0)], b"stepped partially"),                      # a follower alone
             ([(2, 0, 3, 0), (0, 0, 3, 0), (4, 0, 3, 0), (1, 0, 3, 0), (5, 1, 2, 1)], b"leader 2 at 0 + 3")]
    for items, word in cases:
        assert rows.forward_rc(items, [0]) != 0 and word in lib.kk_last_error(), (items, lib.kk_last_error())
    # the leader alone before the group's first pick (its detection round) is a valid round
    assert rows.forward_rc([(4, 0, 1, 0), (2, 0, 1, 0)], [0, 1]) == 0, lib.kk_last_error()
    full = [(4, 0, 3, 0), (1, 0, 3, 0), (2, 0, 3, 0), (5, 0, 3, 0), (0, 0, 3, 0)]
    assert rows.forward_rc(full, [2, 5, 8, 11, 14]) == 0, lib.kk_last_error()
    guard = [rows.state.clone(), rows.gstate.clone()]
    assert rows.pick_rc([4, 0]) != 0 and b"picked partially (1 of its 2 rows" in lib.kk_last_error()
    assert rows.pick_rc([5, 0]) != 0 and b"picked partially" in lib.kk_last_error()
    torch.cuda.synchronize()
    assert torch.equal(rows.state, guard[0]) and torch.equal(rows.gstate, guard[1])
    assert rows.pick_rc([4, 1, 2, 5, 0]) == 0, lib.kk_last_error()
    # after the first select: the leader may no longer run alone, and a beam row takes no initial tokens
    assert rows.forward_rc([(4, 3, 1, -1), (0, 3, 1, -1)], [0, 1]) != 0 and b"stepped partially" in lib.kk_last_error()
    assert rows.forward_rc([(4, 0, 3, 0), (1, 0, 3, 0)], [2, 5]) != 0 and b"prefilled after the group's first select" in lib.kk_last_error()
    assert rows.release(1) != 0 and b"row 1 leads no group" in lib.kk_last_error()
    step = [(4, 3, 1, -1), (1, 3, 1, -1), (2, 3, 1, -1), (5, 3, 1, -1), (0, 3, 1, -1)]
    got = rows.forward(step, [0, 1, 2, 3, 4])
    assert np.isfinite(got).all()
    toks, _, _ = rows.read(0)
    assert np.array_equal(got[4], _solo(rt, feats, init + [int(toks[0])], all_positions=False))  # the single row beside the groups keeps its solo bits
    assert rows.release(4) == 0 and rows.release(4) != 0
    # Rows change kind across a release.  The beam group has selected: its owner rows are rewritten and its flip is 1.  Its former leader comes back as
    # a single row and its former follower as a plain group of one; both prefill and step with the bits of the request alone
    rows.admit(4, feats, init, params)
    rows.admit_group((1,), PLAIN, feats, init, params)
    solo = _solo(rt, feats, init)
    got = rows.forward([(4, 0, 3, 0), (1, 0, 3, 0)], [2, 5])
    assert np.array_equal(got[0].view(np.uint32), solo[2].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), solo[2].view(np.uint32))
    assert rows.pick_rc([4, 1]) == 0, lib.kk_last_error()
    got = rows.forward([(4, 3, 1, -1), (1, 3, 1, -1)], [0, 1])
    toks, _, _ = rows.read(4)
    _, live, _ = rows.group_read(1, 1)
    assert live[0][0] == [int(toks[0])]
    want = _solo(rt, feats, init + [int(toks[0])], all_positions=False)
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want.view(np.uint32))

    # A row that was last a single row goes into a new beam group with no release between: the group's first round -- prefill, offers, select, the step
    # through the owner table -- is that of the same group on a freshly opened state
    def first_round(rows):
        rows.admit_group((4, 3), BEAM, feats, init, params, maxc=2)
        out = [rows.forward([(4, 0, 3, 0), (3, 0, 3, 0)], [2, 5])]
        assert rows.pick_rc([4, 3]) == 0, lib.kk_last_error()
        out += [a for r in (4, 3) for a in rows.offers(r, 3)]
        out.append(rows.forward([(4, 3, 1, -1), (3, 3, 1, -1)], [0, 1]))
        return out, rows.group_read(4, 2)[:2]

    used, used_lists = first_round(rows)
    fresh, fresh_lists = first_round(Groups(rt, 6))
    assert used_lists == fresh_lists and len(used_lists[1][0][0]) == 1
    for a, b in zip(used, fresh):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
