"""Row mode of the Whisper text side at the level of the C ABI (kk_whisper_text_rows_*, csrc/kk_whisper_text.hip): rounds that mix prefill and
step rows of different requests at different positions against the window-mode forward of each request alone, bit for bit; the refusals, which are host
checks in front of every launch; and the per-row pick against the launch-wide pick and the numpy restatement of the filters."""
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

from mlx_audio_amd import _lib, whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402

_cache = {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _runtime(name="a"):
    """(dims, TextRuntime on synthetic weights), once per shape"""
    import torch

    if name not in _cache:
        d = T.dims(**(T.SHAPE_A if name == "a" else T.SHAPE_B))
        lib = _lib.load()
        _cache[name] = (d, WD.TextRuntime(lib, d, WD.check_decoder_tensors(d, T.decoder_weights(d, 21)), torch.device("cuda:0"), _st()))
    return _cache[name]


def _params(d, **kw):
    tok = whisper.special_tokens(d)
    P = T.pick_params(tok, d.n_vocab, **kw)
    return P, _lib.KKWhisperPickParams(**P)


class Rows:
    """row mode on a state buffer the test owns: every byte 0xFF before `open` (NaN as bf16 and as fp32, -1 as int32)"""

    def __init__(self, rt, max_rows, ws_rows=512):
        import torch

        self.lib, self.h, self.d, self.N = rt._lib, rt._h, rt.dims, max_rows
        n = self.lib.kk_whisper_text_rows_state_bytes(self.h, max_rows)
        assert n > 0
        self.state = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
        wn = self.lib.kk_whisper_text_rows_workspace_bytes(self.h, ws_rows, max_rows)
        self.ws = torch.empty(wn, dtype=torch.uint8, device="cuda")
        assert self.lib.kk_whisper_text_rows_open(self.h, _st(), max_rows, _p(self.state), n) == 0, self.lib.kk_last_error()
        self.logits = None

    def admit(self, row, feats, tokens, params, bits=None):
        import torch

        f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
        t = np.ascontiguousarray(np.asarray(tokens, np.int32))
        rc = self.lib.kk_whisper_text_rows_admit(self.h, _st(), row, _p(f), t.ctypes.data_as(C.c_void_p), len(t), C.byref(params),
                                                 None if bits is None else bits.ctypes.data_as(C.c_void_p), _p(self.ws), self.ws.numel())
        assert rc == 0, self.lib.kk_last_error()

    def forward_rc(self, items, out_rows, n_items=None, ws_bytes=None):
        import torch

        arr = (_lib.KKWhisperRowsItem * max(len(items), 1))(*[_lib.KKWhisperRowsItem(*(tuple(it) + (-1, 0))[:6]) for it in items])
        out = np.ascontiguousarray(np.asarray(out_rows, np.int32))
        self.logits = torch.full((max(len(out), 1), self.d.n_vocab), float("nan"), dtype=torch.float32, device="cuda")
        return self.lib.kk_whisper_text_rows_forward(self.h, _st(), C.cast(arr, C.c_void_p), len(items) if n_items is None else n_items,
                                                     out.ctypes.data_as(C.c_void_p), len(out), _p(self.logits), _p(self.ws),
                                                     self.ws.numel() if ws_bytes is None else ws_bytes)

    def forward(self, items, out_rows):
        assert self.forward_rc(items, out_rows) == 0, self.lib.kk_last_error()
        return self.logits.cpu().numpy()

    def pick_rc(self, rows):
        r = np.ascontiguousarray(np.asarray(rows, np.int32))
        return self.lib.kk_whisper_text_rows_pick(self.h, _st(), r.ctypes.data_as(C.c_void_p), len(r))

    def flags(self):
        out = np.full(self.N, 7, np.int32)
        assert self.lib.kk_whisper_text_rows_flags(self.h, _st(), out.ctypes.data_as(C.c_void_p)) == 0
        return [int(v) for v in out]

    def read(self, row):
        import torch

        toks = np.zeros(self.d.n_text_ctx, np.int32)
        st = _lib.KKWhisperPickState()
        kept = torch.empty((2, self.d.n_vocab), dtype=torch.float32, device="cuda")
        assert self.lib.kk_whisper_text_rows_read(self.h, _st(), row, toks.ctypes.data_as(C.c_void_p), len(toks), C.byref(st), _p(kept)) == 0
        return toks, st, kept.cpu().numpy()


def _solo(rt, feats, tokens, all_positions=True):
    """window mode, this request alone: set_audio with B = 1 and one forward -> (S, V), or (V,) of the last position"""
    import torch

    rt.set_audio(torch.from_numpy(np.ascontiguousarray(feats[None])).cuda())
    return rt.forward(torch.from_numpy(np.asarray(tokens, np.int32)[None]).cuda(), all_positions).cpu().numpy()[0]


def _lasts(items):
    """the flat row of every item's last position"""
    out, at = [], 0
    for it in items:
        at += it[2]
        out.append(at - 1)
    return out


def _flat(items):
    """(row, position) of every flat row of a round"""
    return [(it[0], it[1] + k) for it in items for k in range(it[2])]


def _setup(name):
    """rows 2, 0 and 3 of 4 admitted with three windows and 40 random initial tokens each; row 1 never.  -> (rows, {row: solo logits (40, V)})"""
    d, rt = _runtime(name)
    g = np.random.default_rng(3)
    feats = T.features(d, 3, 8)
    toks = {r: g.integers(0, d.n_vocab, 40) for r in (2, 0, 3)}
    _, params = _params(d)
    rows = Rows(rt, 4)
    for i, r in enumerate((2, 0, 3)):
        rows.admit(r, feats[i], toks[r], params)
    ref = {r: _solo(rt, feats[i], toks[r]) for i, r in enumerate((2, 0, 3))}
    return d, rt, rows, feats, toks, ref


@pytest.mark.parametrize("name", ["a", "b"])
def test_mixed_rounds_carry_the_bits_of_each_request_alone(name):
    """Round 1: (row 2, 5 tokens), (row 0, 17 tokens: across the 16-row Linear tile), (row 3, 1 token), R = 23, with an inner position of row 0 listed
    and kept; then single steps with the three rows at positions 5, 17 and 1; a round of R = 16 and one of R = 33.  Every listed logits row is the bits of
    the window-mode forward of that request alone, in any order of the items, and nothing of the 0xFF state is ever read."""
    d, rt, rows, feats, toks, ref = _setup(name)
    rounds = [([(2, 0, 5, 0), (0, 0, 17, 0, 3, 1), (3, 0, 1, 0)], [4, 5 + 3, 21, 22]),
              ([(2, 5, 1, 5), (0, 17, 1, 17), (3, 1, 1, 1)], [0, 1, 2]),
              ([(2, 6, 10, 6), (0, 18, 5, 18), (3, 2, 1, 2)], None),        # R = 16
              ([(2, 16, 14, 16), (0, 23, 17, 23), (3, 3, 2, 3)], None)]     # R = 33
    for items, out in rounds:
        out = _lasts(items) if out is None else out
        got = rows.forward(items, out)
        assert np.isfinite(got).all()
        where = [_flat(items)[f] for f in out]
        for k, (row, pos) in enumerate(where):
            assert np.array_equal(got[k], ref[row][pos]), (name, items, row, pos)
        # the same round with its items in another order: the same positions are rewritten with the same values, every item's bits stay
        perm = [items[2], items[0], items[1]]
        got2 = rows.forward(perm, [_flat(perm).index(w) for w in where])
        assert np.array_equal(got2, got), (name, items)
    assert sum(it[2] for it in rounds[0][0]) == 23 and sum(it[2] for it in rounds[2][0]) == 16 and sum(it[2] for it in rounds[3][0]) == 33
    _, _, kept = rows.read(0)
    assert np.array_equal(kept[1], ref[0][3])  # the kept copy of round 1
    assert rows.flags() == [0, 0, 0, 0]


def test_a_row_steps_to_the_last_position_and_on_its_picked_token():
    """row 3 prefilled to n_text_ctx - 2 in one item beside a step row, then stepped at n_text_ctx - 1: the bits of the 448-token window forward; and a
    step that feeds the token the row's pick chose equals the window forward fed that token"""
    d, rt = _runtime("a")
    g = np.random.default_rng(5)
    feats = T.features(d, 2, 9)
    n = d.n_text_ctx
    long, short = g.integers(0, d.n_vocab, n), g.integers(0, d.n_vocab, 6)
    _, params = _params(d, without_timestamps=True)
    rows = Rows(rt, 4, ws_rows=n + 8)
    rows.admit(3, feats[0], long, params)
    rows.admit(1, feats[1], short, params)
    rows.forward([(3, 0, n - 1, 0), (1, 0, 6, 0)], [n - 2, n + 4])
    assert rows.pick_rc([1]) == 0
    got = rows.forward([(1, 6, 1, -1), (3, n - 1, 1, n - 1)], [0, 1])
    assert np.array_equal(got[1], _solo(rt, feats[0], long, all_positions=False))
    toks, st, _ = rows.read(1)
    assert st.count == 1 and 0 <= toks[0] < d.n_vocab
    assert np.array_equal(got[0], _solo(rt, feats[1], list(short) + [int(toks[0])], all_positions=False))
    assert rows.forward_rc([(3, n - 1, 2, n - 2)], [1]) != 0 and b"exceeds n_text_ctx" in rt._lib.kk_last_error()


def test_refusals_are_error_returns_and_a_valid_round_follows():
    d, rt, rows, feats, toks, ref = _setup("a")
    lib = rt._lib
    small = lib.kk_whisper_text_rows_workspace_bytes(rt._h, 4, 4)
    cases = [(dict(items=[(4, 0, 1, 0)], out_rows=[0]), b"outside [0, max_rows"),
             (dict(items=[(-1, 0, 1, 0)], out_rows=[0]), b"outside [0, max_rows"),
             (dict(items=[(1, 0, 1, 0)], out_rows=[0]), b"never admitted"),
             (dict(items=[(2, 0, 1, 0), (2, 1, 1, 1)], out_rows=[0, 1]), b"twice"),
             (dict(items=[(2, d.n_text_ctx - 1, 2, 0)], out_rows=[1]), b"exceeds n_text_ctx"),
             (dict(items=[(2, 0, 41, 0)], out_rows=[40]), b"beyond row 2's 40 initial tokens"),
             (dict(items=[(2, 0, 3, 38)], out_rows=[2]), b"beyond row 2's 40 initial tokens"),
             (dict(items=[(2, 0, 1, -1)], out_rows=[0]), b"no picked token"),
             (dict(items=[(2, 0, 2, -1)], out_rows=[1]), b"needs count 1"),
             (dict(items=[(2, 0, 17, 0)], out_rows=[16], ws_bytes=small), b"workspace too small for R = 17"),
             (dict(items=[(2, 0, 1, 0)] * 33, out_rows=[0], n_items=33), b"33 items are outside"),
             (dict(items=[(2, 0, 2, 0)], out_rows=[2]), b"out_rows[0] = 2 is outside"),
             (dict(items=[(2, 0, 2, 0, 0, 1)], out_rows=[1]), b"kept position is not in out_rows")]
    for kw, word in cases:
        assert rows.forward_rc(**kw) != 0, kw
        assert word in lib.kk_last_error(), (kw, lib.kk_last_error())
    assert rows.pick_rc([2]) != 0 and b"no logits" in lib.kk_last_error()  # nothing was run for row 2 by the refused rounds
    assert rows.pick_rc([1]) != 0 and b"never admitted" in lib.kk_last_error()
    assert rows.pick_rc([5]) != 0 and b"outside [0, max_rows" in lib.kk_last_error()
    # a handle without row mode
    h = C.c_void_p()
    kc = _lib.KKWhisperTextConfig(**{k: int(getattr(d, k)) for k in ("n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer", "n_audio_ctx",
                                                                      "n_audio_state")})
    assert lib.kk_whisper_text_create(C.byref(kc), C.byref(h)) == 0
    one = (_lib.KKWhisperRowsItem * 1)(_lib.KKWhisperRowsItem(0, 0, 1, 0, -1, 0))
    z = np.zeros(1, np.int32)
    assert lib.kk_whisper_text_rows_forward(h, _st(), C.cast(one, C.c_void_p), 1, z.ctypes.data_as(C.c_void_p), 1, _p(rows.ws), _p(rows.ws), 64) != 0
    assert b"row mode not opened" in lib.kk_last_error()
    assert lib.kk_whisper_text_rows_pick(h, _st(), z.ctypes.data_as(C.c_void_p), 1) != 0 and b"row mode not opened" in lib.kk_last_error()
    lib.kk_whisper_text_destroy(h)
    got = rows.forward([(0, 0, 4, 0), (2, 0, 2, 0)], [3, 5])
    assert np.array_equal(got[0], ref[0][3]) and np.array_equal(got[1], ref[2][1])


def _script(tok, V, g):
    """per step the three rows' logits: N(0, 2) with the winner the script wants 40 above the rest.  Row 0 (no timestamps): the blank at the first
    position is masked.  Row 1 (first timestamp at most 25, 7 and 8 suppressed): a first timestamp beyond the limit, then suppressed ids, a closing
    pair, eot.  Row 2 (limit 50, no mask, blanks allowed): a pair, the blank, then 7 and 8, which ITS mask does not hold, and eot."""
    tb, eot = tok.timestamp_begin, tok.eot
    plans = [[220, 1000, 2000, 7, eot, 3000, 4000, 5000],
             [tb + 40, 7, 8, tb + 9, tb + 9, 2000, eot, 9],
             [tb + 40, 220, tb + 45, tb + 45, 7, 8, eot, 9]]
    steps = []
    for s in range(8):
        x = (2.0 * g.standard_normal((3, V))).astype(np.float32)
        for b in range(3):
            x[b, plans[b][s]] += 40.0
        steps.append(x)
    return steps


def test_per_row_pick_equals_the_launch_wide_pick_row_by_row():
    """three rows with three different parameter sets and masks in ONE launch, 8 scripted steps: tokens and every state field are the bits of
    kk_op_whisper_pick run per row with that row's params on the same logits; tokens equal filter_logits + GreedyRow with sum_logprob within 1e-5 per
    step (the bar of test_gpu_whisper_text_kernels for this kernel); the rows' ended flags are exact after every step"""
    import torch

    d, rt = _runtime("a")
    lib, V = rt._lib, d.n_vocab
    tok = whisper.special_tokens(d)
    g = np.random.default_rng(17)
    sets = [(dict(without_timestamps=True), (), None), (dict(max_initial_timestamp_index=25), (7, 8), WD.suppress_bitmask(V, (7, 8))),
            (dict(max_initial_timestamp_index=50, suppress_blank=False), (), None)]
    use = [3, 0, 2]  # set j runs in decoder row use[j]
    rows = Rows(rt, 4)
    feats = T.features(d, 1, 2)[0]
    ref = []
    for (kw, _, bits), r in zip(sets, use):
        P, params = _params(d, **kw)
        rows.admit(r, feats, [tok.sot], params, bits)
        pd = torch.from_numpy(np.array([P[k] for k in ("n_vocab", "eot", "blank", "no_timestamps", "timestamp_begin", "max_initial_timestamp_index",
                                                        "without_timestamps", "suppress_blank")], np.int32)).cuda()
        state = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
        left = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.kk_op_whisper_pick_reset(_st(), 1, _p(state), _p(left)) == 0
        ref.append(dict(P=P, params=pd, bits=None if bits is None else torch.from_numpy(bits.view(np.int32)).cuda(), state=state, left=left,
                        tokens=torch.full((1, d.n_text_ctx), -1, dtype=torch.int32, device="cuda"), nxt=torch.zeros(1, dtype=torch.int32, device="cuda"),
                        row=T.GreedyRow(tok.eot)))
    for s, x in enumerate(_script(tok, V, g)):
        items = [(r, s, 1, 0 if s == 0 else -1) for r in use]
        assert rows.forward_rc(items, [0, 1, 2]) == 0, lib.kk_last_error()
        rows.logits.copy_(torch.from_numpy(x).cuda())  # the round's logits are the caller's memory: the script goes in before the pick
        assert rows.pick_rc(use) == 0, lib.kk_last_error()
        for j, (kw, sup, _) in enumerate(sets):
            e = ref[j]
            xd = torch.from_numpy(np.ascontiguousarray(x[j:j + 1])).cuda()
            assert lib.kk_op_whisper_pick(_st(), 1, _p(xd), V, _p(e["params"]), _p(e["bits"]), _p(e["state"]), _p(e["tokens"]), d.n_text_ctx, _p(e["nxt"]),
                                          _p(e["left"])) == 0
            f = T.filter_logits(x[j], e["row"].sampled, e["P"], suppress=sup)
            top = np.sort(f[np.isfinite(f)])[-2:]
            assert top[1] - top[0] > 1e-3, "the script's logits must not tie"
            e["row"].update(f)
        fl = rows.flags()
        assert [fl[r] for r in use] == [int(e["row"].ended) for e in ref] and fl[1] == 0, (s, fl)
    for j, r in enumerate(use):
        e = ref[j]
        toks, st, _ = rows.read(r)
        want = e["state"].cpu().numpy()[0]
        got = np.frombuffer(bytes(st), np.int32)
        assert np.array_equal(got, want), (j, got, want)  # every field, sum_logprob and last_logprob as bits
        assert list(toks[:8]) == list(e["tokens"].cpu().numpy()[0, :8])
        assert list(toks[:8]) == e["row"].sampled
        assert abs(st.sum_logprob - e["row"].sum_logprob) <= 1e-5 * 8 and st.count == 8 and st.ended == int(e["row"].ended)
    assert ref[0]["row"].sampled[0] != 220 and ref[0]["row"].sampled[3] == 7  # row 0: blank masked at first, 7 allowed
    assert 7 not in ref[1]["row"].sampled and 8 not in ref[1]["row"].sampled and ref[1]["row"].sampled[0] <= tok.timestamp_begin + 25
    assert ref[2]["row"].sampled[0] == tok.timestamp_begin + 40 and all(e["row"].ended for e in ref)
