"""The sampled pick of the Whisper text side (csrc/kk_whisper_text_kernels.hip) on its own, through the raw kk_op_whisper_pick_sampled entry: against
the numpy restatement of its random contract (tests/_whisper_sample_ref.py), its determinism, masking, the distribution it draws from and its refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_sample_ref as SR  # noqa: E402
import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import _lib, whisper  # noqa: E402
from mlx_audio_amd.whisper_decoding import suppress_bitmask  # noqa: E402

KEYS = ("n_vocab", "eot", "blank", "no_timestamps", "timestamp_begin", "max_initial_timestamp_index", "without_timestamps", "suppress_blank")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Picker:
    """B rows of pick state on the device and one sampled launch per call"""

    def __init__(self, P, sup, B, cap, temperature, seed, streams):
        import torch

        self.lib, self.B, self.cap, self.V = _lib.load(), B, cap, P["n_vocab"]
        self.temperature, self.seed = temperature, seed
        self.params = torch.from_numpy(np.array([P[k] for k in KEYS], np.int32)).cuda()
        self.bits = None if sup is None else torch.from_numpy(suppress_bitmask(self.V, sup).view(np.int32)).cuda()
        self.streams = torch.from_numpy(np.asarray(streams, np.uint32).view(np.int32)).cuda()
        self.state = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
        self.tokens = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
        self.next = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.left = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert self.lib.kk_op_whisper_pick_reset(_st(), B, _p(self.state), _p(self.left)) == 0

    def pick(self, logits, temperature=None):
        """logits: float32 device (B, V) -> the chosen tokens"""
        rc = self.lib.kk_op_whisper_pick_sampled(_st(), self.B, _p(logits), self.V, _p(self.params), _p(self.bits), self.temperature if temperature is None
                                                 else temperature, self.seed, _p(self.streams), _p(self.state), _p(self.tokens), self.cap, _p(self.next), _p(self.left))
        assert rc == 0, self.lib.kk_last_error()
        return [int(t) for t in self.next.cpu().numpy()]


@pytest.mark.parametrize("temperature", SR.PICK_TEMPERATURES)
@pytest.mark.parametrize("n_vocab,mi", SR.PICK_CASES)
def test_sampled_pick_follows_the_numpy_restatement(n_vocab, mi, temperature):
    """The greedy pick test's scripted 8-step walk, B = 4: every token of a row that has not ended lies in the admissible set of its draw (one admissible
    token: equality; at most 2 % of the draws may have more), sum_logprob within 1e-5 per step of the restatement following the device's tokens, an ended
    row emits eot with its sum frozen, the not-ended counter exact after every step."""
    import torch

    tok = whisper.special_tokens(T.dims(128, 2, 1, n_vocab, 100))
    P = T.pick_params(tok, n_vocab, max_initial_timestamp_index=mi)
    steps, sup = SR.pick_script(tok, n_vocab, mi)
    B, cap = 4, 16
    pk = Picker(P, sup, B, cap, temperature, SR.PICK_SEED, SR.PICK_STREAMS)
    rows = [SR.SampledRow(tok.eot, temperature, SR.PICK_SEED, s) for s in SR.PICK_STREAMS]
    for s, x in enumerate(steps):
        got = pk.pick(torch.from_numpy(x).cuda())
        for b in range(B):
            adm = rows[b].update(T.filter_logits(x[b], rows[b].sampled, P, suppress=sup), got[b])
            if adm is None:
                assert got[b] == tok.eot
            else:
                assert got[b] in adm, (s, b, got[b], adm)
        assert int(pk.left.item()) == sum(not r.ended for r in rows)
    draws, multi = sum(r.draws for r in rows), sum(r.multi for r in rows)
    print(f"V {n_vocab} T {temperature}: {multi} of {draws} draws had more than one admissible token")
    assert multi <= SR.CAP * draws
    st = pk.state.cpu().numpy()
    sums = st[:, 5].copy().view(np.float32)
    tk = pk.tokens.cpu().numpy()
    for b in range(B):
        assert list(tk[b, :8]) == rows[b].sampled and (tk[b, 8:] == -1).all()
        assert abs(float(sums[b]) - rows[b].sum_logprob) <= 1e-5 * 8, (b, sums[b], rows[b].sum_logprob)
        assert st[b, 4] == 8 and st[b, 3] == int(rows[b].ended)
    assert any(r.ended for r in rows)  # the walk reaches eot: frozen rows were exercised
    assert all(t != 220 for t in (r.sampled[0] for r in rows)) and all(1500 not in r.sampled and tok.no_timestamps not in r.sampled for r in rows)


def test_sampled_pick_is_a_function_of_seed_stream_and_history():
    """the same (seed, streams) twice: equal tokens; row 2 alone with its stream id: its tokens in the batch; another seed: different somewhere"""
    import torch

    V, B, n = 51865, 4, 6
    tok = whisper.special_tokens(T.dims(128, 2, 1, V, 100))
    P = T.pick_params(tok, V, without_timestamps=True)
    g = np.random.default_rng(2)
    xs = [(2.0 * g.standard_normal((B, V))).astype(np.float32) for _ in range(n)]

    def run(seed, sel):
        pk = Picker(P, None, len(sel), n, 1.0, seed, [SR.PICK_STREAMS[b] for b in sel])
        out = [pk.pick(torch.from_numpy(np.ascontiguousarray(x[sel])).cuda()) for x in xs]
        return np.array(out).T, pk.state.cpu().numpy()[:, 5].copy()  # tokens (row, step) and the BITS of sum_logprob

    a, sa = run(7, [0, 1, 2, 3])
    b, sb = run(7, [0, 1, 2, 3])
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    alone, s1 = run(7, [2])
    assert np.array_equal(alone[0], a[2]) and s1[0] == sa[2]
    other, _ = run(8, [0, 1, 2, 3])
    assert not np.array_equal(other, a)
    assert len({tuple(r) for r in a}) == B  # four streams on four different logit rows: four different walks


def test_sampled_pick_never_chooses_a_masked_token():
    """suppressed ids carry logits 30 above everything else (their probability would be 1 - 1e-8); 64 draws choose none of them, nor the blank / eot at
    the first position"""
    import torch

    V, B = 51866, 16
    tok = whisper.special_tokens(T.dims(128, 2, 1, V, 100))
    P = T.pick_params(tok, V, without_timestamps=True)
    sup = (0, 31, 32, 63, 1000, 25000, 51865, tok.no_speech)
    x = SR.masked_logits(V, sup, 4)
    x[[220, tok.eot]] += np.float32(30.0)  # masked at the first sampled position only
    xd = torch.from_numpy(np.tile(x, (B, 1))).cuda()
    pk = Picker(P, sup, B, 4, 1.0, 5, range(B))
    first = pk.pick(xd)
    assert not set(first) & (set(sup) | {220, tok.eot}), first
    later = [t for _ in range(3) for t in pk.pick(xd)]
    assert not set(later) & set(sup) and set(later) <= {220, tok.eot}  # past the first position the blank and eot are free again, and 30 above the rest


@pytest.mark.parametrize("temperature", SR.PICK_TEMPERATURES)
def test_sampled_pick_draws_from_the_tempered_softmax(temperature):
    """without_timestamps, all but 8 ids masked through the bitmask (eot and the blank among the masked), 32 rows x 64 steps = 2 048 draws of fixed logits:
    every draw equals the restatement's (within the cap on ambiguous ones), and every frequency lies within five binomial standard deviations
    5 sqrt(p (1 - p) / 2048) of softmax(l / T)."""
    import torch

    V, B, n = SR.DIST_V, SR.DIST_ROWS, SR.DIST_STEPS
    tok = whisper.special_tokens(T.dims(128, 2, 1, V, 100))
    assert tok.eot not in SR.DIST_IDS and 220 not in SR.DIST_IDS
    P = T.pick_params(tok, V, without_timestamps=True)
    x = SR.dist_logits()
    xd = torch.from_numpy(np.tile(x, (B, 1))).cuda()
    pk = Picker(P, SR.dist_suppress(), B, n, temperature, SR.DIST_SEED, range(B))
    got = np.array([pk.pick(xd) for _ in range(n)])  # (step, row)
    ids = list(SR.DIST_IDS)
    f = np.full(V, -np.inf)
    f[ids] = x[ids].astype(np.float64)
    multi = 0
    for s in range(n):
        for b in range(B):
            adm, _ = SR.draw(f, temperature, SR.DIST_SEED, b, s)
            assert int(got[s, b]) in adm, (s, b, got[s, b], adm)
            multi += len(adm) > 1
    assert multi <= SR.CAP * B * n
    z = f[ids] / float(np.float32(temperature))
    p = np.exp(z - T.logsumexp(z))
    freq = np.array([(got == i).mean() for i in ids])
    dev = np.abs(freq - p) / np.maximum(np.sqrt(p * (1 - p) / (B * n)), 1e-300)
    print(f"T {temperature}: p {np.round(p, 4)}, frequencies {np.round(freq, 4)}, worst deviation {dev.max():.2f} sigma")
    assert abs(freq.sum() - 1.0) < 1e-12 and (np.abs(freq - p) <= 5.0 * np.sqrt(p * (1 - p) / (B * n))).all()
    lp = pk.state.cpu().numpy()[:, 5].copy().view(np.float32)  # the log-probabilities are those of the UNTEMPERED filtered logits
    lse = T.logsumexp(f[ids])
    for b in range(B):
        assert abs(float(lp[b]) - sum(f[int(t)] - lse for t in got[:, b])) <= 1e-5 * n


def test_sampled_pick_refuses_a_temperature_that_is_not_positive_and_finite():
    import torch

    V = 51865
    tok = whisper.special_tokens(T.dims(128, 2, 1, V, 100))
    pk = Picker(T.pick_params(tok, V, without_timestamps=True), None, 1, 4, 1.0, 0, [0])
    x = torch.zeros((1, V), dtype=torch.float32, device="cuda")
    before = pk.state.clone()
    for t in (0.0, -0.5, float("nan"), float("inf")):
        rc = pk.lib.kk_op_whisper_pick_sampled(_st(), 1, _p(x), V, _p(pk.params), None, t, 0, _p(pk.streams), _p(pk.state), _p(pk.tokens), 4, _p(pk.next), _p(pk.left))
        assert rc != 0 and b"temperature" in pk.lib.kk_last_error()
    assert torch.equal(pk.state, before) and int(pk.left.item()) == 1  # nothing was launched
