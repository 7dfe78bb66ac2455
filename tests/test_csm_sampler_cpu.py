"""The CSM sampler's host surface and the numpy restatement of its rule and RNG (tests/_sampler_ref.py), without a GPU: make_sampler carries
and checks the whole mlx_lm argument family, Philox4x32-10 reproduces the Random123 known answers, the rule reduces to the oracle's top-k
sampler, and generate_audio's keyword pass-through reaches the frame generator."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sampler_ref as R  # noqa: E402
import csm_oracle as C  # noqa: E402
from mlx_audio_amd.sesame import Model, Sampler, Segment, make_sampler  # noqa: E402


def test_make_sampler_carries_and_checks_every_argument():
    s = make_sampler(temp=0.8, top_p=0.95, min_p=0.05, min_tokens_to_keep=2, top_k=0)
    assert (s.temp, s.top_k, s.top_p, s.min_p, s.min_tokens_to_keep) == (0.8, 0, 0.95, 0.05, 2)
    d = make_sampler()
    assert d == Sampler(0.9, 50) and (d.top_p, d.min_p, d.min_tokens_to_keep) == (0.0, 0.0, 1)
    assert make_sampler(0.7, top_k=-1).top_k == -1  # "off", as llama.py:229 of the reference passes it
    assert make_sampler(temp=0.5, logit_bias=None, xtc_threshold=0.1, xtc_probability=0.0) == Sampler(0.5, 50)  # unknown keywords stay ignored
    for bad in (dict(top_p=1.5), dict(top_p=-0.1), dict(min_p=1.01), dict(min_p=-1e-3), dict(min_tokens_to_keep=0), dict(top_k=-2)):
        with pytest.raises(ValueError):
            make_sampler(**bad)
    with pytest.raises(ValueError, match="[Xx][Tt][Cc]"):
        make_sampler(temp=0.8, xtc_probability=0.5)


def test_philox_restatement_reproduces_random123_known_answers():
    assert R.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert R.philox4x32_10([R.M32] * 4, [R.M32] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    u = [R.device_uniform(s, sid, pos, cb) for s in (0, 1, 2**63 + 5) for sid in (0, 7) for pos in (0, 1, 300) for cb in (0, 31)]
    assert all(0.0 < float(x) < 1.0 for x in u) and len({float(x) for x in u}) == len(u)


@pytest.mark.parametrize("V", [67, 1100, 2051, 4000])
def test_rule_reduces_to_the_oracle_sampler_when_only_top_k_is_set(V):
    """Rows of test_csm_sampler_matches_oracle_incl_tie_walls; targets at the midpoints of the CDF intervals (the oracle sums in float32, the
    rule in float64), only where an interval is wider than 1e-5 of the mass (a float32 sum of <= 64 terms is good to 64 * 2^-24 = 4e-6)."""
    rng = np.random.default_rng(V)
    rows = [rng.standard_normal(V) * 3, np.round(rng.standard_normal(V) * 2) / 2, np.zeros(V), np.round(rng.standard_normal(V)),
            np.where(rng.uniform(size=V) < 0.5, -np.inf, rng.standard_normal(V)), -np.abs(rng.standard_normal(V)) * 50]
    lg = np.stack(rows).astype(np.float32)
    checked = 0
    for temp, top_k in ((0.9, 50), (0.7, 5), (1.3, 64)):
        for b in range(lg.shape[0]):
            n, order, p, d = R.kept(lg[b], top_k=top_k)
            assert n == min(top_k, V)
            c = np.concatenate([[0.0], R.cdf(d, n, temp)])
            for j in range(n):
                if c[j + 1] - c[j] < 1e-5:
                    continue
                u = np.float32(0.5 * (c[j] + c[j + 1]))
                want = C.sample(torch.tensor(lg[b : b + 1]), temp, min(top_k, V), np.array([u], np.float32))[0]
                assert R.pick(lg[b], temp, u, top_k=top_k) == want == order[j], (temp, top_k, b, j)
                checked += 1
    assert checked > 100


def test_rule_filters_on_a_hand_made_row():
    """p = (0.5, 0.25, 0.125, 0.0625, 0.0625) in index order 2, 0, 4, 1, 3 (the last two tie: the lower index first)."""
    l = np.log(np.array([0.25, 0.0625, 0.5, 0.0625, 0.125]))
    n, order, p, _ = R.kept(l)
    assert n == 5 and order.tolist() == [2, 0, 4, 1, 3]
    assert R.kept(l, top_p=0.5)[0] == 1 and R.kept(l, top_p=0.51)[0] == 2 and R.kept(l, top_p=0.76)[0] == 3  # mass BEFORE the token < top_p
    assert R.kept(l, min_p=0.2)[0] == 3 and R.kept(l, min_p=0.6)[0] == 1 and R.kept(l, min_p=0.6, min_keep=3)[0] == 3
    assert R.kept(l, top_k=4, top_p=0.99, min_p=0.2)[0] == 3 and R.kept(l, top_k=2, top_p=0.99, min_p=0.2)[0] == 2
    assert R.kept(l, top_k=-1)[0] == 5 and R.kept(l, top_k=7)[0] == 5
    # the temperature acts in the draw only: kept set from p at temperature 1, weights (p / p_max) ** (1 / temp) inside it
    assert [R.pick(l, 0.5, u, top_p=0.76) for u in (0.75, 0.77, 0.94, 0.96)] == [2, 0, 0, 4]  # weights 1, 1/4, 1/16: cdf 0.762, 0.952, 1
    assert R.pick(l, 0.5, np.float32(1.0) - np.float32(2**-24), min_p=0.2) == 4
    nan_row = np.array([np.nan, 1.0, np.nan, 0.0])
    assert R.kept(nan_row)[1].tolist() == [1, 3, 0, 2] and R.pick(nan_row, 1.0, 0.999999) == 3


class _FakeCsm:
    """Records what the frame loop hands the frame generator."""
    cfg = {"max_seq_len": 64, "audio_num_codebooks": 2}
    device = torch.device("cpu")

    def __init__(self):
        self.max_batch, self.calls = 0, []

    def caches_are_enabled(self):
        return self.max_batch > 0

    def setup_caches(self, B):
        self.max_batch = B

    def reset_caches(self):
        pass

    def set_padding(self, pads):
        pass

    def set_graph_mode(self, on):
        pass

    def generate_frame(self, tok, msk, **kw):
        self.calls.append(kw)
        return torch.full((tok.shape[0], 2), 7, dtype=torch.int32)


class _FakeMimi:
    def encode(self, x):
        return torch.ones((x.shape[0], 2, 3), dtype=torch.int64)

    def decode(self, codes):
        return torch.zeros((codes.shape[0], 1, codes.shape[2] * 1920))


def test_generate_audio_passes_sampler_rng_and_seed_through_to_the_frame_generator(tmp_path, monkeypatch):
    from mlx_audio_amd import generate as G

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda *a, **k: 0)
    csm = _FakeCsm()
    m = Model(dict(csm.cfg, backbone={}, decoder={}, text_vocab_size=10, audio_vocab_size=10), mimi=_FakeMimi(), csm=csm)
    ref = np.zeros(1920 * 3, np.float32)
    seed = zlib.crc32(b"pass-through")
    ctx = [Segment(speaker=0, text=[1, 2, 3], audio=ref)]  # (generate_audio's ref_audio is a file path; a context goes through **kwargs)
    kw = dict(model=m, context=ctx, max_audio_length_ms=80 * 3, stop_on_eos=False, verbose=False)
    G.generate_audio([4, 5, 6], file_prefix=str(tmp_path / "a"), sampler=make_sampler(0.8, top_p=0.95, top_k=0), rng="device", seed=seed,
                     top_p=0.1, top_k=3, **kw)  # the bare top_p= / top_k= are ignored, as the reference's signature ignores them
    assert len(csm.calls) == 3
    for c in csm.calls:
        assert c["sampler"] == Sampler(0.8, 0, 0.95) and c["seed"] == seed and c["uniforms"] is None and c["stream_ids"] is None
    # the default sampler on host uniforms: the call a frame generator has always received
    csm.calls.clear()
    G.generate_audio([4, 5, 6], file_prefix=str(tmp_path / "b"), seed=seed, **kw)
    assert len(csm.calls) == 3 and all(set(c) == {"temperature", "top_k", "uniforms"} and (c["temperature"], c["top_k"]) == (0.9, 50) for c in csm.calls)
    assert all(tuple(c["uniforms"].shape) == (1, 2) for c in csm.calls)
    # host uniforms with a filter: the sampler travels, the uniforms still come from numpy
    csm.calls.clear()
    G.generate_audio([4, 5, 6], file_prefix=str(tmp_path / "c"), sampler=make_sampler(0.8, min_p=0.05), seed=seed, **kw)
    assert all(c["sampler"].min_p == 0.05 and c["seed"] is None and c["uniforms"] is not None for c in csm.calls)
    with pytest.raises(ValueError):
        list(m.generate([4, 5, 6], context=ctx, rng="gpu"))
