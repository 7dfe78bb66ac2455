"""Pins the references of tests/_mimi_ref.py, so that a wrong reference cannot excuse a wrong kernel:
  * the float64 ones to 1e-12 against torch's float64 conv1d / conv_transpose1d / elu / tanh-gelu, with the paddings the codec uses
    (causal conv: left pad (K - 1) dil; causal transposed conv: the last K - stride rows dropped; strided causal conv: left pad K - stride and
    zero rows on the right up to ceil(L / stride) outputs);
  * the bit references against the pieces of oracle/mimi_oracle.py that can be called alone (RVQ decode sum, depth-wise up-sample, RoPE, edge
    pad, code-book search).  The oracle computes in fp32, so these comparisons run on small-integer data, on which every fp32 product and sum
    is exact and equality is asked; RoPE, whose cos / sin are fp32 in the oracle, is held to fp32 round-off there and to 1e-12 against a
    float64 complex rotation."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _mimi_ref as R  # noqa: E402
import mimi_oracle as M  # noqa: E402

TOL = 1e-12


def _close(got, ref):
    ref = np.asarray(ref)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= TOL * max(1.0, np.abs(ref).max())


def _t(x):  # [L][C] -> torch [1][C][L] float64
    return torch.tensor(np.asarray(x, np.float64)).T[None]


def _w(w):  # [O][K][I] -> torch conv1d weight [O][I][K]
    return torch.tensor(np.asarray(w, np.float64)).permute(0, 2, 1)


@pytest.mark.parametrize("K,dil", [(1, 1), (3, 1), (7, 1), (3, 2), (16, 1)])
def test_causal_conv(K, dil):
    rng = np.random.default_rng(K * 10 + dil)
    L, I, O = 11, 5, 4
    x, w, b = rng.standard_normal((L, I)), rng.standard_normal((O, K, I)), rng.standard_normal(O)
    ref = F.conv1d(F.pad(_t(x), ((K - 1) * dil, 0)), _w(w), torch.tensor(b), dilation=dil)[0].T.numpy()
    got, ab = R.conv(x, w, b, pad=(K - 1) * dil, dil=dil, Lout=L, absum=True)
    _close(got, ref)
    ref_ab = F.conv1d(F.pad(_t(np.abs(x)), ((K - 1) * dil, 0)), _w(np.abs(w)), torch.tensor(np.abs(b)), dilation=dil)[0].T.numpy()
    _close(ab, ref_ab)


def test_noncausal_pad_conv():
    rng = np.random.default_rng(5)
    L, I, O, K = 9, 3, 2, 7
    x, w = rng.standard_normal((L, I)), rng.standard_normal((O, K, I))
    ref = F.conv1d(F.pad(_t(x), (2, K - 1 - 2)), _w(w))[0].T.numpy()  # pad 2 on the left: rows >= L are met on the right
    _close(R.conv(x, w, None, pad=2, Lout=L), ref)


@pytest.mark.parametrize("r,L", [(4, 10), (5, 13), (2, 8), (8, 17)])
def test_strided_causal_conv(r, L):
    rng = np.random.default_rng(r + L)
    K, I, O = 2 * r, 3, 4
    x, w, b = rng.standard_normal((L, I)), rng.standard_normal((O, K, I)), rng.standard_normal(O)
    Lo = -(-L // r)
    right = (Lo - 1) * r + K - (K - r) - L
    assert right >= 0
    ref = F.conv1d(F.pad(_t(x), (K - r, right)), _w(w), torch.tensor(b), stride=r)[0].T.numpy()
    assert ref.shape[0] == Lo
    _close(R.conv(x, w, b, pad=K - r, stride=r, Lout=Lo), ref)


@pytest.mark.parametrize("s", [1, 2, 4, 5, 6, 8])
def test_causal_transposed_conv(s):
    rng = np.random.default_rng(s)
    K, L, I, O = 2 * s, 6, 5, 3
    x, w, b = rng.standard_normal((L, I)), rng.standard_normal((O, K, I)), rng.standard_normal(O)
    y = F.conv_transpose1d(_t(x), torch.tensor(w).permute(2, 0, 1), torch.tensor(b), stride=s)
    ref = y[0, :, : y.shape[-1] - (K - s)].T.numpy()
    assert ref.shape[0] == L * s
    got, ab = R.conv_transposed(x, w, b, stride=s, Lout=L * s, absum=True)
    _close(got, ref)
    ya = F.conv_transpose1d(_t(np.abs(x)), torch.tensor(np.abs(w)).permute(2, 0, 1), torch.tensor(np.abs(b)), stride=s)
    _close(ab, ya[0, :, : L * s].T.numpy())


def test_transposed_conv_with_pad():
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal((5, 2)), rng.standard_normal((3, 7, 2))
    ref = F.conv_transpose1d(_t(x), torch.tensor(w).permute(2, 0, 1), stride=3, padding=2)[0].T.numpy()
    _close(R.conv_transposed(x, w, None, stride=3, pad=2, Lout=ref.shape[0]), ref)  # torch trims `padding` rows at both ends


def test_elu_gelu_cout1():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((13, 6)) * 3
    _close(R.elu(x), F.elu(torch.tensor(x)).numpy())
    _close(R.gelu_tanh(x), F.gelu(torch.tensor(x), approximate="tanh").numpy())
    w, b = rng.standard_normal((7, 6)), 0.3
    ref = F.conv1d(F.pad(_t(R.elu(x)), (6, 0)), _w(w[None]), torch.tensor([b], dtype=torch.float64))[0, 0].numpy()
    got, ab = R.conv_cout1(R.elu(x), w, b, pad=6)
    _close(got, ref)
    assert (ab >= np.abs(got) - 1e-12).all()
    ref2 = F.conv1d(F.pad(_t(x), (2, 4)), _w(w[None]))[0, 0].numpy()
    _close(R.conv_cout1(x, w, None, pad=2)[0], ref2)


def test_bf16_round_and_ties():
    rng = np.random.default_rng(2)
    a = (rng.standard_normal(4096) * 10).astype(np.float32)
    a[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]  # ties: to even (1.0, 1.015625, -1.0)
    ref = torch.tensor(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bf16_round(a), ref)
    # midpoints of neighbouring bf16 values are ties; the bf16 values themselves are not
    v = np.array([1.0, 1.0078125, 3.5, 0.07373046875], np.float64)
    assert not R.near_bf16_tie(v).any()
    up = v + 2.0 ** (np.floor(np.log2(v)) - 7)  # the next bf16 value
    assert np.array_equal(R.bf16_round(up.astype(np.float32)), up)
    assert (up > v).all()
    assert R.near_bf16_tie((v + up) / 2).all()
    assert R.near_bf16_tie((v + up) / 2 * (1 + 2.0**-15)).all() and not R.near_bf16_tie((v + up) / 2 * (1 + 2.0**-12)).any()
    x = R.bf16_round(-rng.uniform(1 / 16, 4, 20000).astype(np.float32))
    y = R.avoid_elu_ties(x)
    changed = y != x
    assert 0 < changed.mean() < 0.1 and np.array_equal(y[changed], -x[changed])
    # after the rule, a relative error of 1e-5 on elu (far above the device exp's) cannot change the bf16 rounding
    e = R.elu(y)
    for f in (1 - 1e-5, 1 + 1e-5):
        assert np.array_equal(R.bf16_round((e * f).astype(np.float32)), R.bf16_round(e.astype(np.float32)))


def _oracle(cfg, w=None):
    return M.MimiOracle(w or {}, cfg)


def test_rvq_sum_against_oracle():
    rng = np.random.default_rng(4)
    nq, bins, qdim, Nf = 4, 5, 6, 3
    cb = rng.integers(-8, 9, (nq, bins, qdim)).astype(np.float32)
    codes = rng.integers(0, bins, (nq, Nf))
    w = {}
    for which, ids in (("rvq_first", [0]), ("rvq_rest", [1, 2, 3])):
        for j, i in enumerate(ids):
            w[f"quantizer.{which}.vq.layers.{j}.codebook.embedding_sum"] = cb[i] * 2
            w[f"quantizer.{which}.vq.layers.{j}.codebook.cluster_usage"] = np.full(bins, 2.0, np.float32)
        w[f"quantizer.{which}.output_proj.weight"] = np.eye(qdim, dtype=np.float32)[:, None, :]  # identity 1x1 projection
    orc = _oracle({}, w)
    first, rest = R.rvq_sum(codes, cb)
    assert np.array_equal(first, orc.rvq_decode("rvq_first", codes[None, :1])[0].T.numpy())
    assert np.array_equal(rest, orc.rvq_decode("rvq_rest", codes[None, 1:])[0].T.numpy())
    # clamping and nq == 1; the fp32 order on non-integer data
    f1, r1 = R.rvq_sum(np.array([[-1, bins, 2]]), cb[:1])
    assert np.array_equal(f1, cb[0][[0, bins - 1, 2]]) and not r1.any()
    cbf = rng.standard_normal((nq, bins, qdim)).astype(np.float32)
    _, rf = R.rvq_sum(codes, cbf)
    e = [cbf[i][codes[i]] for i in range(nq)]
    assert np.array_equal(rf, np.float32(np.float32(e[1] + e[2]) + e[3])) and rf.dtype == np.float32


@pytest.mark.parametrize("s", [1, 2, 3])
def test_upsample_against_oracle(s):
    rng = np.random.default_rng(s)
    Lin, C = 5, 7
    x = rng.integers(-8, 9, (Lin, C)).astype(np.float32)
    w = rng.integers(-8, 9, (2 * s, C)).astype(np.float32)
    orc = _oracle({"upsample_stride": s}, {"upsample.convtr.convtr.convtr.weight": w[None]})
    ref = orc.upsample(torch.tensor(x).T[None])[0].T.numpy()
    assert np.array_equal(R.upsample_dw(x, w, s), ref)
    # and the float64 transposed conv of this file on real-valued data: the dense eye-masked weight of the reference
    xf, wf = rng.standard_normal((Lin, C)), rng.standard_normal((2 * s, C))
    dense = np.zeros((C, 2 * s, C))
    for c in range(C):
        dense[c, :, c] = wf[:, c]
    got = R.upsample_dw(xf, wf, s).astype(np.float64)
    ref64 = R.conv_transposed(np.float32(xf), np.float32(dense), None, stride=s, Lout=Lin * s)
    assert np.abs(got - ref64).max() <= 4 * 2.0**-24 * np.abs(ref64).max() + 1e-6  # three fp32 roundings


def test_rope_against_oracle_and_float64():
    rng = np.random.default_rng(6)
    T, H, hd = 5, 2, 64
    D = H * hd
    inv = (10000.0 ** (-np.arange(hd // 2, dtype=np.float32) / np.float32(hd // 2))).astype(np.float32)
    qkv = rng.standard_normal((T, 3 * D + 4))
    orc = _oracle({"rope_base": 10000.0})
    for t in range(T):
        got, scale = R.rope(qkv[t], inv, t, D, hd)
        assert np.array_equal(got[2 * D :], qkv[t, 2 * D :])  # v and the pad columns
        for third in range(2):
            for h in range(H):
                seg = slice(third * D + h * hd, third * D + (h + 1) * hd)
                z = (qkv[t, seg][0::2] + 1j * qkv[t, seg][1::2]) * np.exp(1j * (np.float32(t) * inv).astype(np.float64))
                _close(got[seg][0::2], z.real)
                _close(got[seg][1::2], z.imag)
                assert np.array_equal(scale[seg][0::2], np.abs(qkv[t, seg][0::2]) + np.abs(qkv[t, seg][1::2]))
    # the oracle (fp32 cos / sin): [B][H][T][hd]
    q = qkv[:, :D].reshape(T, H, hd).transpose(1, 0, 2)[None]
    ref = orc.rope(torch.tensor(q, dtype=torch.float32))[0].numpy()
    got = np.stack([R.rope(qkv[t], inv, t, D, hd)[0][:D].reshape(H, hd) for t in range(T)], axis=1)
    assert np.abs(got - ref).max() < 5e-6


def test_edge_pad_against_torch():
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    for left, extra in [(2, 0), (2, 3), (0, 1), (5, 5)]:
        ref = F.pad(torch.tensor(x).T[None], (left, extra), mode="replicate")[0].T.numpy()
        assert np.array_equal(R.edge_pad(x, left, left + 4 + extra), ref)
    assert np.array_equal(R.edge_pad(x[:1], 2, 4), np.repeat(x[:1], 4, 0))


def test_rvq_argmin_against_oracle():
    rng = np.random.default_rng(7)
    bins, qdim, T = 9, 4, 6
    E = rng.integers(-4, 5, (bins, qdim)).astype(np.float32) * 2  # |e|^2 / 2 is an integer
    E[5] = E[2]  # a tie: the lower index wins
    res = rng.integers(-4, 5, (T, qdim)).astype(np.float32)
    w = {"quantizer.rvq_first.vq.layers.0.codebook.embedding_sum": E, "quantizer.rvq_first.vq.layers.0.codebook.cluster_usage": np.ones(bins, np.float32),
         "quantizer.rvq_first.input_proj.weight": np.eye(qdim, dtype=np.float32)[:, None, :]}
    ref_codes = _oracle({}, w).rvq_encode("rvq_first", torch.tensor(res).T[None], 1)[0, 0]
    c2 = (E * E).sum(-1) / 2
    codes, new = R.rvq_argmin(res @ E.T, c2, E, res)
    assert np.array_equal(codes, ref_codes) and 5 not in codes
    assert np.array_equal(new, res - E[ref_codes])
    # NaN distances are skipped; a row with none below +inf gives bins - 1
    d = (res @ E.T).astype(np.float32)
    d[0, codes[0]] = np.nan
    d[1, :] = np.nan
    d[2, :] = -np.inf  # v = +inf everywhere
    c3, n3 = R.rvq_argmin(d, c2, E, res)
    assert c3[0] != codes[0] and c3[1] == bins - 1 and c3[2] == bins - 1 and np.array_equal(c3[3:], codes[3:])
    v0 = c2 - d[0]
    assert c3[0] == int(np.nanargmin(v0))
    assert np.array_equal(n3[1], res[1] - E[bins - 1])


def test_state_refs():
    buf = np.arange(7 * 2, dtype=np.float32).reshape(7, 2)
    out = R.state_shift(buf, 6, 1)  # overlapping: every row read before any is written
    assert np.array_equal(out[:6], buf[1:7]) and np.array_equal(out[6:], buf[6:])
    out = R.state_shift(buf, 2, 5)
    assert np.array_equal(out[:2], buf[5:7]) and np.array_equal(out[2:], buf[2:])
    out = R.state_edge_fill(buf, 3)
    assert np.array_equal(out[:3], np.repeat(buf[3:4], 3, 0)) and np.array_equal(out[3:], buf[3:])
