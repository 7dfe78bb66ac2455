"""The Parakeet text-side kernels on their own (csrc/kk_parakeet_text.hip) against the float64 restatements of tests/_parakeet_text_ref.py on
the same bf16-rounded operands.

Bars.  LSTM cell: 4 x the error of the same restatement computed in float32 (both printed).  Joint logits: the bound of DESIGN 8g for an fp32 dot of K
exact products, (K + 4) 2^-23 (sum |a w| + |bias|), the measured share printed.  Arg-maxima: equal to numpy's over the kernel's own logits."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _parakeet_text_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("n_in,H", [(32, 32), (96, 160), (640, 640)])
def test_lstm_cell_rows(n_in, H, M):
    from mlx_audio_amd import parakeet

    g = np.random.default_rng(100 * H + M)
    s = 1.0 / np.sqrt(H)
    wx, wh, b = g.uniform(-s, s, (4 * H, n_in)), g.uniform(-s, s, (4 * H, H)), g.uniform(-s, s, 4 * H)
    V = 7
    embed = R.bf16(g.standard_normal((V + 1, n_in)))
    token = g.integers(0, V, M)
    token[0] = V  # row 0: the blank, a zero input
    idx = g.integers(0, 2, M)
    idx[-1] = 1  # the last row is committed to copy 1
    mask = np.ones(M, np.int64)
    if M > 1:
        mask[1] = 0  # row 1 is masked: its proposed state stays as it is
    hc = g.standard_normal((2, 2, M, H))  # (h | c), copy, row
    h_in, c_in = hc[0][idx, np.arange(M)], hc[1][idx, np.arange(M)]
    x = np.where((token == V)[:, None], 0.0, embed[token])
    want_h, want_c = R.lstm_cell(x, h_in, c_in, wx, wh, b)
    f32_h, f32_c = R.lstm_cell(x, h_in, c_in, wx, wh, b, np.float32)

    def run(rows):
        w, bp = parakeet.pack_lstm(wx, wh, b)
        h, c = dev(hc[0][:, rows]), dev(hc[1][:, rows])
        for r, m in enumerate(rows):
            h[1 - idx[m], r] = c[1 - idx[m], r] = float("nan")
        parakeet.lstm_cell_rows(w, bp, h, c, dev(idx[rows], torch.int32), dev(mask[rows], torch.int32), embed=dev(embed, torch.bfloat16),
                                token=dev(token[rows], torch.int32), blank=V)
        torch.cuda.synchronize()
        h, c = h.cpu().numpy(), c.cpu().numpy()
        return np.stack([h[1 - idx[m], r] for r, m in enumerate(rows)]), np.stack([c[1 - idx[m], r] for r, m in enumerate(rows)]), h, c

    rows = np.arange(M)
    got_h, got_c, h_all, c_all = run(rows)
    on = mask == 1
    assert np.isnan(got_h[~on]).all() and np.isnan(got_c[~on]).all()
    assert np.array_equal(h_all[idx, rows], hc[0][idx, rows].astype(np.float32))  # the committed copies are only read
    err = max(np.abs(got_h[on] - want_h[on]).max(), np.abs(got_c[on] - want_c[on]).max())
    ref = max(np.abs(f32_h[on] - want_h[on]).max(), np.abs(f32_c[on] - want_c[on]).max())
    print(f"lstm_cell_rows in={n_in} H={H} M={M}: max error {err:.3e}, float32 restatement {ref:.3e}")
    assert err <= 4 * ref
    m = M - 1  # a row alone is bit-equal to the same row in the batch
    one_h, one_c, _, _ = run(np.array([m]))
    assert np.array_equal(one_h[0], got_h[m]) and np.array_equal(one_c[0], got_c[m])
    # the fp32 input form (an upper layer) gives the same bits as the embedding form on the same values
    w, bp = parakeet.pack_lstm(wx, wh, b)
    h, c = dev(hc[0]), dev(hc[1])
    parakeet.lstm_cell_rows(w, bp, h, c, dev(idx, torch.int32), dev(mask, torch.int32), x=dev(x))
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy()[1 - idx, rows][on], got_h[on])


@pytest.mark.parametrize("M", [1, 16])
@pytest.mark.parametrize("act", ["relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("n_tok,n_dur", [(5, 0), (38, 5), (1025, 5)])
@pytest.mark.parametrize("Hj", [32, 160, 640])
def test_joint_argmax(Hj, n_tok, n_dur, act, M):
    from mlx_audio_amd import parakeet

    g = np.random.default_rng(Hj + n_tok + M)
    Cn, T = n_tok + n_dur, 5
    w, b = R.bf16(g.standard_normal((Cn, Hj)) / np.sqrt(Hj)), g.standard_normal(Cn)
    if n_tok > 20:  # two bit-identical rows in different tiles, above all others: the lower index must win
        w[19], b[2], b[19] = w[2], 50.0, 50.0
    encp, predp = g.standard_normal((M, T, Hj)).astype(np.float32), g.standard_normal((M, Hj)).astype(np.float32)
    t = g.integers(0, T, M)
    tok, dur, logits = parakeet.joint_argmax(dev(w, torch.bfloat16), dev(b), dev(encp), dev(t, torch.int32), dev(predp), n_tok, act, want_logits=True)
    torch.cuda.synchronize()
    tok, dur, logits = tok.cpu().numpy(), dur.cpu().numpy(), logits.cpu().numpy()
    rows = encp[np.arange(M), t]
    want = R.joint_logits(rows, predp, w, b, act)
    a = R.bf16(R.ACTS[act]((rows + predp).astype(np.float64)))
    bound = (Hj + 4) * 2.0 ** -23 * (np.abs(a) @ np.abs(w).T + np.abs(b))
    share = (np.abs(logits - want) / bound).max()
    print(f"joint_argmax Hj={Hj} C={Cn} {act} M={M}: max error {np.abs(logits - want).max():.3e}, {share:.3f} of the bound")
    assert share <= 1.0
    assert np.array_equal(tok, logits[:, :n_tok].argmax(1))
    if n_dur:
        assert np.array_equal(dur, logits[:, n_tok:].argmax(1))
    if n_tok > 20:
        assert (logits[:, 2] == logits[:, 19]).all() and (tok == 2).all()


@pytest.mark.parametrize("rows", [1, 17, 40])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ctc_argmax(rows, dtype):
    from mlx_audio_amd import parakeet

    g = np.random.default_rng(rows)
    K, Cn = 128, 38
    w, b, feat = R.bf16(g.standard_normal((Cn, K)) / np.sqrt(K)), g.standard_normal(Cn), g.standard_normal((rows, K)).astype(np.float32)
    ids, logits = parakeet.ctc_argmax(dev(w, torch.bfloat16), dev(b), dev(feat, dtype), want_logits=True)
    torch.cuda.synchronize()
    ids, logits = ids.cpu().numpy(), logits.cpu().numpy()
    want = R.linear(feat, w, b)
    bound = (K + 4) * 2.0 ** -23 * (np.abs(R.bf16(feat)) @ np.abs(w).T + np.abs(b))
    assert (np.abs(logits - want) <= bound).all() and np.array_equal(ids, logits.argmax(1))
