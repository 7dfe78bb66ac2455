"""Pins the restatements of tests/_kokoro_ref.py, which tests/test_gpu_kokoro_kernels.py compares the kernels with, against independent sources:
torch float64 (embedding + layer_norm, softmax attention, nn.LSTM, stft), oracle/kokoro_oracle.py (the harmonic source with injected noise) and
tests/_sampler_ref.py (Philox4x32-10).  Also the host surface of ABI minor 29."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import _kokoro_ref as R
import _sampler_ref as SR
import kokoro_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"kk_op_kokoro_style_fc": 8, "kk_op_kokoro_fill_style": 11, "kk_op_kokoro_embedding": 10, "kk_op_kokoro_duration": 14,
           "kk_op_kokoro_alignment": 8, "kk_op_kokoro_gather_rows": 13, "kk_op_kokoro_copy_slice": 11, "kk_op_kokoro_lens": 7,
           "kk_op_kokoro_convert": 10, "kk_op_albert_embed": 15, "kk_op_source_stft_ragged": 16}


def test_abi_minor_and_signatures():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_version() == 2 and lib.kk_abi_minor() >= 29
    hdr = open(os.path.join(ROOT, "include", "kokoro_hip.h")).read()
    assert int(re.search(r"#define KK_ABI_MINOR (\d+)", hdr).group(1)) == lib.kk_abi_minor()
    for name, n in ENTRIES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"{name}(" in hdr, name
        assert len(_lib.SIGNATURES[name][1]) == n, (name, n)
    # the older entry keeps its signature and its refusal of ragged lengths
    assert len(_lib.SIGNATURES["kk_op_source_stft"][1]) == 15


def test_albert_embed_against_torch():
    rng = np.random.default_rng(1)
    for E in (64, 200, 512):
        V, T = 11, 6
        word, pos, typ = (rng.standard_normal(s).astype(np.float32) for s in ((V, E), (T, E), (2, E)))
        lw, lb = rng.standard_normal(E).astype(np.float32), rng.standard_normal(E).astype(np.float32)
        ids = np.array([0, V - 1, 3, 3, 7, 1])
        got, _ = R.albert_embed(ids, word, pos, typ, lw, lb, 1e-12)
        x = F.embedding(torch.tensor(ids), torch.tensor(word).double()) + torch.tensor(pos).double() + torch.tensor(typ).double()[0]
        ref = F.layer_norm(x, (E,), torch.tensor(lw).double(), torch.tensor(lb).double(), 1e-12).numpy()
        assert np.abs(got - ref).max() < 1e-12


def test_glue_restatements():
    table = np.arange(12, dtype=np.float32).reshape(4, 3)
    ids = np.array([[3, 0, 2], [1, 9, 9], [9, 9, 9]])
    got = R.embedding(ids, table, [3, 1, 0])
    ref = F.embedding(torch.tensor(ids[0]), torch.tensor(table)).numpy()
    assert np.array_equal(got[0], ref) and np.array_equal(got[1, 0], table[1]) and not got[1, 1:].any() and not got[2].any()
    # alignment by hand: durations 2, 0, -3, 3 of which 3 tokens are valid -> frames 0 0; with 4 valid: 0 0 3 3 3; cut at Fmax = 4 inside token 3
    dur = np.array([[2, 0, -3, 3], [2, 0, -3, 3], [5, 5, 5, 5]], np.int32)
    idx, lenF = R.alignment(dur, [3, 4, 0], 4)
    assert idx.tolist() == [[0, 0, 0, 0], [0, 0, 3, 3], [0, 0, 0, 0]] and lenF.tolist() == [2, 4, 0]
    assert R.lens4([3, 0], 10, 6, 5).tolist() == [[6, 0], [60, 0], [361, 0], [1800, 0]]
    # the constructed roundings of the duration head: half to even, and the clamp
    assert np.rint(np.float32(25.0) / np.float32(2.0)) == 12 and np.rint(np.float32(27.0) / np.float32(2.0)) == 14
    assert max(1.0, np.rint(np.float32(25.0) / np.float32(100.0))) == 1


def test_duration_seeds_leave_few_rows_undecided():
    for seed in R.DURATION_SEEDS:
        for bf16 in (False, True):
            c = R.duration_case(seed, bf16)
            valid = np.zeros((c["B"], c["T"]), bool)
            for b, n in enumerate(c["lens"]):
                valid[b, :n] = True
            assert (valid & ~c["sure"]).sum() <= 0.02 * valid.sum()
            assert c["d"][valid].min() > 2 and c["bound"][valid].max() < 1e-3  # rounding, not the clamp, decides; the bound is far under 1/2


def test_attention_against_torch():
    rng = np.random.default_rng(2)
    for L, heads in ((1, 1), (33, 3), (129, 1)):
        hs = heads * 64
        qkv = rng.standard_normal((L, 3 * hs + 5)) * 1.5
        got, W, A = R.attention(qkv, heads)
        t = torch.tensor(qkv[:, : 3 * hs])
        q, k, v = [t[:, i * hs : (i + 1) * hs].view(L, heads, 64).permute(1, 0, 2) for i in range(3)]
        ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).permute(1, 0, 2).reshape(L, hs).numpy()
        assert np.abs(got - ref).max() < 1e-12
        assert (W + 1e-15 >= np.abs(got)).all() and (A > 0).all()


def test_lstm_against_torch():
    rng = np.random.default_rng(3)
    for H, L in ((16, 1), (48, 9)):
        I = 7
        m = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
        x = rng.standard_normal((L + 2, I))
        xproj = np.zeros((L + 2, 2, 4 * H))
        whT = np.zeros((2, H, 4 * H))
        for di, sfx in enumerate(("", "_reverse")):
            wih, whh, bih, bhh = (getattr(m, f"{n}_l0{sfx}").detach().numpy() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            xproj[:, di] = x @ wih.T + bih + bhh
            whT[di] = whh.T
        xproj[L:] = np.nan  # rows past the length are not read
        got, err = R.lstm(xproj, whT, L)
        ref = m(torch.tensor(x[None, :L]))[0][0].detach().numpy()
        assert np.abs(got - ref).max() < 1e-12 and not err.any()
        _, err = R.lstm(xproj, whT, L, u_gate=2.0**-22, u_dot=2.0**-24, u_op=2.0**-24)
        # the carried bound is a worst case: it grows by about sum_j |Wh[:, j]| per step (3.5 for torch's initialisation at H = 48), which is
        # why the GPU cases draw Wh with sum |w| = 1 per row
        assert 0 < err.max() < 1e-3 and err[0, :H].max() < 4e-6


def test_stft20_against_torch():
    rng = np.random.default_rng(4)
    win = np.array([0.5 * (1 - math.cos(2 * math.pi * n / 19)) for n in range(20)])  # utils.py:10-14
    for N in (20, 37, 300):
        x = rng.standard_normal(N + 9)
        re, im, S = R.stft20(x, N, exact_tables=True)
        X = torch.stft(torch.tensor(x[:N]), 20, hop_length=5, win_length=20, window=torch.tensor(win), center=True, pad_mode="reflect",
                       return_complex=True).numpy().T
        assert X.shape == re.shape == (N // 5 + 1, 11)
        assert np.abs(re - X.real).max() < 1e-12 and np.abs(im[:, 1:10] - X.imag[:, 1:10]).max() < 1e-12
        assert np.abs(X.imag[:, [0, 10]]).max() < 1e-12 and not im[:, [0, 10]].any()
        # the float32 tables and frame products of the kernel's form stay within float32 round-off of it
        x32 = x.astype(np.float32)
        re32, im32, S32 = R.stft20(x32, N)
        ree, ime, _ = R.stft20(x32, N, exact_tables=True)
        assert np.abs(re32 - ree).max() < 4 * 2.0**-24 * S32.max() * 2 and np.abs(im32 - ime).max() < 4 * 2.0**-24 * S32.max() * 2
    # shorter than the padding (the reference refuses it): numpy's reflect mode is the statement
    x = rng.standard_normal(5)
    assert np.array_equal(x[R.reflect_index(np.arange(-10, 15), 5)], np.pad(x, 10, mode="reflect"))
    assert np.array_equal(x[R.reflect_index(np.arange(-10, 30), 5)], np.pad(x, (10, 25), mode="reflect"))
    hann, cs, sn = R.stft_tables()
    assert np.array_equal(hann, O.hanning(20).astype(np.float32)) and cs[5] == 0 and sn[10] == 0


def test_source_against_oracle():
    """The float32 restatement of the phase accumulator and of the sine's argument, with the sine, the mix and tanh in float64, against the
    oracle's float32 har_features on injected noise: voiced, unvoiced and negative F0, F0 exactly 10 (unvoiced: the test is f0 > 10)."""
    import mlx_audio_amd.params as Pm

    rng = np.random.default_rng(5)
    lw = (rng.standard_normal((1, 9)) * 0.7).astype(np.float32)
    lb = np.array([0.05], np.float32)
    orc = O.KokoroOracle({"decoder.generator.m_source.l_linear.weight": lw, "decoder.generator.m_source.l_linear.bias": lb}, Pm.tiny_config())
    L2 = 12
    f0 = (rng.standard_normal(L2) * 80 + 150).astype(np.float32)
    f0[2:4] = -3.0
    f0[5] = 10.0
    f0[6] = 0.0
    noise = rng.standard_normal((300 * L2, 9)).astype(np.float32)
    _, hs_ref = orc.har_features(f0[None], None, noise[None])
    phase = R.source_phase32(f0)
    ph, lo_w, hi = R.source_arg32(phase, L2)
    assert lo_w[0] == L2 - 1 and lo_w[149] == L2 - 1 and lo_w[150] == 0 and hi[0] == 0 and hi[-1] == L2 - 1 and lo_w[-1] == L2 - 1
    out, pre, T, _ = R.source_sample(ph, f0, noise, lw[0], lb[0])
    assert np.abs(out - hs_ref[0]).max() < 2e-6  # the oracle's float32 sine, mix and tanh: a few ulp of values <= 1
    uv, namp = R.noise_amp32(f0)
    assert uv[5 * 300] == 0 and namp[5 * 300] == np.float32(np.float32(0.1) / np.float32(3.0)) and namp[0] == np.float32(0.003)


def test_philox_against_sampler_ref():
    seed = 0x1234ABCD5678EF01
    ctr = np.array([0, 1, 77, 2**32 - 1, 2**32, 5 * 2**32 + 9], np.uint64)
    for sub in (0, 1, 2):
        got = R.philox4_vec(seed, ctr, sub)
        for i, c in enumerate(ctr):
            assert got[:, i].tolist() == SR.philox4(seed, int(c), sub)
    r = R.philox4_vec(seed, ctr, 0)
    assert R.unit24(r[0])[2] == SR.device_uniform(seed, 0, 77, 0)
    assert R.unit24(np.array([0xFFFFFFFF], np.uint32))[0] == 1.0 and R.unit24(np.array([0], np.uint32))[0] == np.float32(2.0**-25)
    z, rad = R.source_normals(7, 1, 900, 4000)
    assert z.shape == (4000, 9) and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert R.source_normals(8, 1, 900, 16)[0].tolist() != z[:16].tolist()
