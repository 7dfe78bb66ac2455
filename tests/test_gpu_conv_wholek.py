"""Whole-K form of conv variant 4 (kk_conv_mfma4.hip: stride 1, 128 padded input channels -- both 64-channel slabs staged in the
prologue, nothing but MFMAs in the main loop) against the slab-by-slab form of the same kernel, THROUGH THE C ABI.

The two forms feed the same matrix instruction the same operands in the same K order and share the epilogue, so every case runs once
with the reference switch on (kk_debug_set_op_variant(40): slab by slab) and once off (4: whole-K where eligible) and the outputs AND
the statistics partials must be torch.equal.  Each case is also compared with torch on the same bf16 operands, at the bars
tests/test_gpu_kernels.py uses for the same quantities (quoted next to each assertion).  The 11-tap fused cases run on variant 5 as
well (its staging chunk count follows the same halo rule), against the same torch reference.

Shapes: B = 3 ragged (full length, shorter than a tile, ending inside a tile), L in {193, 385} (one / two full 192-row tiles plus a
one-row tile), Cin in {128, 120, 72} (pad channels in slab 1, slab 1 almost all padding), Cout in {128, 136} (one / two column blocks,
pad columns), (taps, dilation) with halos 2 / 10 / 18 / 30 / 10 / 50 (both chunk-count classes, 30 next to the boundary at 32),
symmetric and causal padding."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import err_stats, report

pytestmark = pytest.mark.gpu

TAPS = [(3, 1), (3, 5), (7, 3), (7, 5), (11, 1), (11, 5)]
MODES = ["plain", "plain_epi", "snake_stats", "lrelu_stats_res"]
TILE = 192


def _cases():
    """Every (taps, dilation) x mode once (24 cases); Cin / Cout / L / padding dealt from shuffled decks so that each value meets each mode
    and each tap class (literal seed)."""
    rng = np.random.default_rng(20250611)
    n = len(TAPS) * len(MODES)

    def deck(vals):
        d = []
        while len(d) < n:
            d += [vals[i] for i in rng.permutation(len(vals))]
        return d[:n]

    cins, couts, lens, causal = deck([128, 120, 72]), deck([128, 136]), deck([193, 385]), deck([False, True])
    out = []
    for i, ((k, d), mode) in enumerate((t, m) for t in TAPS for m in MODES):
        out.append((f"k{k}d{d}-{mode}-cin{cins[i]}-cout{couts[i]}-L{lens[i]}-{'causal' if causal[i] else 'sym'}", k, d, mode, cins[i], couts[i], lens[i], causal[i]))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf(a):
    return torch.tensor(a).to(torch.bfloat16).float().numpy()


class _Case:
    """Operands of one case on the host (bf16-rounded fp32) and on the device, and its torch reference."""

    def __init__(self, name, K, d, mode, Cin, Cout, L, causal):
        from mlx_audio_amd import _lib

        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.name, self.K, self.d, self.mode, self.Cin, self.Cout, self.L = name, K, d, mode, Cin, Cout, L
        self.B = B = 3
        halo = (K - 1) * d
        self.pad = halo if causal else halo // 2
        # full length (ends one row into the last tile) / shorter than a tile / ends inside a tile
        self.lens = [L, int(rng.integers(1, TILE)), int(rng.integers(100, TILE + 1)) if L == 193 else int(rng.integers(TILE + 1, 2 * TILE))]
        self.fused = mode in ("snake_stats", "lrelu_stats_res")
        CinP, CoutP = 128, (Cout + 127) // 128 * 128
        self.CinP, self.CoutP = CinP, CoutP
        x = _bf((rng.standard_normal((B, L, Cin)) * (2.0 if self.fused else 1.0) + (0.5 if self.fused else 0.0)).astype(np.float32))
        for b, n in enumerate(self.lens):
            x[b, n:] = 0  # rows past an utterance hold zeros in the model
        self.x = x
        xp = np.full((B, L, CinP), 5.0, np.float32)  # pad channels may hold anything: the kernel masks them
        xp[:, :, :Cin] = x
        self.w = w = _bf((rng.standard_normal((Cout, K, Cin)) / math.sqrt(K * Cin)).astype(np.float32))
        wp = np.zeros((K, CoutP, CinP), np.float32)
        wp[:, :Cout, :Cin] = np.transpose(w, (1, 0, 2))
        self.bias = bias = rng.standard_normal(Cout).astype(np.float32)
        bp = np.zeros(CoutP, np.float32)
        bp[:Cout] = bias
        self.res = _bf(rng.standard_normal((B, L, Cout)).astype(np.float32)) if mode != "plain" and mode != "snake_stats" else None
        self.init = _bf(rng.standard_normal((B, L, Cout)).astype(np.float32)) if mode == "plain_epi" else None
        self.A = np.zeros((B, CinP), np.float32)
        self.Bv = np.zeros((B, CinP), np.float32)
        self.A[:, :Cin] = rng.standard_normal((B, Cin)) * 0.5 + 1
        self.Bv[:, :Cin] = rng.standard_normal((B, Cin)) * 0.3
        self.alpha = rng.uniform(0.5, 1.5, Cin).astype(np.float32)
        self.slope = 0.1
        self.xd, self.wd, self.bd = dev(xp, torch.bfloat16), dev(wp, torch.bfloat16), dev(bp)
        self.rd = dev(self.res, torch.bfloat16) if self.res is not None else None
        self.ad, self.bvd, self.ald = dev(self.A), dev(self.Bv), dev(self.alpha)
        self.lend = dev(np.asarray(self.lens, np.int32), torch.int32)
        self.ntiles = (L + TILE - 1) // TILE
        self.nrm_act = _lib.ACT_SNAKE if mode == "snake_stats" else _lib.ACT_LRELU
        self.KK_BF16 = _lib.KK_BF16
        self.ref = self._reference()  # computed once, shared by every run of the case

    def _reference(self):
        ref = []
        K, d, pad = self.K, self.d, self.pad
        wt, bt = torch.tensor(self.w).permute(0, 2, 1), torch.tensor(self.bias)
        for b, n in enumerate(self.lens):
            xi = self.x[b, :n]
            if self.fused:
                y = xi * self.A[b, : self.Cin][None, :] + self.Bv[b, : self.Cin][None, :]
                if self.mode == "snake_stats":
                    y = y + (1.0 / self.alpha)[None, :] * np.sin(self.alpha[None, :] * y) ** 2
                else:
                    y = np.where(y > 0, y, y * np.float32(self.slope))
                xi = _bf(y.astype(np.float32))  # the kernel rounds the transformed input to bf16
            xpad = F.pad(torch.tensor(xi)[None].transpose(1, 2), (pad, (K - 1) * d - pad))
            r = F.conv1d(xpad, wt, bt, 1, 0, d).transpose(1, 2)[0]
            if self.mode == "plain_epi":
                r = (r + torch.tensor(self.res[b, :n])) * (1 / 3) + torch.tensor(self.init[b, :n])
                r = F.leaky_relu(r, 0.01)
            elif self.res is not None:
                r = r + torch.tensor(self.res[b, :n])
            ref.append(r.numpy())
        return ref

    def run(self, lib, variant):
        """One launch with kk_debug_set_op_variant(variant): (output [B][L][Cout] bf16, statistics partials or None), on the device."""
        B, L, Cout = self.B, self.L, self.Cout
        out = dev(self.init, torch.bfloat16) if self.init is not None else torch.full((B, L, Cout), 7.0, device="cuda", dtype=torch.bfloat16)
        part = torch.full((B, self.ntiles, 2, Cout), -1.0, device="cuda") if self.fused else None
        wf = torch.empty_like(self.wd)
        assert lib.kk_op_pack_w_frag(stream(), P(self.wd), P(wf), self.K, self.CoutP, self.CinP) == 0, lib.kk_last_error()
        lib.kk_debug_set_op_wfrag(P(wf))
        lib.kk_debug_set_op_variant(variant)
        lib.kk_debug_set_op_post_slope(0.01 if self.mode == "plain_epi" else 0.0)
        try:
            if self.fused:
                nt = C.c_int(0)
                rc = lib.kk_op_conv1d_bf16_fused(stream(), B, P(self.xd), self.CinP, L, P(self.lend), P(self.wd), self.CinP, self.CoutP, P(self.bd),
                                                 self.Cin, Cout, self.K, self.pad, self.d, P(self.ad), P(self.bvd), self.CinP, self.nrm_act,
                                                 self.slope, P(self.ald), P(self.rd), Cout, 1.0, P(out), Cout, P(part), C.byref(nt))
                assert rc == 0, lib.kk_last_error()
                assert nt.value == self.ntiles
            else:
                epi = self.mode == "plain_epi"
                rc = lib.kk_op_conv1d_bf16(stream(), B, P(self.xd), self.CinP, L, P(self.lend), P(self.wd), self.CinP, self.CoutP, P(self.bd), Cout,
                                           self.K, 0, 1, self.pad, self.d, 0, 1.0, 0, 0.0, P(self.rd), Cout, 1 / 3 if epi else 1.0, int(epi),
                                           P(out), Cout, L, P(self.lend), self.KK_BF16)
                assert rc == 0, lib.kk_last_error()
            torch.cuda.synchronize()
        finally:
            lib.kk_debug_set_op_wfrag(None)
            lib.kk_debug_set_op_variant(4)
            lib.kk_debug_set_op_post_slope(0.0)
        return out, part

    def check_against_torch(self, tag, out, part):
        got = out.float().cpu().numpy()
        pt = part.cpu().numpy() if part is not None else None
        for b, n in enumerate(self.lens):
            ref = self.ref[b]
            e = err_stats(got[b, :n], ref)
            report(f"conv_wholek/{tag}/{self.name}/b{b}", **e)
            if self.fused:
                assert e["rel_max"] < 1.5e-2, (self.name, b, e)  # test_conv_mfma_fused_adain_snake_and_stats: bf16 rounding of the transformed input and of the output
            elif self.mode == "plain_epi":
                assert e["rel_max"] < 6e-3, (self.name, b, e)  # test_conv_mfma_epilogue_and_ragged
            else:
                assert e["rel_max"] < 5e-3, (self.name, b, e)  # test_conv_mfma_bf16: one bf16 rounding of the result
            assert np.all(got[b, n:] == 0), (self.name, b)
            if pt is not None:
                # column statistics of the fp32 values before the bf16 rounding: the fp32 reference's sums up to summation order (same test)
                s1, s2 = pt[b, :, 0].sum(0), pt[b, :, 1].sum(0)
                np.testing.assert_allclose(s1, ref.astype(np.float64).sum(0), rtol=1e-3, atol=2e-2)
                np.testing.assert_allclose(s2, (ref.astype(np.float64) ** 2).sum(0), rtol=1e-3)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_wholek_bit_identical_to_slabwise(lib, case):
    c = _Case(*case)
    ref_out, ref_part = c.run(lib, 40)  # reference switch on: slab by slab
    out, part = c.run(lib, 4)           # off: the whole-K form
    c.check_against_torch("slabwise", ref_out, ref_part)
    c.check_against_torch("wholek", out, part)
    assert torch.equal(out, ref_out), c.name
    if c.fused:
        assert torch.equal(part, ref_part), c.name
    if c.fused and c.K == 11:  # variant 5's service role stages with the same chunk-count rule
        out5, part5 = c.run(lib, 5)
        c.check_against_torch("variant5", out5, part5)
