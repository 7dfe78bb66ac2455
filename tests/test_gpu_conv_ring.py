"""Ring form of conv variant 4 (kk_conv_mfma4.hip: three or more 64-channel slabs, halo <= 32 rows -- two LDS slab buffers, the next slab
stored behind the last tap of the current one, ONE barrier per slab) against the slab-by-slab form of the same kernel, THROUGH THE C ABI.
The launcher routes the form per measured layer class: plain inputs with one tap, fused AdaIN + Snake inputs with 3 or 7 taps.  Those
classes are crossed with every channel entry below; the other cases ("pin-...") take the slab-by-slab form either way and pin that the
routing leaves them alone.  The last test runs the whole model with the form switched off (debug bit 11) and on.

The two forms feed the same matrix instruction the same operands in the same K order and share the epilogue, so every case runs once
with the reference switch on (kk_debug_set_op_variant(40): slab by slab) and once off (4: the ring form where eligible) and the outputs AND
the statistics partials must be torch.equal.  Each run is also compared with torch on the same bf16 operands, at the bars
tests/test_gpu_conv_wholek.py quotes for the same quantities (next to each assertion).

Shapes: B = 3 ragged (full length, shorter than a tile, ending inside a tile), L in {193, 385}; (padded, real) input channels (192, 192),
(256, 250), (192, 130), (320, 320): three, four and five slabs (the loop ends in either buffer), no pad channels, pad channels, a last slab
that is nearly all padding; Cout in {128, 136}; (taps, dilation) with halos 0 / 2 / 10 / 4 / 18 / 30 (30 next to the limit of 32);
symmetric and causal padding; the four modes of the whole-K test.  The fused Snake input needs a real channel count that is a multiple of
4 (the launcher refuses others), so the Snake cases take 252 / 132 where the deck deals 250 / 130: still pad channels, still a last slab that is nearly all padding.  One 11-tap
case at dilation 5 (halo 50) is not eligible and must take the reference form, and still be equal.  (The polyphase transposed form is
not routed to the ring form, so it has no cases here.)"""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import err_stats, report

pytestmark = pytest.mark.gpu

TAPS = [(1, 1), (3, 1), (3, 5), (5, 1), (7, 3), (7, 5)]
MODES = ["plain", "plain_epi", "snake_stats", "lrelu_stats_res"]
CHANNELS = [(192, 192), (256, 250), (192, 130), (320, 320)]  # (padded, real)
TILE = 192


def routed(k, mode):
    """The launcher's rule (kk_launch_conv_mfma4) for the shapes of this file (CinP >= 192, halo <= 32 but for the 11-tap case)."""
    fused = mode in ("snake_stats", "lrelu_stats_res")
    return (k == 1 and not fused) or (k in (3, 7) and mode == "snake_stats")


def _cases():
    """ROUTED classes -- one tap x the two plain modes (ring<0, 6>), (3, 1) / (3, 5) / (7, 3) / (7, 5) x the Snake mode (ring<1, 7>) --
    crossed with ALL FOUR channel entries, so that both instantiations meet 3, 4 and 5 slabs, pad channels and a last slab
    that is nearly all padding (24 cases).  The rest of the (taps, dilation) x mode grid (18 cases) and the 11-tap case take the slab-by-slab
    form under both switches: routing pins, channels dealt from a shuffled deck.  Cout / L / padding are dealt from shuffled decks over all
    cases (literal seed)."""
    rng = np.random.default_rng(20250712)
    grid = [(t, m) for t in TAPS for m in MODES]
    combos = [(t, m, ch) for (t, m) in grid if routed(t[0], m) for ch in CHANNELS]
    pins = [(t, m) for (t, m) in grid if not routed(t[0], m)]
    n = len(combos) + len(pins)

    def deck(vals, n):
        d = []
        while len(d) < n:
            d += [vals[i] for i in rng.permutation(len(vals))]
        return d[:n]

    couts, lens, causal, pin_ch = deck([128, 136], n), deck([193, 385], n), deck([False, True], n), deck(CHANNELS, len(pins))
    combos += [(t, m, pin_ch[i]) for i, (t, m) in enumerate(pins)]
    out = []
    for i, ((k, d), mode, (cinp, cin)) in enumerate(combos):
        if mode == "snake_stats" and cin % 4:
            cin += 2  # 250 -> 252, 130 -> 132
        tag = "ring" if routed(k, mode) else "pin"
        out.append((f"{tag}-k{k}d{d}-{mode}-cin{cin}in{cinp}-cout{couts[i]}-L{lens[i]}-{'causal' if causal[i] else 'sym'}", k, d, mode, cinp, cin, couts[i],
                    lens[i], causal[i]))
    out.append(("pin-k11d5-lrelu_stats_res-cin250in256-cout136-L385-sym", 11, 5, "lrelu_stats_res", 256, 250, 136, 385, False))
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
    """Operands of one case on the host (bf16-rounded fp32) and on the device, and its torch reference.  stride > 0: the transposed form
    (kernel K, padding (K - stride) / 2, L input rows, L * stride output rows)."""

    def __init__(self, name, K, d, mode, CinP, Cin, Cout, L, causal=False, stride=0):
        from mlx_audio_amd import _lib

        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.name, self.K, self.d, self.mode, self.Cin, self.Cout, self.L, self.stride = name, K, d, mode, Cin, Cout, L, stride
        self.B = B = 3
        self.up = up = stride if stride else 1
        self.Lo = Lo = L * up
        halo = (K - 1) * d
        self.pad = (K - stride) // 2 if stride else (halo if causal else halo // 2)
        # full length (ends one row into the last tile) / shorter than a tile / ends inside a tile (a transposed tile is 192 INPUT rows per phase)
        self.lens = [L, int(rng.integers(1, TILE)), int(rng.integers(100, TILE + 1)) if L == 193 else int(rng.integers(TILE + 1, 2 * TILE))]
        self.lens_out = [n * up for n in self.lens]
        self.fused = mode in ("snake_stats", "lrelu_stats_res")
        CoutP = (Cout + 127) // 128 * 128
        self.CinP, self.CoutP = CinP, CoutP
        x = _bf((rng.standard_normal((B, L, Cin)) * (2.0 if self.fused else 1.0) + (0.5 if self.fused else 0.0)).astype(np.float32))
        for b, n in enumerate(self.lens):
            x[b, n:] = 0  # rows past an utterance hold zeros in the model
        self.x = x
        xp = np.full((B, L, CinP), 5.0, np.float32)  # pad channels may hold anything: the kernel masks them, or meets zero weights
        xp[:, :, :Cin] = x
        self.w = w = _bf((rng.standard_normal((Cout, K, Cin)) / math.sqrt(K * Cin / up)).astype(np.float32))
        wp = np.zeros((K, CoutP, CinP), np.float32)
        wp[:, :Cout, :Cin] = np.transpose(w, (1, 0, 2))
        self.bias = bias = rng.standard_normal(Cout).astype(np.float32)
        bp = np.zeros(CoutP, np.float32)
        bp[:Cout] = bias
        self.res = _bf(rng.standard_normal((B, Lo, Cout)).astype(np.float32)) if mode != "plain" and mode != "snake_stats" else None
        self.init = _bf(rng.standard_normal((B, Lo, Cout)).astype(np.float32)) if mode == "plain_epi" else None
        self.A = np.zeros((B, CinP), np.float32)
        self.Bv = np.zeros((B, CinP), np.float32)
        self.A[:, :Cin] = rng.standard_normal((B, Cin)) * 0.5 + 1
        self.Bv[:, :Cin] = rng.standard_normal((B, Cin)) * 0.3
        self.alpha = rng.uniform(0.5, 1.5, Cin).astype(np.float32)
        self.slope = 0.1
        self.xd, self.wd, self.bd = dev(xp, torch.bfloat16), dev(wp, torch.bfloat16), dev(bp)
        self.rd = dev(self.res, torch.bfloat16) if self.res is not None else None
        self.ad, self.bvd, self.ald = dev(self.A), dev(self.Bv), dev(self.alpha)
        self.lind = dev(np.asarray(self.lens, np.int32), torch.int32)
        self.loutd = dev(np.asarray(self.lens_out, np.int32), torch.int32)
        self.ntiles = (L + TILE - 1) // TILE
        self.nrm_act = _lib.ACT_SNAKE if mode == "snake_stats" else _lib.ACT_LRELU
        self.KK_BF16 = _lib.KK_BF16
        self.ref = self._reference()  # computed once, shared by every run of the case

    def _reference(self):
        ref = []
        K, d, pad = self.K, self.d, self.pad
        wt, bt = torch.tensor(self.w).permute(0, 2, 1), torch.tensor(self.bias)  # [Cout][Cin][K]
        for b, n in enumerate(self.lens):
            xi = self.x[b, :n]
            if self.fused:
                y = xi * self.A[b, : self.Cin][None, :] + self.Bv[b, : self.Cin][None, :]
                if self.mode == "snake_stats":
                    y = y + (1.0 / self.alpha)[None, :] * np.sin(self.alpha[None, :] * y) ** 2
                else:
                    y = np.where(y > 0, y, y * np.float32(self.slope))
                xi = _bf(y.astype(np.float32))  # the kernel rounds the transformed input to bf16
            if self.stride:
                r = F.conv_transpose1d(torch.tensor(xi)[None].transpose(1, 2), wt.transpose(0, 1).contiguous(), bt, self.stride, pad).transpose(1, 2)[0]
            else:
                xpad = F.pad(torch.tensor(xi)[None].transpose(1, 2), (pad, (K - 1) * d - pad))
                r = F.conv1d(xpad, wt, bt, 1, 0, d).transpose(1, 2)[0]
            no = n * self.up
            if self.mode == "plain_epi":
                r = (r + torch.tensor(self.res[b, :no])) * (1 / 3) + torch.tensor(self.init[b, :no])
                r = F.leaky_relu(r, 0.01)
            elif self.res is not None:
                r = r + torch.tensor(self.res[b, :no])
            ref.append(r.numpy())
        return ref

    def run(self, lib, variant):
        """One launch with kk_debug_set_op_variant(variant): (output [B][Lo][Cout] bf16, statistics partials or None), on the device."""
        B, L, Lo, Cout = self.B, self.L, self.Lo, self.Cout
        out = dev(self.init, torch.bfloat16) if self.init is not None else torch.full((B, Lo, Cout), 7.0, device="cuda", dtype=torch.bfloat16)
        part = torch.full((B, self.ntiles, 2, Cout), -1.0, device="cuda") if self.fused else None
        wf = torch.empty_like(self.wd)
        assert lib.kk_op_pack_w_frag(stream(), P(self.wd), P(wf), self.K, self.CoutP, self.CinP) == 0, lib.kk_last_error()
        lib.kk_debug_set_op_wfrag(P(wf))
        lib.kk_debug_set_op_variant(variant)
        lib.kk_debug_set_op_post_slope(0.01 if self.mode == "plain_epi" else 0.0)
        try:
            if self.fused:
                nt = C.c_int(0)
                rc = lib.kk_op_conv1d_bf16_fused(stream(), B, P(self.xd), self.CinP, L, P(self.lind), P(self.wd), self.CinP, self.CoutP, P(self.bd),
                                                 self.Cin, Cout, self.K, self.pad, self.d, P(self.ad), P(self.bvd), self.CinP, self.nrm_act,
                                                 self.slope, P(self.ald), P(self.rd), Cout, 1.0, P(out), Cout, P(part), C.byref(nt))
                assert rc == 0, lib.kk_last_error()
                assert nt.value == self.ntiles
            else:
                epi = self.mode == "plain_epi"
                rc = lib.kk_op_conv1d_bf16(stream(), B, P(self.xd), self.CinP, L, P(self.lind), P(self.wd), self.CinP, self.CoutP, P(self.bd), Cout,
                                           self.K, 1 if self.stride else 0, self.stride or 1, self.pad, self.d, 0, 1.0, 0, 0.0, P(self.rd), Cout,
                                           1 / 3 if epi else 1.0, int(epi), P(out), Cout, Lo, P(self.loutd), self.KK_BF16)
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
        for b, n in enumerate(self.lens_out):
            ref = self.ref[b]
            e = err_stats(got[b, :n], ref)
            report(f"conv_ring/{tag}/{self.name}/b{b}", **e)
            if self.fused:
                assert e["rel_max"] < 1.5e-2, (self.name, b, e)  # test_conv_mfma_fused_adain_snake_and_stats: bf16 rounding of the transformed input and of the output
            elif self.mode == "plain_epi" or self.stride:
                assert e["rel_max"] < 6e-3, (self.name, b, e)  # test_conv_mfma_epilogue_and_ragged, test_conv_mfma_transposed_and_fused
            else:
                assert e["rel_max"] < 5e-3, (self.name, b, e)  # test_conv_mfma_bf16: one bf16 rounding of the result
            assert np.all(got[b, n:] == 0), (self.name, b)
            if pt is not None:
                # column statistics of the fp32 values before the bf16 rounding: the fp32 reference's sums up to summation order (same test)
                s1, s2 = pt[b, :, 0].sum(0), pt[b, :, 1].sum(0)
                np.testing.assert_allclose(s1, ref.astype(np.float64).sum(0), rtol=1e-3, atol=2e-2)
                np.testing.assert_allclose(s2, (ref.astype(np.float64) ** 2).sum(0), rtol=1e-3)


def _both_forms(lib, c):
    ref_out, ref_part = c.run(lib, 40)  # reference switch on: slab by slab
    out, part = c.run(lib, 4)           # off: the ring form where eligible
    c.check_against_torch("slabwise", ref_out, ref_part)
    c.check_against_torch("ring", out, part)
    assert torch.equal(out, ref_out), c.name
    if c.fused:
        assert torch.equal(part, ref_part), c.name


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ring_bit_identical_to_slabwise(lib, case):
    _both_forms(lib, _Case(*case))


def test_model_with_ring_form_equals_slab_by_slab_bitexact():
    """The whole bf16 forward with variant 4 slab by slab everywhere (kk_debug_force_generic bit 11) and as routed: waveform, durations and
    frame counts torch.equal.  9 utterances x 122 token rows = 1098 rows, past the 1024 up to which the Linears take the streaming kernel,
    so Albert's Linears run ring<0, 6> (12 and 32 slabs); the 3-tap Snake layers of stage 0 run ring<1, 7>."""
    import os

    import mlx_audio_amd.params as P
    from mlx_audio_amd import _lib
    from mlx_audio_amd.engine import KokoroEngine

    cfg = P.kokoro_config()
    eng = KokoroEngine(cfg, P.synth_checkpoint(cfg, 0), compute_dtype="bfloat16")
    rng = np.random.default_rng(20250713)
    utts = [rng.integers(1, 178, 120).tolist() for _ in range(9)]
    pack = np.load(os.path.join(os.path.dirname(__file__), "golden", "af_heart_rows.npz"))["rows"]
    ref_s = pack[rng.integers(0, pack.shape[0], len(utts))].astype(np.float32)
    dev_ = eng.device
    ids, lens, Tmax = eng.pack_ids(utts)
    durs = np.zeros((len(utts), Tmax), np.int32)
    for b, u in enumerate(utts):
        durs[b, : len(u) + 2] = 1 + (np.arange(len(u) + 2) + b) % 2
    Fmax = int(durs.sum(1).max())
    res = {}
    try:
        for flag in (2048, 0):
            eng.lib.kk_debug_force_generic(eng._h, flag)
            wav, pred, nfr = eng.forward(ids, lens, torch.tensor(ref_s, device=dev_), torch.ones(len(utts), device=dev_), Fmax,
                                         forced_dur=torch.tensor(durs, device=dev_), noise_mode=_lib.NOISE_ZERO)
            torch.cuda.synchronize()
            assert torch.isfinite(wav).all()
            res[flag] = (wav.clone(), pred.clone(), nfr.clone())
    finally:
        eng.lib.kk_debug_force_generic(eng._h, 0)
    for a, b in zip(res[0], res[2048]):
        assert torch.equal(a, b)
