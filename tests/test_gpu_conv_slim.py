"""Epilogue classes of the fused conv kernels (kk_conv_mfma_shared.h KK_EPI_*), THROUGH THE C ABI.

The whole-K and ring forms of variant 4 and the persistent variant 5 exist once per epilogue class that the Kokoro generator launches on
them (residual / scale / final LeakyReLU / statistics / read-and-add stated at compile time, no output activation compiled in) and once
in the generic form that decides all of it at run time.  The arithmetic of a path is the same text in both, so:

  * variant 4 (kk_debug_set_op_variant(4): whole-K / ring with the class the launcher picks) must be torch.equal to the slab-by-slab
    reference form (40), outputs and statistics partials;
  * variant 5 (5) must be torch.equal to the generic instantiation of the same kernel (51).

kk_debug_last_conv_epi() says which instantiation ran; the tables below restate the launchers' choice and are asserted against it.

Shapes (the smallest that reach every path): B = 3 with lengths {1, 193, 400} in 400 rows = three 192-row tiles (an utterance whose
second and third tiles are dead, one that ends one row into its second tile, one with an interior tile and an edge tile); channels
128 -> 128 (two slabs: whole-K, variant 5 with 6 row tasks per period), 256 -> 256 (four slabs and two column blocks: ring / slab by slab,
variant 5 with 3 row tasks per period and its read-and-add kernel), 120 -> 128 (pad channels in the last slab); (taps, dilation)
(3, 1), (7, 3), (11, 1), (11, 5) (both staging chunk counts).  The output buffer of every launch lies between guard rows that must keep
their fill value."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RES, SCALE, POST, STAT, ACC = 1, 2, 4, 8, 16  # KK_EPI_* (kk_conv_mfma_shared.h)
GENERIC = -1
LENS = [1, 193, 400]
L = 400
TILE = 192
GUARD = 4  # rows in front of and behind the output buffer
FILL = 7.0

CHANNELS = [(128, 128), (256, 256), (120, 128)]
TAPS = [(3, 1), (7, 3), (11, 1), (11, 5)]
# (residual, scale, post_slope, statistics, read-and-add): every class a launcher has compiled in, and combinations it has not
EPIS = [
    (False, 1.0, 0.0, True, False),       # first conv of a pair
    (True, 1.0, 0.0, True, False),        # second conv of a pair
    (True, 1.0, 0.0, False, False),       # last conv of a noise resblock
    (True, 1 / 3, 0.0, False, False),     # first term of the mean over the resblocks
    (True, 1 / 3, 0.0, False, True),      # read-and-add to it
    (True, 1 / 3, 0.01, False, True),     # ... with the final LeakyReLU
    (False, 1 / 3, 0.01, True, False),    # not launched by the model: generic
    (False, 1.0, 0.0, False, False),      # not launched by the model: generic
    (True, 1 / 3, 0.01, True, False),     # not launched by the model: generic
]


def _mask(res, scale, post, stat, acc):
    return (RES if res else 0) | (SCALE if scale != 1.0 else 0) | (POST if post not in (0.0, 1.0) else 0) | (STAT if stat else 0) | (ACC if acc else 0)


def expected_v4(CinP, K, d, snake, m):
    """kk_launch_conv_mfma4's choice."""
    halo = (K - 1) * d
    if not snake or halo > 32:
        return GENERIC
    if CinP == 128:  # whole-K, 7 chunks
        return m if m in (STAT, RES | STAT, RES | SCALE, RES | SCALE | ACC, RES | SCALE | ACC | POST) else GENERIC
    if K in (3, 7):  # ring
        return m if m in (STAT, RES | STAT, RES | SCALE) else GENERIC
    return GENERIC  # slab by slab


def expected_v5(K, d, snake, m):
    """kk_launch_conv_mfma5's choice (read-and-add is a template parameter of its own there, not part of the class)."""
    if not snake:
        return GENERIC
    x7 = (K - 1) * d <= 32
    if m & ACC:
        return RES | SCALE if x7 and m == (RES | SCALE | ACC) else GENERIC
    if m == STAT or (x7 and m in (RES | STAT, RES)):
        return m
    return GENERIC


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


class _Operands:
    """Device operands of one (channels, taps) shape, shared by every launch of it."""

    def __init__(self, lib, Cin, Cout, K, d):
        rng = np.random.default_rng(zlib.crc32(f"slim-{Cin}-{Cout}-{K}-{d}".encode()))
        self.Cin, self.Cout, self.K, self.d = Cin, Cout, K, d
        self.B = B = len(LENS)
        self.pad = (K - 1) * d // 2
        self.CinP = CinP = (Cin + 127) // 128 * 128
        self.CoutP = CoutP = (Cout + 127) // 128 * 128
        x = rng.standard_normal((B, L, Cin)).astype(np.float32) * 2.0 + 0.5
        for b, n in enumerate(LENS):
            x[b, n:] = 0  # rows past an utterance hold zeros in the model
        xp = np.full((B, L, CinP), 5.0, np.float32)  # pad channels may hold anything: the kernel masks them
        xp[:, :, :Cin] = x
        wp = np.zeros((K, CoutP, CinP), np.float32)
        wp[:, :Cout, :Cin] = rng.standard_normal((K, Cout, Cin)) / math.sqrt(K * Cin)
        bp = np.zeros(CoutP, np.float32)
        bp[:Cout] = rng.standard_normal(Cout)
        A, Bv = np.zeros((B, CinP), np.float32), np.zeros((B, CinP), np.float32)
        A[:, :Cin] = rng.standard_normal((B, Cin)) * 0.5 + 1
        Bv[:, :Cin] = rng.standard_normal((B, Cin)) * 0.3
        self.xd, self.wd, self.bd = dev(xp, torch.bfloat16), dev(wp, torch.bfloat16), dev(bp)
        self.ad, self.bvd, self.ald = dev(A), dev(Bv), dev(rng.uniform(0.5, 1.5, Cin).astype(np.float32))
        self.rd = dev(rng.standard_normal((B, L, Cout)), torch.bfloat16)
        self.init = dev(rng.standard_normal((B, L, Cout)), torch.bfloat16)  # what a read-and-add launch finds in the output rows
        self.lend = dev(np.asarray(LENS, np.int32), torch.int32)
        self.wf = torch.empty_like(self.wd)
        assert lib.kk_op_pack_w_frag(stream(), P(self.wd), P(self.wf), K, CoutP, CinP) == 0, lib.kk_last_error()
        self.ntiles = (L + TILE - 1) // TILE

    def _buffer(self, acc):
        """[GUARD + B * L + GUARD][Cout] bf16; the launch sees the middle."""
        buf = torch.full((GUARD + self.B * L + GUARD, self.Cout), FILL, device="cuda", dtype=torch.bfloat16)
        out = buf[GUARD:GUARD + self.B * L].view(self.B, L, self.Cout)
        if acc:
            out.copy_(self.init)
        return buf, out

    def _check_guards(self, buf, what):
        assert torch.all(buf[:GUARD] == FILL) and torch.all(buf[-GUARD:] == FILL), what

    def fused(self, lib, variant, snake, epi):
        """One fused launch: (output, statistics partials or None, class of the instantiation that ran)."""
        from mlx_audio_amd import _lib

        res, scale, post, stat, acc = epi
        buf, out = self._buffer(acc)
        part = torch.full((self.B, self.ntiles, 2, self.Cout), -1.0, device="cuda") if stat else None
        lib.kk_debug_set_op_wfrag(P(self.wf))
        lib.kk_debug_set_op_variant(variant)
        lib.kk_debug_set_op_post_slope(post)
        lib.kk_debug_set_op_accumulate(int(acc))
        try:
            nt = C.c_int(0)
            rc = lib.kk_op_conv1d_bf16_fused(stream(), self.B, P(self.xd), self.CinP, L, P(self.lend), P(self.wd), self.CinP, self.CoutP, P(self.bd),
                                             self.Cin, self.Cout, self.K, self.pad, self.d, P(self.ad), P(self.bvd), self.CinP,
                                             _lib.ACT_SNAKE if snake else _lib.ACT_LRELU, 0.1, P(self.ald), P(self.rd) if res else None, self.Cout,
                                             scale, P(out), self.Cout, P(part), C.byref(nt))
            assert rc == 0, lib.kk_last_error()
            chosen = lib.kk_debug_last_conv_epi()
            torch.cuda.synchronize()
        finally:
            lib.kk_debug_set_op_wfrag(None)
            lib.kk_debug_set_op_variant(4)
            lib.kk_debug_set_op_post_slope(0.0)
            lib.kk_debug_set_op_accumulate(0)
        self._check_guards(buf, (variant, snake, epi))
        return out, part, chosen

    def plain(self, lib, variant, act):
        """One launch on the raw input with an output activation: (output, class of the instantiation that ran)."""
        from mlx_audio_amd import _lib

        buf, out = self._buffer(False)
        lib.kk_debug_set_op_wfrag(P(self.wf))
        lib.kk_debug_set_op_variant(variant)
        try:
            rc = lib.kk_op_conv1d_bf16(stream(), self.B, P(self.xd), self.CinP, L, P(self.lend), P(self.wd), self.CinP, self.CoutP, P(self.bd), self.Cout,
                                       self.K, 0, 1, self.pad, self.d, 0, 1.0, act, 0.0, P(self.rd), self.Cout, 1.0, 0, P(out), self.Cout, L,
                                       P(self.lend), _lib.KK_BF16)
            assert rc == 0, lib.kk_last_error()
            chosen = lib.kk_debug_last_conv_epi()
            torch.cuda.synchronize()
        finally:
            lib.kk_debug_set_op_wfrag(None)
            lib.kk_debug_set_op_variant(4)
        self._check_guards(buf, (variant, act))
        return out, chosen


def _v5_takes(CinP, acc):
    return not (acc and CinP < 256)  # kk_mfma5_eligible: read-and-add needs four slabs


@pytest.mark.parametrize("K,d", TAPS, ids=[f"k{k}d{d}" for k, d in TAPS])
@pytest.mark.parametrize("Cin,Cout", CHANNELS, ids=[f"{a}to{b}" for a, b in CHANNELS])
def test_epilogue_classes_bit_identical(lib, Cin, Cout, K, d):
    op = _Operands(lib, Cin, Cout, K, d)
    picked4, picked5 = set(), set()
    for snake in (True, False):
        for epi in EPIS:
            m = _mask(*epi)
            what = (Cin, Cout, K, d, snake, epi)
            # variant 4: the routed form with the launcher's class against the slab-by-slab reference form
            ref, ref_part, c_ref = op.fused(lib, 40, snake, epi)
            out, part, c4 = op.fused(lib, 4, snake, epi)
            assert c_ref == GENERIC, what
            assert c4 == expected_v4(op.CinP, K, d, snake, m), what
            picked4.add(c4)
            assert torch.equal(out, ref), what
            if part is not None:
                assert torch.equal(part, ref_part), what
            assert not torch.isnan(out.float()).any(), what
            # rows past an utterance are exact zeros in a launch that does not add to what was there
            if not epi[4]:
                for b, n in enumerate(LENS):
                    assert torch.all(out[b, n:] == 0), what
            # variant 5: the launcher's class against the generic instantiation of the same kernel
            if _v5_takes(op.CinP, epi[4]):
                ref5, ref5_part, c_ref5 = op.fused(lib, 51, snake, epi)
                out5, part5, c5 = op.fused(lib, 5, snake, epi)
                assert c_ref5 == GENERIC, what
                assert c5 == expected_v5(K, d, snake, m), what
                picked5.add(c5)
                assert torch.equal(out5, ref5), what
                if part5 is not None:
                    assert torch.equal(part5, ref5_part), what
    # the shape reached compiled-in classes where its kernels have them (the test would otherwise compare the generic form with itself)
    assert len(picked5 - {GENERIC}) >= 1, picked5
    if (K - 1) * d <= 32 and (op.CinP == 128 or K in (3, 7)):
        assert len(picked4 - {GENERIC}) >= 3, picked4


@pytest.mark.parametrize("K,d,variant,ref_variant", [(3, 1, 4, 40), (11, 1, 5, 51)], ids=["wholek", "variant5"])
def test_gelu_epilogue_runs_the_generic_instantiation(lib, K, d, variant, ref_variant):
    from mlx_audio_amd import _lib

    op = _Operands(lib, 128, 128, K, d)
    ref, c_ref = op.plain(lib, ref_variant, _lib.ACT_GELU)
    out, chosen = op.plain(lib, variant, _lib.ACT_GELU)
    assert chosen == GENERIC and c_ref == GENERIC
    assert torch.equal(out, ref)
    # the activation did run: exact GELU of (conv + bias) + residual differs from the same launch without it
    lin, _ = op.plain(lib, variant, _lib.ACT_NONE)
    assert not torch.equal(out, lin)
