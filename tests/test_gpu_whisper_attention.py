"""The long-sequence attention kernel (kk_op_attention_long, csrc/kk_whisper.hip) against float64 softmax(q k^T / 8) v on the
identical bf16 operands, through the C ABI.

Bound, derived: |out - ref| <= 2^-7 max|v| per (item, head).  The probabilities enter the second matrix product rounded to bf16 (2^-9 each,
weights summing to 1), the normaliser is taken before that rounding (2^-9), the output is rounded to bf16 (2^-9), and one more 2^-9 is spare.
q is scaled so that the scores reach +-8: the running maximum then moves across key tiles and the accumulators are rescaled."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import _whisper_ref as R  # noqa: E402

from mlx_audio_amd import _lib  # noqa: E402
from mlx_audio_amd._lib import KokoroHipError  # noqa: E402

pytestmark = pytest.mark.gpu


def _qkv(B, T, heads, seed):
    """bf16-exact float32 [B][T][3 * heads * 64], q scaled per (item, head) so that max |q k / 8| is 8"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, 3, heads, 64)).astype(np.float32)
    for b in range(B):
        for h in range(heads):
            s = x[b, :, 0, h].astype(np.float64) @ x[b, :, 1, h].astype(np.float64).T / 8.0
            x[b, :, 0, h] *= 8.0 / np.abs(s).max()
    return R.bf16_round(x.reshape(B, T, 3 * heads * 64))


def _run(x, T, heads, out=None, ld_claim=None):
    """x float32 [B][T_rows][ld] (bf16-exact) -> bf16 device out [B][T_rows][heads * 64]"""
    lib = _lib.load()
    B, T_rows, ld = x.shape
    xd = torch.from_numpy(x).cuda().to(torch.bfloat16).contiguous()
    if out is None:
        out = torch.zeros((B, T_rows, heads * 64), dtype=torch.bfloat16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.kk_op_attention_long(st, B, C.c_void_p(xd.data_ptr()), ld if ld_claim is None else ld_claim, T_rows, T, heads,
                                        C.c_void_p(out.data_ptr()), heads * 64), "kk_op_attention_long")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 63, 64, 65, 127, 129, 1500])
def test_against_float64(T, heads):
    B = 2
    x = _qkv(B, T, heads, 1000 * heads + T)
    got = _run(x, T, heads).float().cpu().numpy()
    worst = 0.0
    for b in range(B):
        for h in range(heads):
            q, k, v = (x[b, :, (i * heads + h) * 64 : (i * heads + h + 1) * 64] for i in range(3))
            ref = R.attention(q, k, v)
            err = float(np.abs(got[b, :, h * 64 : (h + 1) * 64] - ref).max())
            bound = 2.0 ** -7 * float(np.abs(v).max())
            worst = max(worst, err / bound)
            assert err <= bound, (b, h, err, bound)
    print(f"T {T} heads {heads}: max error / bound = {worst:.3f}")


@pytest.mark.parametrize("T", [65, 129])
def test_garbage_rows_are_neither_read_nor_written(T):
    heads, B = 3, 2
    x = np.concatenate([_qkv(B, T, heads, 77 + T), np.full((B, 5, 3 * heads * 64), np.nan, np.float32)], axis=1)
    out = torch.full((B, T + 5, heads * 64), 7.0, dtype=torch.bfloat16, device="cuda")
    got = _run(x, T, heads, out=out).float().cpu().numpy()
    assert not np.isnan(got[:, :T]).any()
    assert (got[:, T:] == 7.0).all()
    clean = _run(np.ascontiguousarray(x[:, :T]), T, heads).float().cpu().numpy()
    assert np.array_equal(got[:, :T], clean)


def test_an_items_bits_do_not_depend_on_the_batch():
    x = _qkv(3, 200, 3, 5)
    all3 = _run(x, 200, 3)
    one = _run(np.ascontiguousarray(x[1:2]), 200, 3)
    assert torch.equal(all3[1], one[0])


def test_host_refusals():
    lib = _lib.load()
    x = _qkv(1, 16, 2, 3)
    with pytest.raises(KokoroHipError, match="ld is smaller"):
        _run(x, 16, 2, ld_claim=3 * 2 * 64 - 8)
    with pytest.raises(KokoroHipError, match="T_rows"):
        _run(x, 17, 2)
    # a head dimension other than 64: 128 channels over 4 heads
    kc = _lib.KKWhisperConfig(80, 100, 128, 4, 1)
    h = C.c_void_p()
    assert lib.kk_whisper_create(C.byref(kc), C.byref(h)) != 0
    assert b"head dimension" in lib.kk_last_error()
