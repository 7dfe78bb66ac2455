"""The bf16 fragment pack of the CSM matrix-core GEMV / prompt GEMM (kk_csm_frag_pack, kk_csm_frag_choice) on the host, no GPU: the layout
against a numpy restatement, the rounding against torch's float32 -> bfloat16, and the (split-K slices, sub-blocks) the generator picks for every
Linear of CSM-1B -- including shapes whose K slice the GEMV cannot run, which must get a runnable pack or none."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlx_audio_amd.params as P
from mlx_audio_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def bf16_bits(a):
    """torch's float32 -> bfloat16 (round to nearest even), as uint16 bit patterns."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def frag_pack_ref(w, nsub):
    """[K][N] -> [N / (16 nsub)][K / 32][nsub][64 lanes][8]: lane L of chunk c, sub-block s holds k = 32 c + 8 (L / 16) + j and column
    16 s + L % 16 of its block; the columns that pad N to whole blocks are zero."""
    K, N = w.shape
    cb = 16 * nsub
    nblk = -(-N // cb)
    wp = np.zeros((K, nblk * cb), np.float32)
    wp[:, :N] = w
    t = bf16_bits(wp).reshape(K // 32, 4, 8, nblk, nsub, 16)  # k = 32 c + 8 q + j, n = cb blk + 16 s + l
    return np.ascontiguousarray(t.transpose(3, 0, 4, 1, 5, 2)).reshape(-1)  # [blk][c][s][q][l][j], lane L = 16 q + l


def frag_pack(lib, w, nsub):
    K, N = w.shape
    w = np.ascontiguousarray(w, np.float32)
    out = np.full(-(-N // (16 * nsub)) * 16 * nsub * K, 0xBEEF, np.uint16)  # (every element must be written, padding included)
    rc = lib.kk_csm_frag_pack(w.ctypes.data_as(C.c_void_p), K, N, nsub, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.kk_last_error()
    return out


def frag_choice(lib, K, N, split_ok):
    ks, nsub = C.c_int32(-1), C.c_int32(-1)
    assert lib.kk_csm_frag_choice(K, N, int(split_ok), C.byref(ks), C.byref(nsub)) == 0
    return ks.value, nsub.value


@pytest.mark.parametrize("N", [16, 48, 2051])
@pytest.mark.parametrize("nsub", [1, 2, 4])
def test_frag_pack_layout_matches_numpy(lib, N, nsub):
    rng = np.random.default_rng(N * 10 + nsub)
    K = 96
    w = (rng.standard_normal((K, N)) * np.exp2(rng.integers(-20, 20, (K, N)))).astype(np.float32)
    w[0, : min(N, 5)] = [np.inf, -np.inf, -0.0, 1e-42, -3.4e38][: min(N, 5)]
    got = frag_pack(lib, w, nsub)
    np.testing.assert_array_equal(got, frag_pack_ref(w, nsub))
    # spot check of the rule itself (independent of the reshape above): element (k, n) sits at lane 16 (k % 32 / 8) + n % 16, j = k % 8
    cb, nch = 16 * nsub, K // 32
    for k, n in [(0, 0), (37, N - 1), (95, N // 2), (8, min(N - 1, 17))]:
        blk, s, c = n // cb, (n % cb) // 16, k // 32
        L = 16 * ((k % 32) // 8) + n % 16
        assert got[((((blk * nch) + c) * nsub + s) * 64 + L) * 8 + k % 8] == bf16_bits(w[k : k + 1, n])[0]


def test_frag_pack_rounding_matches_torch_on_edge_values(lib):
    bits = np.array([
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even, both signs
        0x3F808001, 0x3F807FFF,                          # just above / below a tie
        0x7F7FFFFF, 0x7F7F8000, 0xFF7FFFFF, 0xFF7F8000,  # round up to +-inf
        0x7F7F7FFF, 0xFF7F7FFF,                          # largest that stays finite
        0x7F800000, 0xFF800000,                          # +-inf
        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x80008000, 0x00017FFF,  # subnormals, ties among them, to the smallest normal
        0x00000000, 0x80000000,                          # signed zero
    ], np.uint32)
    vals = bits.view(np.float32)
    w = np.zeros((32, 16), np.float32)
    w.reshape(-1)[: vals.size] = vals
    got = frag_pack(lib, w, 1)
    np.testing.assert_array_equal(got, frag_pack_ref(w, 1))
    # and by value, without the layout: k = i // 16, n = i % 16 -> lane 16 (k / 8) + n, j = k % 8 (one chunk, one sub-block)
    for i, b in enumerate(bits):
        k, n = divmod(i, 16)
        assert got[(16 * (k // 8) + n) * 8 + k % 8] == bf16_bits(vals[i : i + 1])[0], hex(int(b))
    assert got[(16 * 0 + 6) * 8 + 0] == 0x7F80  # 0x7F7FFFFF -> +inf


def _linears(cfg):
    """(name, K, N, split_ok) of every Linear the generator packs."""
    out = []
    for stack in ("backbone", "decoder"):
        a = cfg[stack]
        H, KV, hd, D, I = a["num_heads"], a["num_kv_heads"], a["head_dim"], a["hidden"], a["intermediate"]
        out += [(f"{stack}.qkv", D, (H + 2 * KV) * hd, False), (f"{stack}.o", H * hd, D, False), (f"{stack}.gate_up", D, 2 * I, False),
                (f"{stack}.down", I, D, True)]
    D, Dd, V = cfg["backbone"]["hidden"], cfg["decoder"]["hidden"], cfg["audio_vocab_size"]
    return out + [("projection", D, Dd, False), ("codebook0_head", D, V, False), ("audio_head", Dd, V, False)]


# (ks, nsub) of every Linear of CSM-1B (llama-1B backbone, llama-100M depth decoder): derived from the rule -- split-K slices of 1024 rows for
# K >= 4096 on the down projections, then 4 / 2 / 1 sub-blocks where that still leaves >= 192 column blocks x slices
CSM1B_TABLE = {
    "backbone.qkv": (2048, 3072, 1, 1),
    "backbone.o": (2048, 2048, 1, 1),
    "backbone.gate_up": (2048, 16384, 1, 4),
    "backbone.down": (8192, 2048, 8, 4),
    "decoder.qkv": (1024, 1536, 1, 1),
    "decoder.o": (1024, 1024, 1, 1),
    "decoder.gate_up": (1024, 16384, 1, 4),
    "decoder.down": (8192, 1024, 8, 2),
    "projection": (2048, 1024, 1, 1),
    "codebook0_head": (2048, 2051, 1, 1),
    "audio_head": (1024, 2051, 1, 1),
}


def test_frag_choice_table_of_csm_1b(lib):
    lin = _linears(P.csm_config())
    assert {n for n, *_ in lin} == set(CSM1B_TABLE)
    for name, K, N, split_ok in lin:
        assert CSM1B_TABLE[name][:2] == (K, N), name
        assert frag_choice(lib, K, N, split_ok) == CSM1B_TABLE[name][2:], name


@pytest.mark.parametrize("K,N,split_ok,want", [
    (2240, 2048, False, (1, 1)),   # the longest K slice that fits the GEMV's 160 KiB of LDS
    (2272, 2048, False, (1, 0)),   # one chunk more: no pack (the stack runs on the fp32 path)
    (2304, 2304, False, (1, 0)),
    (2304, 2304, True, (2, 1)),    # a down projection takes two slices instead
    (3072, 2304, True, (2, 1)),
    (3072, 2304, False, (1, 0)),
    (4096, 4096, False, (1, 0)),   # a hidden-4096 stack's q|k|v: the form it is launched in takes no split-K
    (4096, 4096, True, (4, 4)),
    (2272, 2048, True, (1, 0)),    # 71 chunks: no slice count of whole chunks
    (4128, 512, True, (3, 1)),     # not a multiple of 1024: the first slice count that divides K into whole chunks and fits
    (16384, 2048, True, (16, 4)),
    (65536, 1024, True, (1, 0)),   # more than 16 slices of 2240 rows: none fits
    (1000, 512, False, (1, 0)),    # K not a multiple of 32
    (32, 16, False, (1, 1)),
])
def test_frag_choice_gives_only_runnable_packs(lib, K, N, split_ok, want):
    assert frag_choice(lib, K, N, split_ok) == want


def test_frag_choice_never_gives_a_pack_the_gemv_refuses(lib):
    # the launcher's limits: a K slice of at most 2240 rows (70 chunks of 32: 160 KiB of LDS), <= 16 slices of whole chunks, split-K only where allowed
    for K in range(32, 20000, 32):
        for split_ok in (False, True):
            ks, nsub = frag_choice(lib, K, 2048, split_ok)
            if nsub == 0:
                assert ks == 1
                continue
            assert nsub in (1, 2, 4) and 1 <= ks <= 16 and K % ks == 0 and (K // ks) % 32 == 0 and K // ks <= 2240, (K, split_ok, ks)
            assert split_ok or ks == 1
