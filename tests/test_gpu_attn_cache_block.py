"""GPU tests, kernel level, of the KV-cache attention's block forms (kk_attn_cache.hip) through kk_op_attn_cache_block -- the launchers Mimi's
streaming transformer runs, on caller-owned buffers: the launch-wide form (kk_launch_rope_append + kk_launch_attn_cache, no causal mask) and
the per-row form (kk_launch_rope_append_rows + kk_launch_attn_cache_rows: row b at row_pos[b], rows with active[b] == 0 left alone).

* A row's bits in the per-row form are those of the launch-wide form run on that row alone at offset = row_pos[b]; the appended K and the
  rotated q are the fp32 RoPE expressions bit for bit; both forms are within 1e-5 of max|V| of the float64 windowed attention.
* A row that is inactive, or whose position is below 0 or past max_pos - S, appends nothing and gets a zero output; nothing outside
  [row_pos[b], row_pos[b] + S) of a cache is written.  Every buffer carries one spare row of a sentinel behind the B rows, so a missing
  device guard shows as changed bytes inside the allocation.
* The output bits of every case, and of a handful of kk_op_csm_attn_single / kk_op_csm_attn_prompt cases, equal the hashes recorded in
  tests/golden/attn_cache_bits.json from the kernels as they stood before they moved into their own file (_attn_ref.check_bits).
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from _attn_ref import attn_ref, check_bits, make_attn_case, rope_table, rot32, rot64
from _util import report

pytestmark = pytest.mark.gpu

B, MAX_POS = 4, 24
SENTINEL = np.float32(-123456.75)
CASES = list(itertools.product([64, 128], [(2, 2), (4, 2)], [1, 3], [-1, 6]))  # hd, (H, KV), S, ctx
IDS = [f"hd{hd}_H{H}_KV{KV}_S{S}_ctx{ctx}" for hd, (H, KV), S, ctx in CASES]


@pytest.fixture(scope="module")
def lib():
    from mlx_audio_amd import _lib

    return _lib.load()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(device="cuda", dtype=dtype).contiguous()  # (a copy: the shared inputs are read-only)


def P(t, row=0):
    return C.c_void_p(t[row:].data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def row_positions(S):
    return [0, 5, 20, MAX_POS - S]  # a fresh row, a short row, a row whose window slides past ctx = 6, the last position that fits


def make_inputs(hd, H, KV, S):
    """qkv [B + 1][S][W], caches [B + 1][MAX_POS][KV hd], out [B + 1][S][H hd]: the last row of each is the sentinel; cache slots at or above a row's
    position hold large junk that no kernel may read; the rope table has a spare row in front and behind."""
    rng = np.random.default_rng(hd * 100 + H * 10 + S)
    W = (H + 2 * KV) * hd
    pos = row_positions(S)
    rope = np.zeros((MAX_POS + 2, hd // 2, 2), np.float32)
    rope[1:-1] = rope_table(rng, MAX_POS, hd)
    qkv = rng.standard_normal((B + 1, S, W)).astype(np.float32)
    kc = (rng.standard_normal((B + 1, MAX_POS, KV * hd)) * 1e3).astype(np.float32)
    vc = (rng.standard_normal((B + 1, MAX_POS, KV * hd)) * 1e3).astype(np.float32)
    for b in range(B):
        kc[b, : pos[b]] = rng.standard_normal((pos[b], KV * hd))
        vc[b, : pos[b]] = rng.standard_normal((pos[b], KV * hd))
    out = np.full((B + 1, S, H * hd), 7.0, np.float32)
    for a in (qkv, kc, vc, out):
        a[B] = SENTINEL
    return qkv, kc, vc, out, rope


def run_block(lib, hd, H, KV, S, ctx, inputs, *, row_pos=None, active=None, row=0, nrows=B, offset=0):
    """kk_op_attn_cache_block on fresh device copies of `inputs`, over rows [row, row + nrows) -> (qkv, kc, vc, out) as numpy, all B + 1 rows"""
    qkv, kc, vc, out, rope = inputs
    qd, kd, vd, od, rd = dev(qkv), dev(kc), dev(vc), dev(out), dev(rope)
    pd = dev(np.asarray(row_pos, np.int32), torch.int32) if row_pos is not None else None
    ad = dev(np.asarray(active, np.int32), torch.int32) if row_pos is not None else None
    rc = lib.kk_op_attn_cache_block(stream(), nrows, S, H, KV, hd, P(qd, row), P(kd, row), P(vd, row), MAX_POS, offset, P(pd), P(ad), P(rd, 1), ctx,
                                    P(od, row))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    return qd.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy(), od.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(lib, hd, H, KV, S, ctx):
    """inputs, the per-row form with every row active, and the launch-wide form run on each row alone: computed once, shared, never modified"""
    inputs = make_inputs(hd, H, KV, S)
    pos = row_positions(S)
    rows = run_block(lib, hd, H, KV, S, ctx, inputs, row_pos=pos, active=[1] * B)
    wide = [run_block(lib, hd, H, KV, S, ctx, inputs, row=b, nrows=1, offset=pos[b]) for b in range(B)]
    for a in itertools.chain(inputs, rows, *wide):
        a.setflags(write=False)
    return inputs, rows, wide


def pieces(res, H, hd, S, pos, rows=range(B)):
    """what a call produces, row by row: out, the appended K and V rows, the rotated q"""
    qkv, kc, vc, out = res
    return [np.ascontiguousarray(a) for b in rows for a in (out[b], kc[b, pos[b] : pos[b] + S], vc[b, pos[b] : pos[b] + S], qkv[b, :, : H * hd])]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("hd,hkv,S,ctx", CASES, ids=IDS)
def test_per_row_form_has_the_bits_of_the_launch_wide_form_on_that_row(lib, hd, hkv, S, ctx):
    H, KV = hkv
    inputs, rows, wide = _case(lib, hd, H, KV, S, ctx)
    pos = row_positions(S)
    for b in range(B):
        got, alone = pieces(rows, H, hd, S, pos, [b]), pieces(wide[b], H, hd, S, pos, [b])
        for name, g, a in zip(("out", "k", "v", "q"), got, alone):
            np.testing.assert_array_equal(u32(g), u32(a), err_msg=f"row {b}: {name}")
        # the launch-wide call on row b alone left every other row of its buffers as it was
        for got_buf, inp in zip(wide[b], inputs):
            keep = np.ones(B + 1, bool)
            keep[b] = False
            np.testing.assert_array_equal(u32(got_buf[keep]), u32(inp[keep]), err_msg=f"row {b} alone")
    check_bits(f"block/{IDS[CASES.index((hd, hkv, S, ctx))]}/rows", *pieces(rows, H, hd, S, pos))
    check_bits(f"block/{IDS[CASES.index((hd, hkv, S, ctx))]}/wide", *[a for b in range(B) for a in pieces(wide[b], H, hd, S, pos, [b])])


@pytest.mark.parametrize("hd,hkv,S,ctx", CASES, ids=IDS)
def test_rope_bits_and_float64_reference(lib, hd, hkv, S, ctx):
    H, KV = hkv
    inputs, rows, wide = _case(lib, hd, H, KV, S, ctx)
    qkv, kc, vc, _, rope = inputs
    rope = rope[1:-1]
    pos = row_positions(S)
    scale = float(1.0 / np.sqrt(np.float32(hd)))
    for form, results in (("rows", [rows] * B), ("wide", wide)):
        err = 0.0
        for b in range(B):
            qg, kg, vg, og = results[b]
            cs = rope[pos[b] + np.arange(S)]  # [S][hd / 2][2]
            q32 = rot32(qkv[b, :, : H * hd].reshape(S, H, hd), cs[:, None])
            k32 = rot32(qkv[b, :, H * hd : (H + KV) * hd].reshape(S, KV, hd), cs[:, None])
            np.testing.assert_array_equal(u32(qg[b, :, : H * hd]), u32(q32.reshape(S, -1)), err_msg=f"{form} row {b}: q")
            np.testing.assert_array_equal(u32(kg[b, pos[b] : pos[b] + S]), u32(k32.reshape(S, -1)), err_msg=f"{form} row {b}: k")
            np.testing.assert_array_equal(u32(vg[b, pos[b] : pos[b] + S]), u32(qkv[b, :, (H + KV) * hd :]), err_msg=f"{form} row {b}: v")
            # every query of the block sees the keys [klo, pos + S): the last ctx cached ones and the block
            klo = pos[b] - ctx if ctx >= 0 and pos[b] > ctx else 0
            keys = kg[b, klo : pos[b] + S].reshape(-1, KV, hd).astype(np.float64)
            vals = vg[b, klo : pos[b] + S].reshape(-1, KV, hd).astype(np.float64)
            vmax = float(np.abs(vals).max())
            for s in range(S):
                ref = attn_ref(rot64(qkv[b, s, : H * hd].reshape(H, hd), cs[s]), keys, vals, scale).reshape(-1)
                err = max(err, float(np.abs(og[b, s] - ref).max()) / vmax)
            assert np.isfinite(og[b]).all()
        report(f"attn_cache_block/{form}/{IDS[CASES.index((hd, hkv, S, ctx))]}", err_over_vmax=err, bar=1e-5, ratio=err / 1e-5)
        assert err <= 1e-5, (form, err)


@pytest.mark.parametrize("hd,hkv,S,ctx", CASES, ids=IDS)
def test_nothing_else_is_written(lib, hd, hkv, S, ctx):
    H, KV = hkv
    inputs, rows, wide = _case(lib, hd, H, KV, S, ctx)
    qkv, kc, vc, out, _ = inputs
    qg, kg, vg, og = rows
    pos = row_positions(S)
    keep = np.ones((B + 1, MAX_POS), bool)
    for b in range(B):
        keep[b, pos[b] : pos[b] + S] = False
    np.testing.assert_array_equal(u32(kg[keep]), u32(kc[keep]))
    np.testing.assert_array_equal(u32(vg[keep]), u32(vc[keep]))
    np.testing.assert_array_equal(u32(qg[:, :, H * hd :]), u32(qkv[:, :, H * hd :]))  # the k and v parts of qkv are read only
    for a in (qg, kg, vg, og):
        assert (a[B] == SENTINEL).all()


@pytest.mark.parametrize("hd,hkv,S,ctx", CASES, ids=IDS)
@pytest.mark.parametrize("how", ["inactive", "below_zero", "past_the_end"])
def test_inert_row(lib, hd, hkv, S, ctx, how):
    """Row 1 is inactive, or sits at -1, or at max_pos - S + 1: its K / V keep their bytes, its output is zero, the other rows are those of the
    all-active call, the sentinel row is untouched."""
    H, KV = hkv
    inputs, rows, wide = _case(lib, hd, H, KV, S, ctx)
    qkv, kc, vc, out, _ = inputs
    pos = row_positions(S)
    active = [1, 0, 1, 1] if how == "inactive" else [1] * B
    if how != "inactive":
        pos[1] = -1 if how == "below_zero" else MAX_POS - S + 1
    qg, kg, vg, og = run_block(lib, hd, H, KV, S, ctx, inputs, row_pos=pos, active=active)
    np.testing.assert_array_equal(u32(kg[1]), u32(kc[1]))
    np.testing.assert_array_equal(u32(vg[1]), u32(vc[1]))
    np.testing.assert_array_equal(u32(qg[1]), u32(qkv[1]))
    assert not og[1].any()
    others = [0, 2, 3]
    for got, ref in zip((qg, kg, vg, og), rows):
        np.testing.assert_array_equal(u32(got[others]), u32(ref[others]))
        assert (got[B] == SENTINEL).all()
    check_bits(f"block/{IDS[CASES.index((hd, hkv, S, ctx))]}/{how}", og[:B], *pieces((qg, kg, vg, og), H, hd, S, pos, others))


def test_refusals_happen_before_any_launch(lib):
    qkv, kc, vc, out, rope = (torch.zeros(4096, device="cuda") for _ in range(5))
    pos, act = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.ones(4, dtype=torch.int32, device="cuda")

    def call(hd, max_pos, ctx, rows, S=1, offset=0):
        return lib.kk_op_attn_cache_block(stream(), 1, S, 2, 2, hd, P(qkv), P(kc), P(vc), max_pos, offset, P(pos) if rows else None,
                                          P(act) if rows else None, P(rope), ctx, P(out))

    for rows in (False, True):
        assert call(96, 4, -1, rows) != 0 and b"head_dim" in lib.kk_last_error()
        assert call(64, 20000, -1, rows) != 0  # the score buffer of 20000 keys: more than 64 KB of LDS
        assert call(64, 4, -1, rows, S=5) != 0
    assert call(64, 4, -1, False, offset=4) != 0 and call(64, 4, -1, False, offset=-1) != 0
    assert lib.kk_op_attn_cache_block(stream(), 1, 1, 2, 2, 64, P(qkv), P(kc), P(vc), 4, 0, P(pos), None, P(rope), -1, P(out)) != 0  # row_pos without active
    assert lib.kk_op_attn_cache_block(stream(), 1, 1, 2, 2, 64, None, P(kc), P(vc), 4, 0, None, None, P(rope), -1, P(out)) != 0
    torch.cuda.synchronize()
    for t in (qkv, kc, vc, out):
        assert not t.any()


# ---- the single-token and prompt entry points: recorded bits only (their parity tests are in test_gpu_csm_kernels.py)
@pytest.mark.parametrize("form,hd,max_pos", [(f, hd, mp) for f in (1, 2, 3) for hd in (64, 128) for mp in (33, 200) if not (f == 1 and mp > 64)])
def test_attn_single_recorded_bits(lib, form, hd, max_pos):
    G, KV, pads = 4, 2, [0, 5]
    H, offset = G * KV, max_pos - 2
    rng = np.random.default_rng(form * 1000 + hd + max_pos)
    qkv, kc, vc, rope = make_attn_case(rng, len(pads), H, KV, hd, max_pos, offset, pads, "moderate")
    qd, kd, vd, rd, pd = dev(qkv), dev(kc), dev(vc), dev(rope), dev(np.asarray(pads, np.int32), torch.int32)
    out = torch.full((len(pads), H * hd), 7.0, device="cuda")
    part = torch.full((8 * len(pads) * H * (hd + 2),), 5.0, device="cuda")
    rc = lib.kk_op_csm_attn_single(stream(), form, len(pads), H, KV, hd, P(qd), P(kd), P(vd), max_pos, offset, P(rd), P(pd), P(out), P(part))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    check_bits(f"single/form{form}_hd{hd}_mp{max_pos}", out.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy())


def test_attn_prompt_recorded_bits(lib):
    S, offset, G, hd, pads = 9, 30, 8, 64, [2, 0, 29]
    rng = np.random.default_rng(S + offset + hd)
    KV = 2
    H, nb = G * KV, len(pads)
    max_pos = offset + S + 5
    rope = rope_table(rng, max_pos, hd)
    qkv = rng.standard_normal((nb, S, (H + 2 * KV) * hd)).astype(np.float32)
    kc = (rng.standard_normal((nb, max_pos, KV * hd)) * 1e3).astype(np.float32)
    vc = (rng.standard_normal((nb, max_pos, KV * hd)) * 1e3).astype(np.float32)
    for b in range(nb):
        kc[b, pads[b] : offset] = rng.standard_normal((offset - pads[b], KV * hd))
        vc[b, pads[b] : offset] = rng.standard_normal((offset - pads[b], KV * hd))
    qd, kd, vd, rd, pd = dev(qkv), dev(kc), dev(vc), dev(rope), dev(np.asarray(pads, np.int32), torch.int32)
    out = torch.full((nb, S, H * hd), 7.0, device="cuda")
    rc = lib.kk_op_csm_attn_prompt(stream(), nb, S, H, KV, hd, P(qd), P(kd), P(vd), max_pos, offset, P(rd), P(pd), P(out))
    assert rc == 0, lib.kk_last_error()
    torch.cuda.synchronize()
    check_bits(f"prompt/S{S}_off{offset}_G{G}_hd{hd}", out.cpu().numpy(), qd.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy())
