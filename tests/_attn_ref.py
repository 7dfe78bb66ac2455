"""Shared helpers of the cache-attention kernel tests (test_gpu_csm_kernels.py, test_gpu_attn_cache_block.py): the RoPE table and rotation, the
float64 GQA attention, the single-token input cases, and the recorded-bits fixture tests/golden/attn_cache_bits.json."""
import hashlib
import json
import os

import numpy as np

BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_cache_bits.json")
RECORD_ENV = "KK_RECORD_ATTN_BITS"  # set (to anything non-empty): check_bits writes the fixture instead of comparing against it


def rope_table(rng, max_pos, hd):
    ang = rng.uniform(-np.pi, np.pi, (max_pos, hd // 2))
    ang[0] = 0.0
    return np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)


def rot32(x, cs):
    """the kernels' RoPE in fp32 arithmetic (no contraction): y0 = x0 c - x1 s, y1 = x1 c + x0 s on interleaved pairs"""
    x = np.asarray(x, np.float32)
    x0, x1, c, s = x[..., 0::2], x[..., 1::2], cs[..., 0], cs[..., 1]
    y = np.empty_like(x)
    y[..., 0::2] = x0 * c - x1 * s
    y[..., 1::2] = x1 * c + x0 * s
    return y


def rot64(x, cs):
    x, cs = np.asarray(x, np.float64), np.asarray(cs, np.float64)
    x0, x1, c, s = x[..., 0::2], x[..., 1::2], cs[..., 0], cs[..., 1]
    y = np.empty_like(x)
    y[..., 0::2] = x0 * c - x1 * s
    y[..., 1::2] = x1 * c + x0 * s
    return y


def attn_ref(q, keys, vals, scale):
    """q [H][hd], keys / vals [n][KV][hd] (float64) -> [H][hd]; GQA: head h reads kv head h / (H / KV)"""
    H, KV = q.shape[0], keys.shape[1]
    G = H // KV
    out = np.zeros(q.shape)
    for h in range(H):
        s = keys[:, h // G] @ q[h] * scale
        p = np.exp(s - s.max())
        out[h] = p @ vals[:, h // G] / p.sum()
    return out


def make_attn_case(rng, B, H, KV, hd, max_pos, offset, pads, regime, dom=None):
    """qkv [B][(H + 2 KV) hd], caches [B][max_pos][KV hd] (slots outside pad .. offset - 1 hold large junk no kernel may read), rope table.
    regime "large": scores up to ~80, the dominant key of item b at slot dom[b] (or the new key when dom[b] == offset)."""
    W = (H + 2 * KV) * hd
    rope = rope_table(rng, max_pos, hd)
    qkv = rng.standard_normal((B, W)).astype(np.float32)
    kc = (rng.standard_normal((B, max_pos, KV * hd)) * 1e3).astype(np.float32)
    vc = (rng.standard_normal((B, max_pos, KV * hd)) * 1e3).astype(np.float32)
    scale = 1.0 / np.sqrt(np.float32(hd))
    for b in range(B):
        live = slice(pads[b], offset)
        kc[b, live] = rng.standard_normal((offset - pads[b], KV * hd))
        vc[b, live] = rng.standard_normal((offset - pads[b], KV * hd))
        if regime == "large":
            kc[b, live] *= 3.0  # background scores of ~ +-10 .. 30
            if dom is not None and pads[b] <= dom[b] < offset:
                qr = rot64(qkv[b, : H * hd].reshape(H, hd), rope[offset - pads[b]])
                for kvh in range(KV):
                    qh = qr[kvh * (H // KV)]
                    kc[b, dom[b], kvh * hd : (kvh + 1) * hd] = qh * (80.0 / (scale * (qh @ qh)))
    return qkv, kc, vc, rope


def check_bits(case_id, *arrays):
    """SHA-256 of the arrays' raw bytes (in order) against the hash recorded under `case_id`.  The fixture was recorded from the kernels as
    they stood BEFORE the cache-attention family moved into kk_attn_cache.hip; with RECORD_ENV set the hash is written instead."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    digest = h.hexdigest()
    if os.environ.get(RECORD_ENV):
        rec = json.load(open(BITS)) if os.path.exists(BITS) else {}
        rec[case_id] = digest
        with open(BITS, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    rec = json.load(open(BITS))
    assert case_id in rec, f"{case_id}: no recorded hash"
    assert digest == rec[case_id], f"{case_id}: output bits differ from the recorded ones"
