"""Vocos timing at the vocos-mel-24khz shape on synthetic weights: the forward (fp32 and bf16) at B = 1 and B = 8, 10 s of audio per item; the
two new kernels timed alone at the forward's shapes (kk_op_vocos_dwconv_ln times the num_layers launches a forward makes, kk_op_vocos_istft once) as their
share of the forward; and each kernel's bytes per second (x / h read once, the output written once) beside a device-to-device copy of the same tensors
timed in the same session, the floor a fused kernel can approach.  The iSTFT is also timed at group = 13 (16 frames a workgroup, 19 % re-transformed
instead of 37.5 %).
python tools/bench_vocos.py [--seconds 10] [--steps 20] [--out profiles/vocos_bench.json]      prints one JSON line"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mlx_audio_amd import _lib, vocos  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--out", default="")
a = ap.parse_args()


def synth(shapes, seed=0):
    """random parameters: unit-gain matrices, norm weights 1, gamma 0.5, the head's magnitude rows damped so that exp stays under the clip"""
    rng, w = np.random.default_rng(seed), {}
    for name, shape in shapes.items():
        if name.endswith(".weight") and len(shape) >= 2:
            v = rng.standard_normal(shape) / math.sqrt(np.prod(shape[1:]))
            if name == "head.out.weight":
                v[: shape[0] // 2] *= 0.5
        elif name.endswith((".norm.weight", "_norm.weight")):
            v = np.ones(shape)
        elif name.endswith(".gamma"):
            v = np.full(shape, 0.5)
        else:
            v = 0.05 * rng.standard_normal(shape)
        w[name] = v.astype(np.float32)
    return w


def timed(fn, steps):
    """ms per call (GPU events) after three warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


cfg = vocos.vocos_mel_24khz()
sr, D, N, hop = 24000, cfg.dim, cfg.n_fft, cfg.hop_length
T = int(round(a.seconds * sr / hop))
w = synth(vocos.param_shapes(cfg))
out = {"metric": "ms per call, Vocos vocos-mel-24khz on synthetic weights", "seconds_per_item": (T - 1) * hop / sr, "frames": T, "steps": a.steps,
       "dwconv_ln_launches_per_forward": cfg.num_layers, "forward": [], "dwconv_ln_kernel": [], "istft_kernel": [],
       "data": "synthetic (random weights, random features)"}
rng = np.random.default_rng(0)
lib = _lib.load()
P = lambda t: C.c_void_p(t.data_ptr())
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
kw, kb = (torch.tensor(w[f"backbone.convnext.0.dwconv.{s}"], device="cuda").reshape(D, -1).contiguous() for s in ("weight", "bias"))
lw, lb = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
for dt, tdt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
    m = vocos.Vocos(cfg, w, compute_dtype=dt)
    for B in a.batches:
        feat = torch.tensor(rng.standard_normal((B, T, cfg.input_channels)).astype(np.float32), device="cuda")
        ms = timed(lambda: m.decode(feat), a.steps)
        # the fused dwconv -> LayerNorm at the forward's shape: fp32 in, the compute dtype out (pitch rounded up to 64 for bf16, as the forward's)
        ldo = D if dt == "float32" else (D + 63) // 64 * 64
        x, y = torch.randn(B, T, D, device="cuda"), torch.empty(B, T, ldo, device="cuda", dtype=tdt)

        def dw():  # the library entry directly: the kernel alone, its parameters already on the device
            _lib.check(lib.kk_op_vocos_dwconv_ln(S(), B, P(x), T * D, D, T, D, P(kw), P(kb), P(lw), P(lb), 0, 1e-6, P(y), T * ldo, ldo, int(dt == "bfloat16"), 0), "dwconv_ln")

        dw_ms = timed(dw, 10 * a.steps)
        yc = torch.empty(B, T, D, device="cuda", dtype=tdt)
        c_ms = timed(lambda: yc.copy_(x), 10 * a.steps)
        nbytes = B * T * D * (4 + y.element_size())
        out["dwconv_ln_kernel"].append({"batch": B, "out_dtype": dt, "rows": T, "channels": D, "rows_per_workgroup": vocos.dwconv_rows(D), "ms": dw_ms,
                                        "gbs": nbytes / (dw_ms * 1e-3) / 1e9, "copy_ms": c_ms, "copy_gbs": nbytes / (c_ms * 1e-3) / 1e9})
        rec = {"batch": B, "dtype": dt, "ms": ms, "xRT": B * (T - 1) * hop / sr / (ms * 1e-3), "dwconv_ln_ms": cfg.num_layers * dw_ms,
               "dwconv_ln_share": cfg.num_layers * dw_ms / ms}
        if dt == "float32":  # the iSTFT is fp32 in both modes: timed once per batch
            h = torch.randn(B, T, N + 2 + 6, device="cuda") * torch.cat([torch.full((N // 2 + 1,), 0.5), torch.full((N // 2 + 1,), 4.0), torch.ones(6)]).cuda()
            hv = h[:, :, : N + 2]
            hc, oc = torch.empty(B, T, N + 2, device="cuda"), torch.empty(B, (T - 1) * hop, device="cuda")
            src = torch.empty(B, (T - 1) * hop, device="cuda")
            nb = 4 * B * (T * (N + 2) + (T - 1) * hop)

            def copies():
                hc.copy_(hv)
                oc.copy_(src)

            c_ms = timed(copies, 10 * a.steps)
            for g in (0, 13):
                i_ms = timed(lambda: _lib.check(lib.kk_op_vocos_istft(S(), B, T, P(h), T * (N + 8), N + 8, N, hop, P(oc), (T - 1) * hop, g), "istft"), 10 * a.steps)
                out["istft_kernel"].append({"batch": B, "frames": T, "n_fft": N, "group": g or 5, "ms": i_ms, "gbs": nb / (i_ms * 1e-3) / 1e9, "copy_ms": c_ms,
                                            "copy_gbs": nb / (c_ms * 1e-3) / 1e9})
            del h, hc, oc, src
        ist = next(r for r in out["istft_kernel"] if r["batch"] == B and r["group"] == 5)
        rec.update({"istft_ms": ist["ms"], "istft_share": ist["ms"] / ms})
        out["forward"].append(rec)
        del feat, x, y, yc
        torch.cuda.empty_cache()
    del m
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
