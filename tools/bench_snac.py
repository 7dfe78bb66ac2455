"""SNAC codec timing at the snac_24khz shape on synthetic weights: SNAC.decode (fp32 and bf16) and SNAC.encode (fp32) at B = 1 and
B = 8, 10 s of audio per item; the residual unit of every decoder block on its own (kk_op_snac_residual_unit: the depth-wise launch + the 1x1
launch) with its bytes per second beside a device-to-device copy of the same size; launches per decode with and without a fused unit.
python tools/bench_snac.py [--seconds 10] [--steps 5] [--out profiles/snac_bench.json]      prints one JSON line"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mlx_audio_amd import _lib, snac  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--out", default="")
a = ap.parse_args()


def synth(shapes, seed=0):
    """random parameters: unit-gain convs, the residual 1x1s and the last conv damped so that the tanh is not saturated"""
    rng, w = np.random.default_rng(seed), {}
    for name, shape in shapes.items():
        if name.endswith(".alpha"):
            v = rng.uniform(0.5, 2.0, shape)
        elif name.endswith(".weight_v"):
            v = rng.standard_normal(shape) / math.sqrt(shape[1] * shape[2])
        elif name.endswith(".weight_g"):
            continue
        elif name.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape)
        w[name] = v.astype(np.float32)
    for name, shape in shapes.items():
        if name.endswith(".weight_g"):
            v = w[name[:-1] + "v"].astype(np.float64)
            gain = 0.3 if name.endswith(".block.layers.3.weight_g") else (0.25 if shape[0] == 1 else 1.0)
            w[name] = (gain * np.sqrt((v**2).sum(axis=(1, 2), keepdims=True))).astype(np.float32)
    return w


def timed(fn, steps):
    """ms per call (GPU events) after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


cfg = snac.snac_24khz()
w = synth(snac.param_shapes(cfg))
models = {dt: snac.SNAC(cfg, w, compute_dtype=dt) for dt in ("float32", "bfloat16")}
lib = _lib.load()
unit = models["float32"].pad_to()
N = math.ceil(a.seconds * cfg.sampling_rate / unit) * unit
T = N // models["float32"].hop_length
rng = np.random.default_rng(0)
out = {"metric": "ms per call, SNAC snac_24khz on synthetic weights", "seconds_per_item": N / cfg.sampling_rate, "latent_frames": T, "steps": a.steps,
       "decode": [], "encode": [], "residual_unit": [], "data": "synthetic (random weights, random codes, noise audio)"}
nb = len(cfg.decoder_rates)
out["launches_per_decode"] = {"unfused": 3 + nb * (2 + (2 if cfg.noise else 0) + 6) + 1, "with_a_fused_unit": 3 + nb * (2 + (2 if cfg.noise else 0) + 3) + 1,
                              "note": "the fused residual unit is not built: the codec runs the unfused count"}
for B in a.batches:
    codes = [torch.tensor(rng.integers(0, cfg.codebook_size, (B, T // s)), device="cuda", dtype=torch.int32) for s in cfg.vq_strides]
    audio = torch.tensor((0.3 * rng.standard_normal((B, 1, N))).astype(np.float32), device="cuda")
    for dt, m in models.items():
        noise = [n.cuda() for n in m.draw_noise(B, 0)]
        ms = timed(lambda: m.decode(codes, noise=noise), a.steps)
        out["decode"].append({"batch": B, "dtype": dt, "ms": ms, "xRT": B * N / cfg.sampling_rate / (ms * 1e-3)})
    ms = timed(lambda: models["float32"].encode(audio), a.steps)
    out["encode"].append({"batch": B, "dtype": "float32", "ms": ms, "xRT": B * N / cfg.sampling_rate / (ms * 1e-3)})
    del codes, audio
    torch.cuda.empty_cache()


# the residual unit of each decoder block on its own, dil 9 (the widest halo), and a copy of the same tensor for scale
def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
L = T
for l, s in enumerate(cfg.decoder_rates):
    L, Cc = L * s, cfg.decoder_dim >> (l + 1)
    for B in a.batches:
        for dt, tdt, es in (("float32", torch.float32, 4), ("bfloat16", torch.bfloat16, 2)):
            x = torch.randn(B, L, Cc, device="cuda").to(tdt)
            tmp, y = torch.empty_like(x), torch.empty_like(x)
            dw, db = torch.randn(Cc, 7, device="cuda") / 7**0.5, torch.zeros(Cc, device="cuda")
            a1, a2 = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")
            pw = 0.3 * torch.randn(Cc, Cc, device="cuda") / Cc**0.5  # [O][I]
            ldw = (Cc + 63) // 64 * 64
            pk = torch.zeros(1, Cc, ldw, device="cuda")
            pk[0, :, :Cc] = pw.t()
            wf, CinP, CoutP, bias = None, 0, 0, torch.zeros(ldw + 128, device="cuda")
            if dt == "bfloat16":
                CinP, CoutP = (Cc + 63) // 64 * 64, (Cc + 127) // 128 * 128
                wb = torch.zeros(1, CoutP, CinP, device="cuda", dtype=torch.bfloat16)
                wb[0, :Cc, :Cc] = pw.to(torch.bfloat16)
                wf = torch.empty_like(wb)
                _lib.check(lib.kk_op_pack_w_frag(st(), P(wb), P(wf), 1, CoutP, CinP), "kk_op_pack_w_frag")
            path = C.c_int(-1)

            def run():
                _lib.check(lib.kk_op_snac_residual_unit(st(), B, P(x), Cc, int(dt == "bfloat16"), L, Cc, 9, P(dw), P(db), P(a1), P(a2), P(pk), ldw, P(wf), CinP,
                                                        CoutP, P(bias), P(tmp), P(y), Cc, C.byref(path)), "kk_op_snac_residual_unit")

            ms = timed(run, a.steps)
            ms_copy = timed(lambda: y.copy_(x), a.steps)
            nbytes = B * L * Cc * es
            out["residual_unit"].append({"block": l, "batch": B, "dtype": dt, "rows": L, "channels": Cc, "ms": ms, "path_1x1": path.value,
                                         # x read and y written once is what a fused unit would move; the two launches move x twice, tmp twice, y once
                                         "gbs_ideal_traffic": 2 * nbytes / (ms * 1e-3) / 1e9, "gbs_moved": 5 * nbytes / (ms * 1e-3) / 1e9,
                                         "copy_ms": ms_copy, "copy_gbs": 2 * nbytes / (ms_copy * 1e-3) / 1e9})
            del x, tmp, y
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
