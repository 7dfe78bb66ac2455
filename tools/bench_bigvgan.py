"""BigVGAN timing at the bigvgan_v2_24khz_100band_256x shape on synthetic weights: the forward (fp32 and bf16) at B = 1 and B = 8, 10 s of
audio per item; the fused activation (kk_op_bigvgan_amp_act) timed alone at every stage's tensor shape, times the launches the forward makes at that
shape, as its share of the forward; and for the first-stage and last-stage shapes its bytes per second (x read once, out written once) beside a
device-to-device copy of the same tensor, the floor a fused kernel can approach.
python tools/bench_bigvgan.py [--seconds 10] [--steps 5] [--out profiles/bigvgan_bench.json]      prints one JSON line"""
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
from mlx_audio_amd import _lib, bigvgan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--out", default="")
a = ap.parse_args()


def synth(shapes, seed=0):
    """random parameters: unit-gain convs, the residual branches and the last conv damped so that nothing saturates"""
    rng, w = np.random.default_rng(seed), {}
    for name, shape in shapes.items():
        if name.endswith((".filter", ".weight_g")):
            continue
        if name.endswith(".weight_v"):
            v = (rng.standard_normal(shape, dtype=np.float32) / math.sqrt(shape[1] * shape[2])).astype(np.float32)
            g = shapes[name[:-1] + "g"]
            gain = 0.3 if ".convs" in name else (0.25 if name.startswith("conv_post") else 1.0)
            w[name[:-1] + "g"] = (gain * np.sqrt((v.astype(np.float64) ** 2).sum(axis=tuple(i for i in range(3) if g[i] == 1), keepdims=True))).astype(np.float32)
        elif name.endswith((".alpha", ".beta")):
            v = rng.uniform(-0.5, 0.5, shape)
        else:
            v = 0.05 * rng.standard_normal(shape)
        w[name] = v.astype(np.float32)
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


cfg = bigvgan.bigvgan_v2_24khz_100band_256x()
hop, sr = int(np.prod(cfg.upsample_rates)), 24000
T = int(round(a.seconds * sr / hop))
w = synth(bigvgan.param_shapes(cfg))
# (rows, channels, activation launches) per stage, and the last activation before conv_post
per_block = sum(len(d) for d in cfg.resblock_dilation_sizes) * (2 if cfg.resblock == "1" else 1)
shapes, L = [], T
for i, u in enumerate(cfg.upsample_rates):
    L *= u
    shapes.append((L, cfg.upsample_initial_channel >> (i + 1), per_block + (1 if i == len(cfg.upsample_rates) - 1 else 0)))
out = {"metric": "ms per call, BigVGAN bigvgan_v2_24khz_100band_256x on synthetic weights", "seconds_per_item": T * hop / sr, "mel_frames": T, "steps": a.steps,
       "activation_launches_per_forward": sum(s[2] for s in shapes), "forward": [], "activation_kernel": [], "data": "synthetic (random weights, random mel)"}
rng = np.random.default_rng(0)
lib = _lib.load()
P = lambda t: C.c_void_p(t.data_ptr())
for dt, tdt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
    m = bigvgan.BigVGAN(cfg, w, compute_dtype=dt)
    for B in a.batches:
        mel = torch.tensor(rng.standard_normal((B, cfg.num_mels, T)).astype(np.float32), device="cuda")
        ms = timed(lambda: m(mel), a.steps)
        act_ms = 0.0
        for si, (L, Cc, n) in enumerate(shapes):
            ld = Cc if dt == "float32" else (Cc + 63) // 64 * 64  # the forward's pitches
            x = torch.randn(B, L, ld, device="cuda").to(tdt)
            y = torch.empty_like(x)
            al, ib = torch.ones(Cc, device="cuda"), torch.ones(Cc, device="cuda")  # alpha = 1, 1 / (beta + 1e-9) = 1: the kernel alone, tables on the device

            def act():
                _lib.check(lib.kk_op_bigvgan_amp_act(C.c_void_p(torch.cuda.current_stream().cuda_stream), B, P(x), L * ld, ld, int(dt == "bfloat16"), L, Cc, P(al), P(ib),
                                                     P(y), L * ld, ld, 0), "kk_op_bigvgan_amp_act")

            k_ms = timed(act, 20 * a.steps)
            act_ms += n * k_ms
            if si in (0, len(shapes) - 1):
                xc, yc = x[:, :, :Cc].contiguous(), torch.empty(B, L, Cc, device="cuda", dtype=tdt)
                c_ms = timed(lambda: yc.copy_(xc), 20 * a.steps)
                nbytes = 2 * B * L * Cc * x.element_size()
                out["activation_kernel"].append({"stage": si, "batch": B, "dtype": dt, "rows": L, "channels": Cc, "ms": k_ms, "gbs": nbytes / (k_ms * 1e-3) / 1e9,
                                                 "copy_ms": c_ms, "copy_gbs": nbytes / (c_ms * 1e-3) / 1e9})
                del xc, yc
            del x, y
        out["forward"].append({"batch": B, "dtype": dt, "ms": ms, "xRT": B * T * hop / sr / (ms * 1e-3), "activation_ms": act_ms, "activation_share": act_ms / ms})
        del mel
        torch.cuda.empty_cache()
    del m
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
