"""Times of the Whisper audio side (mlx-audio_amd/whisper.py, csrc/kk_whisper.hip) at the whisper-large-v3-turbo encoder shape --
128 mels, 1500 positions of width 1280, 20 heads, 32 layers -- on synthetic weights: the encoder per 30 s window at B = 1 and B = 8, the
attention kernel alone (as TFLOP/s of its 4 T^2 64 heads B FLOPs) and the log-mel of 30 s of audio.  Every figure is the median of `--steps`
calls after `--warmup`, each call between two device events.  Prints one JSON line per case.

Usage:  python tools/bench_whisper.py [--steps 20] [--warmup 3] [--layers 32] [--out profiles/whisper_bench.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd import _lib  # noqa: E402
from mlx_audio_amd import whisper  # noqa: E402

N_MELS, CTX, WIDTH, HEADS = 128, 1500, 1280, 20


def timed(fn, steps, warmup):
    """median / min / max milliseconds of fn() between device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), steps=steps, warmup=warmup)


def synthetic_model(layers):
    """N(0, 1 / fan_in) matrices, one set of arrays shared by every layer (the time does not depend on the values being distinct)"""
    d = whisper.ModelDimensions(N_MELS, CTX, WIDTH, HEADS, layers, 51866, 448, WIDTH, HEADS, 4)
    g = np.random.default_rng(0)
    made = {}

    def arr(shape):
        if shape not in made:
            fan_in = shape[-1] * (shape[1] if len(shape) == 3 else 1)
            made[shape] = (g.standard_normal(shape) / math.sqrt(fan_in)).astype(np.float32) if len(shape) > 1 else \
                (0.1 * g.standard_normal(shape)).astype(np.float32)
        return made[shape]

    w = {k: (np.ones(s, np.float32) if "ln" in k and k.endswith("weight") else arr(s)) for k, s in whisper.encoder_shapes(d).items()}
    return d, whisper.Model(d).load_weights(w)


def encoder_flops(d, B):
    D, T = d.n_audio_state, d.n_audio_ctx
    per_layer = 2 * T * 12 * D * D + 4 * T * T * D
    stem = 2 * 2 * T * 3 * d.n_mels * D + 2 * T * 3 * D * D
    return B * (d.n_audio_layer * per_layer + stem)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper.py needs a GPU: a time taken elsewhere says nothing")
    if a.steps < 20:
        raise SystemExit("--steps must be at least 20 (the figures are medians)")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    # log-mel of 30 s
    x = (0.1 * torch.randn(whisper.N_SAMPLES, generator=torch.Generator().manual_seed(0))).cuda()
    for B in (1, 8):
        rows = x.repeat(B, 1).contiguous()
        r = timed(lambda: whisper.log_mel_rows(rows, [whisper.N_SAMPLES] * B, N_MELS, 0), a.steps, a.warmup)
        emit(dict(case="log_mel_30s", B=B, n_mels=N_MELS, frames=whisper.N_FRAMES, note="includes the upload of the lengths and two allocations", **r))

    # the attention kernel alone
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B in (1, 8):
        qkv = torch.randn((B, CTX, 3 * WIDTH), generator=torch.Generator().manual_seed(1)).cuda().to(torch.bfloat16)
        out = torch.empty((B, CTX, WIDTH), dtype=torch.bfloat16, device="cuda")
        r = timed(lambda: _lib.check(lib.kk_op_attention_long(st, B, C.c_void_p(qkv.data_ptr()), 3 * WIDTH, CTX, CTX, HEADS, C.c_void_p(out.data_ptr()),
                                                              WIDTH), "kk_op_attention_long"), a.steps, a.warmup)
        flops = 4 * CTX * CTX * 64 * HEADS * B
        emit(dict(case="attention_long", B=B, T=CTX, heads=HEADS, flops=flops, tflops=round(flops / (r["ms_median"] * 1e-3) / 1e12, 2), **r))

    # the encoder
    d, model = synthetic_model(a.layers)
    for B in (1, 8):
        mel = (0.5 * torch.randn((B, 2 * CTX, N_MELS), generator=torch.Generator().manual_seed(2))).cuda()
        r = timed(lambda: model.embed_audio(mel), a.steps, a.warmup)
        flops = encoder_flops(d, B)
        emit(dict(case="encoder", B=B, layers=a.layers, ms_per_window=round(r["ms_median"] / B, 4), flops=flops,
                  tflops=round(flops / (r["ms_median"] * 1e-3) / 1e12, 2), **r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), shape=dict(n_mels=N_MELS, ctx=CTX, width=WIDTH, heads=HEADS, layers=a.layers),
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
