"""CSM-1B frame generation rate (config 4): B streams, one prompt block then N single-token frames; audio-seconds (80 ms per frame)
per wall-second.  python tools/bench_csm.py [--batch 8] [--prompt 64] [--frames 10] [--weights float32|bfloat16|q8|q4] [--group-size 64]
--top-k / --top-p / --min-p: the sampler (defaults: top-50 alone, the shipped configuration); --rng device: Philox uniforms inside the sampling kernels.
--row-samplers: the frame loop in table mode (generate_frame(sampler="rows")) with the sampler above stored in every row's table entry, to be
compared with the same command without the flag (launch-argument mode).
--weights q8 / q4: the synthetic checkpoint MLX-affine-quantised (quant.quantize_checkpoint) and kept packed in device memory."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_audio_amd.params as P  # noqa: E402
from mlx_audio_amd.csm import SesameModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--prompt", type=int, default=64)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--e2e", action="store_true", help="config 4 end to end: reference-audio prompt (Mimi.encode) -> frame loop -> Mimi.decode")
ap.add_argument("--weights", default="float32", choices=["float32", "bfloat16", "q8", "q4"],
                help="weight storage of the Linear layers (kk_csm_set_weight_dtype; q8 / q4: a quantised checkpoint, packed storage)")
ap.add_argument("--group-size", type=int, default=64, help="quantisation group of --weights q8 / q4")
ap.add_argument("--top-k", type=int, default=50, help="0: no top-k filter (the whole vocabulary)")
ap.add_argument("--top-p", type=float, default=0.0)
ap.add_argument("--min-p", type=float, default=0.0)
ap.add_argument("--rng", default="host", choices=["host", "device"], help="host: injected uniforms (resident on the device); device: Philox in the sampling kernels")
ap.add_argument("--row-samplers", action="store_true", help="read every row's sampler from the device table (set_row_sampler) instead of launch arguments")
a = ap.parse_args()
cfg = P.csm_config()
t0 = time.time()
w = P.csm_synth_checkpoint(cfg, 0)
quantization = None
if a.weights in ("q8", "q4"):
    from mlx_audio_amd.quant import csm_quantised_layer_names, quantize_checkpoint

    # (the embedding tables are gather tables, dequantised at load whatever the storage: left as floats here to spare the host their quantisation)
    names = [k for k in csm_quantised_layer_names(w, a.group_size) if not k.endswith("embeddings.weight")]
    quantization = {"group_size": a.group_size, "bits": int(a.weights[1])}
    w = quantize_checkpoint(w, a.group_size, quantization["bits"], names=names)
t1 = time.time()
model = SesameModel(cfg, w, weight_dtype="float32" if quantization else a.weights, quantization=quantization)
storage = {"weight_format": model.weight_format, "weight_fallback": model.weight_fallback, "weight_bytes": model.weight_bytes}
wname = {"float32": "fp32", "bfloat16": "bf16 weights / fp32 arithmetic"}.get(a.weights, f"{a.weights} packed weights (group {a.group_size}) / fp32 arithmetic")
del w
model.setup_caches(a.batch)
t2 = time.time()
rng = np.random.default_rng(0)
n, B = cfg["audio_num_codebooks"], a.batch
if a.e2e:
    from mlx_audio_amd.mimi import Mimi, mimi_202407
    from mlx_audio_amd.sesame import Model, Segment

    mcfg = P.mimi_config(32)
    mimi = Mimi(mimi_202407(32), P.mimi_synth_checkpoint(mcfg, 0, encode=True), compute_dtype="bfloat16")
    loop = Model(model, mimi)
    ref = [(0.1 * rng.standard_normal(24000 * 2)).astype(np.float32) for _ in range(B)]  # 2 s of reference audio per stream
    ctx = [[Segment(speaker=0, text=rng.integers(0, cfg["text_vocab_size"], 24).tolist(), audio=ref[b])] for b in range(B)]
    prompts = [loop.prompt_frames(ctx[b], rng.integers(0, cfg["text_vocab_size"], 24).tolist(), 0, voice_match=False) for b in range(B)]
    loop.generate_batch(prompts, max_audio_length_ms=80 * 3, stop_on_eos=False)  # warm-up
    res = loop.generate_batch(prompts, max_audio_length_ms=80 * a.frames, stop_on_eos=False)
    secs = res.audio[0].shape[0] / 24000.0
    print(json.dumps({"metric": "audio-sec/sec (xRT), CSM-1B end to end: reference-audio prompt (Mimi.encode) + text ids -> frames -> Mimi.decode",
                      "value": B * secs / res.processing_time_seconds, "wall_s": res.processing_time_seconds, "audio_s_per_stream": secs, "batch": B,
                      "frames": res.frames[0], "prompt_frames": 24 + 26 + 24, "dtype": ("f32" if a.weights == "float32" else a.weights + "-weight") + " frame generator, fp32 Mimi.encode, bf16 Mimi.decode", **storage,
                      "data": "synthetic (random-init weights, random token ids, noise reference audio, EOS ignored)",
                      "setup_s": {"synth_checkpoint": round(t1 - t0, 1), "load_finalize": round(t2 - t1, 1)}}))
    sys.exit(0)
tok = np.zeros((B, a.prompt, n + 1), np.int64)
msk = np.zeros((B, a.prompt, n + 1), np.float32)
tok[:, :, -1] = rng.integers(0, cfg["text_vocab_size"], (B, a.prompt))
msk[:, :, -1] = 1
from mlx_audio_amd.sesame import make_sampler  # noqa: E402

sampler = make_sampler(temp=0.9, top_k=a.top_k, top_p=a.top_p, min_p=a.min_p)


if a.row_samplers:
    for b in range(B):
        model.set_row_sampler(b, sampler, seed=0)


def frame(t, m, u):
    if a.row_samplers:
        return model.generate_frame(t, m, sampler="rows", device_rng=True) if a.rng == "device" else model.generate_frame(t, m, sampler="rows", uniforms=u)
    if a.rng == "device":
        return model.generate_frame(t, m, sampler=sampler, seed=0)
    return model.generate_frame(t, m, sampler=sampler, uniforms=u)


torch.cuda.synchronize()
tp = time.perf_counter()
codes = frame(torch.tensor(tok), torch.tensor(msk), torch.tensor(rng.uniform(size=(B, n)).astype(np.float32)))
torch.cuda.synchronize()
prefill_ms = (time.perf_counter() - tp) * 1e3
# the same prompt again on reset caches: without the first call's one-time costs (kernel loading, workspace allocation)
model.reset_caches()
ptok, pmsk, pu = torch.tensor(tok).cuda(), torch.tensor(msk).cuda(), torch.tensor(rng.uniform(size=(B, n)).astype(np.float32)).cuda()
torch.cuda.synchronize()
tp = time.perf_counter()
codes = frame(ptok, pmsk, pu)
torch.cuda.synchronize()
prefill2_ms = (time.perf_counter() - tp) * 1e3
step_tok = torch.zeros((B, 1, n + 1), dtype=torch.int32, device="cuda")
step_msk = torch.zeros((B, 1, n + 1), dtype=torch.float32, device="cuda")
step_msk[:, 0, :n] = 1
us = torch.tensor(rng.uniform(size=(a.frames + 3, B, n)).astype(np.float32), device="cuda")
model.set_graph_mode(True)
for i in range(3):  # warm-up frames (eager, capture, first replay)
    step_tok[:, 0, :n] = codes
    codes = frame(step_tok, step_msk, us[i])
torch.cuda.synchronize()
ts = time.perf_counter()
for i in range(a.frames):
    step_tok[:, 0, :n] = codes
    codes = frame(step_tok, step_msk, us[3 + i])
torch.cuda.synchronize()
dt = (time.perf_counter() - ts) / a.frames
print(json.dumps({"metric": "audio-sec/sec (xRT), CSM-1B frame generation (80 ms of audio per frame and stream), " + wname, "value": B * 0.08 / dt,
                  "ms_per_frame": dt * 1e3, "batch": B, "prompt_tokens": a.prompt, "prefill_ms": prefill_ms, "prefill_ms_second_call": prefill2_ms, "frames_timed": a.frames, "dtype": wname, **storage,
                  "sampler": {"temp": 0.9, "top_k": a.top_k, "top_p": a.top_p, "min_p": a.min_p, "rng": a.rng,
                              "settings": "per-row table" if a.row_samplers else "launch arguments"},
                  "data": "synthetic (random-init CSM-1B weights, random prompt, " + ("injected uniforms)" if a.rng == "host" else "device uniforms)"),
                  "setup_s": {"synth_checkpoint": round(t1 - t0, 1), "load_finalize": round(t2 - t1, 1)}}))
