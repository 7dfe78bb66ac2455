"""Times of the Parakeet encoder's kernels (mlx-audio_amd/parakeet.py, csrc/kk_parakeet.hip) at the parakeet-0.6b shape -- width 1024,
8 heads of 128, depth-wise k = 9, sub-sampling by 8 over 128 mels with 256 conv channels -- on random operands: the relative-position attention
at 30 s (T = 375) and 2 min (T = 1500), the same kernel at 16 heads of 64 next to kk_op_attention_long at the same T (the price of the positional
term), the conv core, the two forms of the 3 x 3 stride-2 conv and the log-mel of 30 s.  A figure is the median over `--steps` windows of `--inner` calls each, a
window between two device events.  FLOPs and bytes are what the algorithm needs, computed from the shapes.  Prints one JSON line per case.

The encoder (24 layers, synthetic weights) is timed per call for 30 s of features at B = 1 and B = 8.

Usage:  python tools/bench_parakeet.py [--layers 24] [--steps 20] [--warmup 3] [--inner 20] [--out profiles/parakeet_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd import _lib, parakeet  # noqa: E402

WIDTH, K, MELS, CONV_CH = 1024, 9, 128, 256


def timed(fn, steps, warmup, inner):
    """median / min / max milliseconds per call of fn(), `inner` calls between two device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return dict(ms_median=round(statistics.median(ms), 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5), steps=steps, warmup=warmup, inner=inner)


def synthetic_weights(enc):
    """N(0, 1 / fan_in) matrices under the reference's names, one set of arrays shared by every layer"""
    import numpy as np

    g, D, Cc, FF, k = np.random.default_rng(0), enc["d_model"], enc["subsampling_conv_channels"], 4 * enc["d_model"], enc["conv_kernel_size"]
    mat = lambda *s: (g.standard_normal(s) / np.sqrt(np.prod(s[1:]))).astype(np.float32)  # noqa: E731
    vec = lambda n, m=0.0: (m + 0.1 * g.standard_normal(n)).astype(np.float32)  # noqa: E731
    w, pre = {}, "encoder.pre_encode."
    for i, shape in ((0, (Cc, 3, 3, 1)), (2, (Cc, 3, 3, 1)), (3, (Cc, 1, 1, Cc)), (5, (Cc, 3, 3, 1)), (6, (Cc, 1, 1, Cc))):
        w[pre + f"conv.{i}.weight"], w[pre + f"conv.{i}.bias"] = mat(*shape), vec(Cc)
    w[pre + "out.weight"], w[pre + "out.bias"] = mat(D, Cc * enc["feat_in"] // 8), vec(D)
    layer = {}
    for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out", "conv.batch_norm"):
        layer[n + ".weight"], layer[n + ".bias"] = vec(D, 1.0), vec(D)
    layer["conv.batch_norm.running_mean"], layer["conv.batch_norm.running_var"] = vec(D), vec(D, 1.0)
    for n, shape in (("feed_forward1.linear1", (FF, D)), ("feed_forward1.linear2", (D, FF)), ("feed_forward2.linear1", (FF, D)), ("feed_forward2.linear2", (D, FF)),
                     ("self_attn.linear_q", (D, D)), ("self_attn.linear_k", (D, D)), ("self_attn.linear_v", (D, D)), ("self_attn.linear_out", (D, D)),
                     ("conv.pointwise_conv1", (2 * D, 1, D)), ("conv.depthwise_conv", (D, k, 1)), ("conv.pointwise_conv2", (D, 1, D))):
        layer[n + ".weight"], layer[n + ".bias"] = mat(*shape), vec(shape[0])
    layer["self_attn.linear_pos.weight"] = mat(D, D)
    layer["self_attn.pos_bias_u"], layer["self_attn.pos_bias_v"] = vec(D).reshape(enc["n_heads"], -1), vec(D).reshape(enc["n_heads"], -1)
    for li in range(enc["n_layers"]):
        w.update({f"encoder.layers.{li}.{n}": v for n, v in layer.items()})
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_parakeet.py needs a GPU: a time taken elsewhere says nothing")
    if a.steps < 20:
        raise SystemExit("--steps must be at least 20 (the figures are medians)")
    results = []
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randn(shape, generator=gen)  # noqa: E731

    def emit(r, t):
        r.update(t)
        if "flops" in r:
            r["tflops"] = round(r["flops"] / (r["ms_median"] * 1e-3) / 1e12, 2)
        if "bytes" in r:
            r["gb_per_s"] = round(r["bytes"] / (r["ms_median"] * 1e-3) / 1e9, 1)
        results.append(r)
        print(json.dumps(r), flush=True)

    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for T in (375, 1500):
        for B in (1, 8):
            for heads, hd in ((8, 128), (16, 64)):
                qkv, pos = rnd(B, T, 3 * WIDTH).cuda().bfloat16(), rnd(2 * T - 1, WIDTH).cuda().bfloat16()
                u, v = (0.5 * rnd(heads, hd)).cuda(), (0.5 * rnd(heads, hd)).cuda()
                out = torch.empty((B, T, WIDTH), dtype=torch.bfloat16, device="cuda")
                P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731  (both attention kernels are timed through the bare C entry)
                t = timed(lambda: _lib.check(lib.kk_op_rel_pos_attention(st, B, P(qkv), 3 * WIDTH, T, T, heads, hd, P(pos), WIDTH, P(u), P(v), P(out), WIDTH),
                                             "kk_op_rel_pos_attention"), a.steps, a.warmup, a.inner)
                emit(dict(case="rel_pos_attention", B=B, T=T, heads=heads, head_dim=hd, flops=6 * T * T * WIDTH * B,
                          note="flops: the two score products and the value product"), t)
            t = timed(lambda: _lib.check(lib.kk_op_attention_long(st, B, C.c_void_p(qkv.data_ptr()), 3 * WIDTH, T, T, 16, C.c_void_p(out.data_ptr()), WIDTH),
                                         "kk_op_attention_long"), a.steps, a.warmup, a.inner)
            emit(dict(case="attention_long", B=B, T=T, heads=16, head_dim=64, flops=4 * T * T * WIDTH * B, note="no positional term: the comparison"), t)
    for B in (1, 8):
        T = 375
        x, w, b = rnd(B, T, 2 * WIDTH).cuda().bfloat16(), (rnd(K, WIDTH) / 3).cuda(), (0.1 * rnd(WIDTH)).cuda()
        emit(dict(case="conformer_dwconv", B=B, T=T, D=WIDTH, k=K, bytes=B * T * WIDTH * 6, flops=2 * K * B * T * WIDTH),
             timed(lambda: parakeet.conformer_dwconv(x, w, b), a.steps, a.warmup, a.inner))
        mel, w9, b9 = rnd(B, 3000, MELS).cuda(), (rnd(9, CONV_CH) / 3).cuda(), (0.1 * rnd(CONV_CH)).cuda()
        emit(dict(case="conv2d_s2_stem", B=B, T=3000, F=MELS, C=CONV_CH, bytes=B * 3000 * MELS * 4 + B * 1500 * 64 * CONV_CH * 2),
             timed(lambda: parakeet.conv2d_s2(mel, w9, b9, True), a.steps, a.warmup, a.inner))
        y = rnd(B, 1500, 64, CONV_CH).cuda().bfloat16()
        emit(dict(case="conv2d_s2_depthwise", B=B, T=1500, F=64, C=CONV_CH, bytes=B * 1500 * 64 * CONV_CH * 2 + B * 750 * 32 * CONV_CH * 2),
             timed(lambda: parakeet.conv2d_s2(y, w9, b9, False), a.steps, a.warmup, a.inner))
    # the features of 30 s of audio
    pre = parakeet.PreprocessArgs(sample_rate=16000, normalize="per_feature", window_size=0.025, window_stride=0.01, window="hann", features=MELS, n_fft=512)
    for B in (1, 8):
        audio = (0.1 * rnd(B, 480000)).cuda()
        emit(dict(case="log_mel_30s", B=B, features=MELS, frames=3001, note="includes one allocation"), timed(lambda: parakeet.log_mel_spectrogram(audio, pre), a.steps, a.warmup, 1))
    # the encoder at the 0.6b shape on synthetic weights, 30 s of features
    enc = dict(feat_in=MELS, n_layers=a.layers, d_model=WIDTH, n_heads=8, ff_expansion_factor=4, subsampling_factor=8, conv_kernel_size=K,
               subsampling_conv_channels=CONV_CH, self_attention_model="rel_pos", subsampling="dw_striding", use_bias=True, xscaling=False)
    model = parakeet.Model(dict(encoder=enc, preprocessor={})).load_weights(synthetic_weights(enc))
    for B in (1, 8):
        mel = rnd(B, 3000, MELS).cuda()
        emit(dict(case="encoder_30s", B=B, layers=a.layers, T_mel=3000, note="includes the output's allocation; the workspace is kept across calls"), timed(lambda: model.encode(mel), a.steps, a.warmup, 1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), shape=dict(width=WIDTH, k=K, mels=MELS, conv_channels=CONV_CH), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
