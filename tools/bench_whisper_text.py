"""Times of the Whisper text side (mlx-audio_amd/whisper_decoding.py, csrc/kk_whisper_text.hip and kk_whisper_text_kernels.hip) at the whisper-large-v3-turbo decoder shape
-- 4 layers of width 1280, 20 heads, 51866 tokens, 1500 audio positions -- on synthetic weights, for B = 1 and 8: `set_audio` (the cross K/V of a
window), a 4-token prefill, and the steady-state decode step (one forward of S = 1 plus one pick) at a fixed position, with the bytes the step must
read and the rate that makes of the measured time.  Every figure is the median of `--steps` samples after `--warmup`, each sample `--inner` calls
between two device events.  Prints one JSON line per case.

The per-step share of each kernel family comes from a run of its own under the profiler (tracing slows the host, so no time above is taken there):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_whisper_text.py --only-steps 200 --batch 8 [--weights q4 --layers 32]
    python tools/bench_whisper_text.py --digest DIR/.../k_kernel_trace.csv --digest-steps 200 --batch 8 [--out the bench's file: appended]

`--align` times the token-timestamp path instead (mlx-audio_amd/whisper_timing.py, csrc/kk_whisper_align.hip) at the same shape: a 448-token
sequence (443 text tokens, 444 warped rows) against 1500 frames with the default alignment heads (the upper two layers, 40 heads), B = 1 and 8 -- the
capturing forward, `align_matrix`, and the DTW with its backtrace, each between device events of its own (the two raw entries read their row and column
counts back, so their figures include that round trip).  The kernels' own durations come from a profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_whisper_text.py --align --only-steps 20 --batch 8

`--best-of G` and / or `--temperature T` time sampling instead (mlx-audio_amd/whisper_sampling.py): for 1 and 8 windows of G rows each, the plain
state of the same row count on repeated features (`set_audio`, the step with the greedy pick) against the grouped state on ONE cross K/V slice per window
(`set_audio_groups`, the step with the sampled pick when T > 0), either pick alone, and the two states' sizes.

`--beam K` times beam search instead (mlx-audio_amd/whisper_beam.py): for 1 and 8 windows of K rows each on the grouped state, the beam step
(forward through the owner table + top-k + select) next to the sampled `best_of = K` step at temperature 1, either pick alone, the forward alone at
key counts 32, 224 and 448 under both (four layers of owned against direct self-attention on the same keys are all that differs), and the bytes of
the beam state next to the grouped state.

`--weights bf16|q8|q4 [--group-size 64] [--layers N]` times the greedy decode step on a synthetic MLX-quantised checkpoint instead: the
checkpoint is loaded twice in one process, "dequantized" (the bf16 kernels, which are what a float checkpoint runs) and "packed" (the decoder's matrices
and the token embedding kept as integers), and the two models' steps are timed in alternating rounds at B = 1 and 8, each round the median of `--steps`
samples.  `bf16` times the dequantised model against itself: the spread of a repeated measurement.  `--layers 4` (the default) is the large-v3-turbo
decoder, `--layers 32` large-v3's.  Every case carries both models' `weight_report()` and is appended to `--out`.

Usage:  python tools/bench_whisper_text.py [--steps 20] [--warmup 3] [--inner 20] [--position 64] [--out profiles/whisper_text_bench.json]
        python tools/bench_whisper_text.py --align [--steps 20] [--warmup 3] [--out profiles/whisper_align_bench.json]
        python tools/bench_whisper_text.py --best-of 5 --temperature 1.0 [--steps 20] [--warmup 3] [--out profiles/whisper_sample_bench.json]
        python tools/bench_whisper_text.py --beam 5 [--steps 20] [--warmup 3] [--out profiles/whisper_beam_bench.json]
        python tools/bench_whisper_text.py --weights q4 [--group-size 64] [--layers 32] [--rounds 5] [--out profiles/whisper_text_bench.json]"""
import argparse
import csv
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CTX, WIDTH, HEADS, LAYERS, VOCAB, TEXT_CTX = 1500, 1280, 20, 4, 51866, 448

FAMILIES = (("linear_rows", "linear_rows_kernel"), ("linear_rows (packed)", "linear_rows_q_kernel"), ("embed + row tables", "embed_q_kernel"), ("attention", "attn_rows_kernel"), ("attention", "attn_merge_kernel"), ("layernorm", "layernorm_kernel"),
            ("pick", "pick_kernel"), ("pick", "pick_sampled_kernel"), ("beam top-k", "beam_topk_kernel"), ("beam select", "beam_select_kernel"), ("embed + row tables", "embed_kernel"), ("embed + row tables", "text_rows_kernel"))


def step_bytes(B, position):
    """what one decode step must read, from the shapes: every block Linear and the tied embedding once (bf16), every layer's cross K/V of every row
    and the self K/V up to the position (bf16); and what it must write and re-read of the logits (fp32: written once, read twice by the pick)"""
    D = WIDTH
    weights = LAYERS * 14 * D * D * 2
    embedding = VOCAB * D * 2
    cross = LAYERS * B * CTX * 2 * D * 2
    self_kv = LAYERS * B * (position + 1) * 2 * D * 2
    logits = B * VOCAB * 4 * 3
    return dict(block_weights=weights, embedding=embedding, cross_kv=cross, self_kv=self_kv, logits=logits, total=weights + embedding + cross + self_kv + logits)


def digest(path, steps):
    """rocprofv3's kernel_trace.csv of an --only-steps run -> microseconds per step and share by kernel family, over the dispatches AFTER the first pick
    (what comes before it is the window's set-up and the prompt), and the steps' span from the first dispatch's start to the last one's end"""
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    first = next(i for i, r in enumerate(rows) if "pick_kernel" in r[2] or "pick_sampled_kernel" in r[2] or "beam_select_kernel" in r[2])
    rows = rows[first + 1:]
    fam, calls, total, other = {}, {}, 0.0, 0.0
    for t0, t1, name in rows:
        for label, needle in FAMILIES:
            if needle in name:
                fam[label] = fam.get(label, 0.0) + (t1 - t0)
                calls[label] = calls.get(label, 0) + 1
                total += t1 - t0
                break
        else:
            other += t1 - t0
    span = rows[-1][1] - rows[0][0]
    return dict(case="step_kernel_families", steps=steps, us_per_step=round(total / steps / 1e3, 2), span_us_per_step=round(span / steps / 1e3, 2),
                other_kernels_us_per_step=round(other / steps / 1e3, 2),
                families={k: dict(us_per_step=round(v / steps / 1e3, 2), launches_per_step=round(calls[k] / steps, 2), share=round(v / max(total, 1.0), 4))
                          for k, v in sorted(fam.items(), key=lambda kv: -kv[1])})


def synthetic_weights():
    """N(0, 1 / fan_in) matrices, one set of arrays shared by every layer (the time does not depend on the values being distinct)"""
    from mlx_audio_amd import whisper

    d = whisper.ModelDimensions(128, CTX, WIDTH, HEADS, 1, VOCAB, TEXT_CTX, WIDTH, HEADS, LAYERS)
    g = np.random.default_rng(0)
    made = {}

    def arr(shape):
        if shape not in made:
            fan_in = shape[-1] * (shape[1] if len(shape) == 3 else 1)
            made[shape] = (g.standard_normal(shape, dtype=np.float32) / np.float32(math.sqrt(fan_in))) if len(shape) > 1 else \
                (0.1 * g.standard_normal(shape)).astype(np.float32)
        return made[shape]

    shapes = {**whisper.encoder_shapes(d), **whisper.decoder_shapes(d)}
    w = {k: (np.ones(s, np.float32) if "ln" in k and k.endswith("weight") else arr(s)) for k, s in shapes.items()}
    return d, w


def synthetic_model():
    from mlx_audio_amd import whisper

    d, w = synthetic_weights()
    return d, whisper.Model(d).load_weights(w)


def quantised_models(bits, group):
    """(dims, the model on the dequantised checkpoint, the model on the packed one); bits None: the dequantised model alone, twice.  A distinct array is
    quantised once however many layers share it."""
    from mlx_audio_amd import quant, whisper

    d, w = synthetic_weights()
    q, deq, done = dict(w), dict(w), {}
    for k in quant.whisper_quantised_layer_names(w, group):
        if id(w[k]) not in done:
            t = quant.quantize_affine(w[k], group, bits or 4)
            done[id(w[k])] = (t, quant.dequantize_affine(*t, group, bits or 4))
        (words, scales, biases), back = done[id(w[k])]
        p = k[: -len(".weight")]
        q[k], q[p + ".scales"], q[p + ".biases"], deq[k] = words, scales, biases, back
    bf16 = whisper.Model(d).load_weights(deq)
    if bits is None:
        return d, bf16, bf16
    return d, bf16, whisper.Model(d).load_weights(q, {"group_size": group, "bits": bits}, "packed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--position", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-steps", type=int, default=0, help="run this many decode steps and nothing else (the profiler's run)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--align", action="store_true", help="time the token-timestamp path (capturing forward, align_matrix, dtw) instead of the decode step")
    ap.add_argument("--temperature", type=float, default=0.0, help="> 0: the grouped state's picks are sampled at this temperature (DESIGN 8j)")
    ap.add_argument("--best-of", type=int, default=0, help="G > 0: time G rows per window on one cross K/V slice against the plain state of as many rows")
    ap.add_argument("--beam", type=int, default=0, help="K > 0: time the beam step of K rows per window against the sampled best_of = K step (DESIGN 8k)")
    ap.add_argument("--weights", choices=("bf16", "q8", "q4"), default=None, help="time the step on a quantised checkpoint, packed against dequantised (DESIGN 8l)")
    ap.add_argument("--group-size", type=int, default=64)
    ap.add_argument("--layers", type=int, default=LAYERS, help="decoder layers of the --weights shape: 4 (large-v3-turbo) or 32 (large-v3)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per model of --weights")
    ap.add_argument("--digest", default=None)
    ap.add_argument("--digest-steps", type=int, default=200)
    a = ap.parse_args()
    if a.digest:
        r = digest(a.digest, a.digest_steps)
        print(json.dumps(r))
        if a.out and os.path.exists(a.out):  # appended to the bench's file
            with open(a.out) as f:
                doc = json.load(f)
            doc["results"].append(dict(r, B=a.batch, **(dict(weights=a.weights, layers=a.layers) if a.weights else {})))
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        return
    import torch

    from mlx_audio_amd import _lib
    from mlx_audio_amd import whisper_decoding as WD

    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper_text.py needs a GPU: a time taken elsewhere says nothing")
    if a.steps < 20 and not a.only_steps:
        raise SystemExit("--steps must be at least 20 (the figures are medians)")
    if a.weights:
        return bench_weights(a)
    d, model = synthetic_model()
    rt, tok = model._text, WD.special_tokens(d)
    params = _lib.KKWhisperPickParams(n_vocab=d.n_vocab, eot=tok.eot, blank=WD.BLANK_TOKEN, no_timestamps=tok.no_timestamps, timestamp_begin=tok.timestamp_begin,
                                      max_initial_timestamp_index=50, without_timestamps=0, suppress_blank=1)
    bits = WD.suppress_bitmask(d.n_vocab, WD.suppress_list(tok, WD.DecodingOptions()))

    def begin(B):
        feats = torch.randn((B, CTX, WIDTH), generator=torch.Generator().manual_seed(B)).cuda()
        rt.set_audio(feats)
        rt.pick_setup(params, bits)
        prompt = torch.randint(0, 50000, (B, a.position), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()
        rt.forward(prompt, False)  # the self K/V up to the position
        rt.pick()
        return feats

    def step():
        rt.rewind(a.position)  # host only: every timed step runs at the same position
        rt.step()
        rt.pick()

    if a.only_steps and not a.align:
        begin(a.batch)
        for _ in range(a.only_steps):
            step()
        torch.cuda.synchronize()
        return

    def timed(fn, inner):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), steps=a.steps, warmup=a.warmup, inner=inner)

    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    def write_out():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(device=torch.cuda.get_device_name(0), shape=dict(ctx=CTX, width=WIDTH, heads=HEADS, layers=LAYERS, n_vocab=VOCAB, n_text_ctx=TEXT_CTX),
                               results=results), f, indent=1)
                f.write("\n")

    if a.align:
        from mlx_audio_amd import whisper_timing as WT

        heads = model.alignment_heads
        text = [int(t) for t in np.random.default_rng(3).integers(0, tok.eot, TEXT_CTX - 5)]  # sot, language, task, no_timestamps, 443 text tokens, eot
        seq, r0, r1 = WT.alignment_tokens(d, text)
        for B in ((a.batch,) if a.only_steps else (1, 8)):
            feats = torch.randn((B, CTX, WIDTH), generator=torch.Generator().manual_seed(B)).cuda()
            rt.set_audio(feats)
            toks = torch.tensor([seq] * B, dtype=torch.int32).cuda()
            rows, frames = [len(seq)] * B, [CTX] * B
            state = {}

            def forward():
                rt.rewind(0)
                state["qk"] = rt.forward_qk(toks, heads, CTX)[1]

            def plain():
                rt.rewind(0)
                rt.forward(toks, True)

            def matrix():
                state["mat"] = WT.align_matrix_rows(state["qk"], rows, frames, 7, 1.0)

            def warp():
                state["path"] = WT.dtw_rows(state["warped"], [r1 - r0] * B, frames, negate=True)

            if a.only_steps:  # the profiler's run: the three stages back to back and nothing else
                for _ in range(a.only_steps):
                    forward()
                    matrix()
                    state["warped"] = state["mat"][:, r0:r1].contiguous()
                    warp()
                torch.cuda.synchronize()
                return
            emit(dict(case="align_forward_plain", B=B, tokens=len(seq), **timed(plain, 1)))
            emit(dict(case="align_forward_qk", B=B, tokens=len(seq), pairs=int(heads.shape[0]), n_keys=CTX, **timed(forward, 1)))
            emit(dict(case="align_matrix", B=B, heads=int(heads.shape[0]), rows=len(seq), frames=CTX, medfilt_width=7, **timed(matrix, 1)))
            state["warped"] = state["mat"][:, r0:r1].contiguous()
            r = timed(warp, 1)
            emit(dict(case="align_dtw_and_backtrace", B=B, rows=r1 - r0, frames=CTX, path_length=int(state["path"][2][0]), **r))
        write_out()
        return

    if a.best_of or a.temperature:
        G = a.best_of or 1
        if a.temperature < 0 or not 1 <= G <= _lib.WHISPER_MAX_GROUP:
            raise SystemExit(f"--temperature must be >= 0 and --best-of in 1 .. {_lib.WHISPER_MAX_GROUP}")
        lib = rt._lib
        for windows in ((a.batch,) if a.only_steps else (1, 8)):
            B = windows * G
            feats = torch.randn((windows, CTX, WIDTH), generator=torch.Generator().manual_seed(windows)).cuda()
            prompt = torch.randint(0, 50000, (B, a.position), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()

            def begin_state(grouped):
                if grouped:
                    rt.set_audio_groups(feats, G)
                else:
                    rt.set_audio(feats.repeat_interleave(G, dim=0).contiguous())
                rt.pick_setup(params, bits)
                if grouped and a.temperature > 0:
                    rt.sample_setup(a.temperature, 0, np.arange(B))
                rt.forward(prompt, False)
                rt.pick()

            if a.only_steps:  # the profiler's run: the grouped state's steps and nothing else
                begin_state(True)
                for _ in range(a.only_steps):
                    step()
                torch.cuda.synchronize()
                return
            emit(dict(case="state_bytes", windows=windows, G=G, rows=B, plain=int(lib.kk_whisper_text_state_bytes(rt._h, B)),
                      grouped=int(lib.kk_whisper_text_state_bytes_groups(rt._h, windows, G))))
            for grouped in (False, True):
                kind = dict(windows=windows, G=G, rows=B, state="grouped" if grouped else "plain, repeated features",
                            pick="sampled" if grouped and a.temperature > 0 else "greedy", temperature=a.temperature if grouped else 0.0)
                rep = feats.repeat_interleave(G, dim=0).contiguous()
                begin_state(grouped)
                emit(dict(case="set_audio", **kind, **timed((lambda: rt.set_audio_groups(feats, G)) if grouped else (lambda: rt.set_audio(rep)), 1)))
                del rep
                begin_state(grouped)
                emit(dict(case="decode_step", position=a.position, **kind, **timed(step, a.inner)))
                emit(dict(case="pick_only", **kind, **timed(rt.pick, a.inner)))
        write_out()
        return

    if a.beam:
        K = a.beam
        if not 1 <= K <= _lib.WHISPER_MAX_GROUP:
            raise SystemExit(f"--beam must be in 1 .. {_lib.WHISPER_MAX_GROUP}")
        lib = rt._lib
        for windows in ((a.batch,) if a.only_steps else (1, 8)):
            B = windows * K
            feats = torch.randn((windows, CTX, WIDTH), generator=torch.Generator().manual_seed(windows)).cuda()

            def begin_beam(beam, position):
                prompt = torch.randint(0, 50000, (B, position), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()
                rt.set_audio_groups(feats, K)
                rt.pick_setup(params, bits)
                if beam:
                    rt.beam_setup(K, K)
                else:
                    rt.sample_setup(1.0, 0, np.arange(B))
                rt.forward(prompt, False)
                rt.pick()
                a.position = position  # what step() rewinds to
                step()  # (beam: one select has run, so the forward reads through a table that is no longer the identity)

            def forward_only():
                rt.rewind(a.position)
                rt.step()

            if a.only_steps:  # the profiler's run: the beam's steps and nothing else
                begin_beam(True, a.position)
                for _ in range(a.only_steps):
                    step()
                torch.cuda.synchronize()
                return
            position = a.position
            emit(dict(case="state_bytes", windows=windows, K=K, rows=B, grouped=int(lib.kk_whisper_text_state_bytes_groups(rt._h, windows, K)),
                      beam=int(lib.kk_whisper_text_beam_state_bytes(rt._h, windows, K, K))))
            for beam in (False, True):
                kind = dict(windows=windows, K=K, rows=B, pick="beam top-k + select" if beam else "sampled, temperature 1.0")
                begin_beam(beam, position)
                emit(dict(case="decode_step", position=position, **kind, **timed(step, a.inner)))
                emit(dict(case="pick_only", **kind, **timed(rt.pick, a.inner)))
            for keys in (32, 224, 448):  # the forward alone, alternating the two states at every key count
                for beam in (False, True, False, True):
                    begin_beam(beam, keys - 1)
                    emit(dict(case="forward_only", keys=keys, windows=windows, K=K, rows=B, self_attention="owned" if beam else "direct", **timed(forward_only, a.inner)))
            a.position = position
        write_out()
        return

    for B in (1, 8):
        feats = begin(B)
        emit(dict(case="set_audio", B=B, **timed(lambda: rt.set_audio(feats), 1)))
        begin(B)
        four = torch.randint(0, 50000, (B, 4), generator=torch.Generator().manual_seed(2), dtype=torch.int32).cuda()

        def prefill():
            rt.rewind(0)
            rt.forward(four, True)

        emit(dict(case="prefill_4_tokens", B=B, **timed(prefill, 1)))
        begin(B)
        r = timed(step, a.inner)
        by = step_bytes(B, a.position)
        emit(dict(case="decode_step", B=B, position=a.position, bytes=by, tbytes_per_s=round(by["total"] / (r["ms_median"] * 1e-3) / 1e12, 3),
                  tokens_per_s=round(B / (r["ms_median"] * 1e-3), 1), note="forward(S = 1) + pick, eager launches, no host synchronisation inside the window", **r))

        def forward_only():
            rt.rewind(a.position)
            rt.step()

        emit(dict(case="decode_step_forward_only", B=B, position=a.position, **timed(forward_only, a.inner)))
        emit(dict(case="pick_only", B=B, **timed(rt.pick, a.inner)))
    write_out()


def bench_weights(a):
    """--weights: see the module's text"""
    global LAYERS
    import torch

    from mlx_audio_amd import _lib
    from mlx_audio_amd import whisper_decoding as WD

    LAYERS = a.layers
    bits = {"bf16": None, "q8": 8, "q4": 4}[a.weights]
    d, m_bf16, m_q = quantised_models(bits, a.group_size)
    tok = WD.special_tokens(d)
    params = _lib.KKWhisperPickParams(n_vocab=d.n_vocab, eot=tok.eot, blank=WD.BLANK_TOKEN, no_timestamps=tok.no_timestamps, timestamp_begin=tok.timestamp_begin,
                                      max_initial_timestamp_index=50, without_timestamps=0, suppress_blank=1)
    mask = WD.suppress_bitmask(d.n_vocab, WD.suppress_list(tok, WD.DecodingOptions()))
    sides = (("bf16", m_bf16), ("bf16 again" if bits is None else a.weights, m_q))
    if a.only_steps:  # the profiler's run: the steps of the --weights model and nothing else
        rt = m_q._text
        rt.set_audio(torch.randn((a.batch, CTX, WIDTH), generator=torch.Generator().manual_seed(a.batch)).cuda())
        rt.pick_setup(params, mask)
        rt.forward(torch.randint(0, 50000, (a.batch, a.position), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda(), False)
        rt.pick()
        for _ in range(a.only_steps):
            rt.rewind(a.position)
            rt.step()
            rt.pick()
        torch.cuda.synchronize()
        return
    results = []
    for B in (1, 8):
        feats = torch.randn((B, CTX, WIDTH), generator=torch.Generator().manual_seed(B)).cuda()
        prompt = torch.randint(0, 50000, (B, a.position), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()

        def begin(rt):
            rt.set_audio(feats)
            rt.pick_setup(params, mask)
            rt.forward(prompt, False)  # the self K/V up to the position
            rt.pick()

        def sample(rt):  # the median of --steps samples of --inner steps each, between device events
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    rt.rewind(a.position)  # host only: every timed step runs at the same position
                    rt.step()
                    rt.pick()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.inner)
            return statistics.median(ms)

        rounds = {name: [] for name, _ in sides}
        for r in range(a.rounds + 1):  # round 0 warms both up and is dropped
            for name, m in sides:
                if r == 0:  # each model keeps its own window state
                    begin(m._text)
                t = sample(m._text)
                if r:
                    rounds[name].append(round(t, 4))
        base, other = (rounds[name] for name, _ in sides)
        res = dict(case="decode_step_by_weights", weights=a.weights, group_size=a.group_size, layers=a.layers, B=B, position=a.position,
                   bf16_ms_rounds=base, bf16_ms_median=round(statistics.median(base), 4), bf16_spread_ms=round(max(base) - min(base), 4),
                   other=sides[1][0], other_ms_rounds=other, other_ms_median=round(statistics.median(other), 4),
                   other_minus_bf16_ms=round(statistics.median(other) - statistics.median(base), 4), steps=a.steps, inner=a.inner, rounds=a.rounds,
                   bf16_weight_report=m_bf16.weight_report(), other_weight_report=m_q.weight_report())
        results.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        doc = dict(device=torch.cuda.get_device_name(0), results=[])
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["results"].extend(results)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
