"""Times of long-form transcription (mlx-audio_amd/whisper_transcribe.py) at the whisper-large-v3-turbo shape -- 128 mels, a 32-layer encoder over
1500 positions of width 1280, a 4-layer decoder -- on seeded synthetic weights, in ONE process:

 (a) the round with 8 live step rows (rows_forward of 8 one-token items + rows_pick) with every row greedy next to the same round with every row
     sampling at temperature 1 (kk_whisper_text_rows_set_draw), at the same fixed position, sampled in turn, each the median of `--steps` samples of
     `--inner` calls between two device events;
 (b) whether `embed_audio` on 8 windows gives every row the bits of its B = 1 call at this shape (the contract of `transcribe` rests on it);
 (c) 16 files of 2 to 5 thirty-second windows (seeded noise) through `Model.transcribe` with `max_rows=8` against the same files one after the other
     (`max_rows=1`), in windows per second of wall time with the device idle before and after, the median of `--repeats` runs; the results of the two
     are compared with ==.  `without_timestamps` keeps a window's advance at its size (random weights would otherwise sample random timestamps) and
     synthetic weights never sample eot, so a window costs `--sample-len` tokens per pass.  Two settings: greedy only (`logprob_threshold=None`), and the
     ladder (0.0, 0.4) under the default threshold, which random weights always miss: every window is decoded greedily, then sampled, on ONE encoding.

Usage:  python tools/bench_whisper_transcribe.py [--steps 20] [--warmup 3] [--inner 20] [--position 64] [--repeats 3] [--sample-len 100] [--out FILE.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_MELS, CTX, WIDTH, HEADS, ENC_LAYERS, DEC_LAYERS, VOCAB, TEXT_CTX = 128, 1500, 1280, 20, 32, 4, 51866, 448
ROWS, FILES, SEED = 8, 16, 20


def synthetic_model(enc_layers=ENC_LAYERS):
    """N(0, 1 / fan_in) matrices, one set of arrays shared by every layer (the time does not depend on the values being distinct)"""
    from mlx_audio_amd import whisper

    d = whisper.ModelDimensions(N_MELS, CTX, WIDTH, HEADS, enc_layers, VOCAB, TEXT_CTX, WIDTH, HEADS, DEC_LAYERS)
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
    return d, whisper.Model(d).load_weights(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--position", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample-len", type=int, default=100)
    ap.add_argument("--enc-layers", type=int, default=ENC_LAYERS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from mlx_audio_amd import whisper
    from mlx_audio_amd import whisper_decoding as WD

    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper_transcribe.py needs a GPU: a time taken elsewhere says nothing")
    if a.steps < 20:
        raise SystemExit("--steps must be at least 20 (the figures are medians)")
    d, model = synthetic_model(a.enc_layers)
    rt, tok = model._text, WD.special_tokens(d)
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    def timed_pair(fa, fb):
        """the two cases sample by sample in turn (other work shares the machine: what drifts, drifts for both)"""
        for _ in range(a.warmup):
            fa()
            fb()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(a.steps):
            for k, fn in enumerate((fa, fb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.inner)
        return [dict(ms_median=round(statistics.median(m), 4), ms_min=round(min(m), 4), ms_max=round(max(m), 4), steps=a.steps, warmup=a.warmup, inner=a.inner)
                for m in ms]

    # ---- (a) a round of 8 step rows: greedy rows, then the same rows sampling ---------------------------------------------------------------
    params, bits = WD.pick_params(d, tok, WD.DecodingOptions())
    feats = torch.randn((ROWS, CTX, WIDTH), generator=torch.Generator().manual_seed(ROWS)).cuda()
    prompt = torch.randint(0, 50000, (ROWS, a.position), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    items, out, every = [(r, a.position, 1, -1, -1, 0) for r in range(ROWS)], list(range(ROWS)), list(range(ROWS))

    def open_rows(sampled):
        rows = WD.RowRuntime(rt, ROWS)
        for r in range(ROWS):
            rows.admit(r, feats[r], prompt[r].numpy(), params, bits)
            if sampled:
                rows.set_draw(r, 1.0, SEED, r)
        rows.forward([(r, 0, a.position, 0, -1, 0) for r in range(ROWS)], [(r + 1) * a.position - 1 for r in range(ROWS)])
        rows.pick(every)
        return rows

    # one handle has one row state at a time: the two cases are timed one after the other, each against the launch-wide static step as its yardstick
    def static_step():
        rt.rewind(a.position)
        rt.step()
        rt.pick()

    rt.set_audio(feats)
    rt.pick_setup(params, bits)
    rt.forward(prompt.cuda(), False)
    rt.pick()
    for name, sampled in (("row_round_8_greedy_rows", False), ("row_round_8_sampled_rows", True)):
        rows = open_rows(sampled)

        def round_of_steps(rows=rows):
            rows.forward(items, out)
            rows.pick(every)

        static, rnd = timed_pair(static_step, round_of_steps)
        emit(dict(case=name, rows=ROWS, position=a.position, static_decode_step_ms=static["ms_median"], **rnd))
        del rows

    # ---- (b) the encoder on 8 windows against each window alone -----------------------------------------------------------------------------------
    mel = torch.randn((ROWS, 2 * CTX, N_MELS), generator=torch.Generator().manual_seed(5)).cuda()
    together = model.embed_audio(mel)
    equal = [bool(torch.equal(together[r], model.embed_audio(mel[r].clone()))) for r in range(ROWS)]
    emit(dict(case="embed_audio_rows_equal_their_solo_call", B=ROWS, equal=equal, all_equal=all(equal)))
    del mel, together

    # ---- (c) 16 files through transcribe: 8 rows against one file after the other -------------------------------------------------------------------
    g = np.random.default_rng(SEED)
    n_windows = [int(n) for n in g.integers(2, 6, FILES)]
    seconds = [30.0 * (n - 1) + float(g.uniform(5.0, 29.0)) for n in n_windows]
    clips = [(0.1 * g.standard_normal(int(s * 16000))).astype(np.float32) for s in seconds]
    total = sum(n_windows)

    def wall(fn):
        fn()  # warm
        secs, last = [], None
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return dict(seconds_median=round(statistics.median(secs), 4), seconds_min=round(min(secs), 4), seconds_max=round(max(secs), 4),
                    windows_per_s=round(total / statistics.median(secs), 2)), last

    for name, kw, passes in (("transcribe_16_files_greedy", dict(logprob_threshold=None), 1),
                             ("transcribe_16_files_greedy_then_sampled", dict(temperature=(0.0, 0.4)), 2)):
        opts = dict(compression_ratio_threshold=None, language=0, without_timestamps=True, sample_len=a.sample_len, seed=SEED, **kw)
        batched, rb = wall(lambda: model.transcribe(clips, max_rows=ROWS, **opts))
        serial, rs = wall(lambda: [model.transcribe(c, max_rows=1, **opts) for c in clips])
        windows = [len({s["seek"] for s in r.segments}) for r in rb]
        emit(dict(case=name, files=FILES, windows_per_file=n_windows, windows_total=total, windows_seen=sum(windows), passes_per_window=passes,
                  sample_len=a.sample_len, tokens_total=sum(len(r.tokens) for r in rb), results_equal=rb == rs, max_rows_8=batched, max_rows_1_one_file_at_a_time=serial,
                  repeats=a.repeats, speedup=round(serial["seconds_median"] / batched["seconds_median"], 3)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0),
                           shape=dict(n_mels=N_MELS, ctx=CTX, width=WIDTH, heads=HEADS, encoder_layers=a.enc_layers, decoder_layers=DEC_LAYERS, n_vocab=VOCAB),
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
