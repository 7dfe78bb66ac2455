"""Times of Whisper serving (mlx-audio_amd/whisper_serve.py, row mode of csrc/kk_whisper_text.hip on the kernels of csrc/kk_whisper_text_kernels.hip) at the whisper-large-v3-turbo decoder shape
on synthetic weights (tools/bench_whisper_text.py's model), in ONE process:

 (a) the round with 8 live step rows (rows_forward of 8 one-token items + rows_pick) next to the static decode step at B = 8 (forward S = 1 + pick of
     window mode), both at the same fixed position, sampled in turn, each the median of `--steps` samples of `--inner` calls between two device events;
 (b) a mixed workload: 64 windows whose token counts come from a fixed seeded list between 4 and 200 (synthetic weights never sample eot, so a window's
     count is its `sample_len`), served in arrival order as static `decode` batches of 8 -- a batch runs to its longest row -- and through the batcher
     with 8 rows, in windows per second of wall time (device idle before and after), the median of `--repeats` runs.

With `--beam K` the mixed workload (b) is left out and two cases follow (a) instead:
 (c) a round of 6 beam groups of K rows (rows_forward of 6 K one-token items through the owner tables + rows_pick: the per-row top-k and one select
     workgroup per group) next to window mode's beam step at 6 windows x K (forward S = 1 + beam_topk + beam_select), same position, sampled in turn;
 (d) 32 windows with token counts from the seeded list of (b), at beam K: static `beam_search` batches of 6 in arrival order against `submit_beam` on
     a batcher of 6 K rows, in windows per second of wall time.

Usage:  python tools/bench_whisper_serve.py [--steps 20] [--warmup 3] [--inner 20] [--position 64] [--repeats 3] [--beam K]
                                            [--out profiles/whisper_serve_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS, WINDOWS, SEED = 8, 64, 20
BEAM_GROUPS, BEAM_WINDOWS = 6, 32  # 6 groups of 5 are 30 of KK_WHISPER_MAX_ROWS = 32 rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--position", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--beam", type=int, default=0, help="beam size: measure beam groups instead of the mixed greedy workload")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from bench_whisper_text import CTX, WIDTH, synthetic_model
    from mlx_audio_amd import whisper_decoding as WD

    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper_serve.py needs a GPU: a time taken elsewhere says nothing")
    if a.steps < 20:
        raise SystemExit("--steps must be at least 20 (the figures are medians)")
    d, model = synthetic_model()
    rt, tok = model._text, WD.special_tokens(d)
    params, bits = WD.pick_params(d, tok, WD.DecodingOptions())
    feats = torch.randn((ROWS, CTX, WIDTH), generator=torch.Generator().manual_seed(ROWS)).cuda()
    prompt = torch.randint(0, 50000, (ROWS, a.position), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
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

    # ---- (a) the static step and the round of 8 step rows, the same position, the same session ------------------------------------------------
    rt.set_audio(feats)
    rt.pick_setup(params, bits)
    rt.forward(prompt.cuda(), False)
    rt.pick()

    def static_step():
        rt.rewind(a.position)
        rt.step()
        rt.pick()

    rows = WD.RowRuntime(rt, ROWS)
    for r in range(ROWS):
        rows.admit(r, feats[r], prompt[r].numpy(), params, bits)
    rows.forward([(r, 0, a.position, 0, -1, 0) for r in range(ROWS)], [(r + 1) * a.position - 1 for r in range(ROWS)])
    rows.pick(list(range(ROWS)))
    items, out, every = [(r, a.position, 1, -1, -1, 0) for r in range(ROWS)], list(range(ROWS)), list(range(ROWS))

    def round_of_steps():
        rows.forward(items, out)
        rows.pick(every)

    static, rnd = timed_pair(static_step, round_of_steps)  # the window state and the row state live side by side on one handle
    emit(dict(case="static_decode_step", B=ROWS, position=a.position, **static))
    emit(dict(case="row_round_8_step_rows", rows=ROWS, position=a.position, extra_us_over_static=round(1e3 * (rnd["ms_median"] - static["ms_median"]), 2), **rnd))
    del rows

    def wall(fn):
        fn()  # warm
        secs, last = [], None
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return statistics.median(secs), min(secs), max(secs), last

    def seconds(w, n):
        return dict(seconds_median=round(w[0], 4), seconds_min=round(w[1], 4), seconds_max=round(w[2], 4), windows_per_s=round(n / w[0], 1))

    def finish():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
                f.write("\n")

    if a.beam:
        # ---- (c) the beam step of 6 windows x K in window mode and the round of 6 beam groups of K rows -----------------------------------------
        K, G = a.beam, BEAM_GROUPS
        if not 1 <= K * G <= 32:
            raise SystemExit("--beam: 6 groups of K rows must fit KK_WHISPER_MAX_ROWS = 32")
        rt.set_audio_groups(feats[:G].contiguous(), K)
        rt.pick_setup(params, bits)
        rt.beam_setup(K, K)
        rt.forward(prompt[:G].repeat_interleave(K, dim=0).cuda(), False)
        rt.pick()

        def static_beam_step():
            rt.rewind(a.position)
            rt.step()
            rt.pick()

        rows = WD.RowRuntime(rt, K * G)
        members = [[g + G * k for k in range(K)] for g in range(G)]  # interleaved physical rows
        for g in range(G):
            rows.admit_group(members[g], True, feats[g], prompt[g].numpy(), params, bits, K)
        every = [r for grp in members for r in grp]
        rows.forward([(r, 0, a.position, 0, -1, 0) for r in every], [(j + 1) * a.position - 1 for j in range(K * G)])
        rows.pick(every)
        items, out = [(r, a.position, 1, -1, -1, 0) for r in every], list(range(K * G))

        def round_of_groups():
            rows.forward(items, out)
            rows.pick(every)

        static, rnd = timed_pair(static_beam_step, round_of_groups)
        emit(dict(case="static_beam_step", windows=G, beam=K, position=a.position, **static))
        emit(dict(case="row_round_beam_groups", groups=G, beam=K, rows=K * G, position=a.position,
                  extra_us_over_static=round(1e3 * (rnd["ms_median"] - static["ms_median"]), 2), **rnd))
        del rows

        # ---- (d) 32 windows of mixed lengths at beam K: static batches of 6 against submit_beam --------------------------------------------------
        counts = [int(c) for c in np.random.default_rng(SEED).integers(4, 201, BEAM_WINDOWS)]
        windows = [feats[i % ROWS] for i in range(BEAM_WINDOWS)]

        def static_beams():
            for g in range(0, BEAM_WINDOWS, G):
                model.beam_search(torch.stack(windows[g:g + G]), language=0, sample_len=max(counts[g:g + G]), beam_size=K)

        def served_beams():
            with model.serve(max_rows=K * G) as s:
                futs = [s.submit_beam(windows[i], language=0, sample_len=counts[i], beam_size=K) for i in range(BEAM_WINDOWS)]
                s.run_until_idle()
                return s.stats, sum(len(f.result(timeout=1).tokens) for f in futs)

        st, sv = wall(static_beams), wall(served_beams)
        stats, served_tokens = sv[3]
        emit(dict(case="mixed_32_windows_beam", beam=K, seed=SEED, token_counts=counts, tokens_total=sum(counts), served_tokens=served_tokens,
                  static_steps=sum(max(counts[g:g + G]) for g in range(0, BEAM_WINDOWS, G)), served_rounds=stats.rounds, served_polls=stats.polls,
                  served_groups=stats.groups, static_batches_of_6=seconds(st, BEAM_WINDOWS), batcher_groups=seconds(sv, BEAM_WINDOWS), repeats=a.repeats,
                  speedup=round(st[0] / sv[0], 3)))
        return finish()

    # ---- (b) 64 windows of mixed lengths: static batches of 8 against the batcher --------------------------------------------------------------
    counts = [int(c) for c in np.random.default_rng(SEED).integers(4, 201, WINDOWS)]
    windows = [feats[i % ROWS] for i in range(WINDOWS)]

    def static_run():
        for g in range(0, WINDOWS, ROWS):
            model.decode(torch.stack(windows[g:g + ROWS]), language=0, sample_len=max(counts[g:g + ROWS]))

    def served_run():
        with model.serve(max_rows=ROWS) as s:
            futs = [s.submit(windows[i], language=0, sample_len=counts[i]) for i in range(WINDOWS)]
            s.run_until_idle()
            return s.stats, sum(len(f.result(timeout=1).tokens) for f in futs)

    st = wall(static_run)
    sv = wall(served_run)
    stats, served_tokens = sv[3]
    emit(dict(case="mixed_64_windows", seed=SEED, token_counts=counts, tokens_total=sum(counts), served_tokens=served_tokens,
              static_steps=sum(max(counts[g:g + ROWS]) for g in range(0, WINDOWS, ROWS)), served_rounds=stats.rounds, served_polls=stats.polls,
              static_batches_of_8=seconds(st, WINDOWS), batcher_8_rows=seconds(sv, WINDOWS), repeats=a.repeats, speedup=round(st[0] / sv[0], 3)))
    finish()


if __name__ == "__main__":
    main()
