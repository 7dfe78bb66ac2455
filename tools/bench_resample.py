"""Time of one row-mode resampler step (resample.RowResampler, kk_resample.hip) at the shape a listen round gives it: 8 rows,
each with the samples of one round of 6 frames (0.48 s) at its source rate, for the ratios 3 / 1 (8 kHz), 3 / 2 (16 kHz) and 80 / 147 (44.1 kHz)
to 24 kHz, and the three mixed in one launch.  Prints one JSON line per case: the stream's time per step (device events around `--steps` steps
after `--warmup`, so host enqueue gaps count where the host is the slower side) and the host's wall-clock per step.

Usage:  python tools/bench_resample.py [--rows 8] [--steps 10000] [--warmup 200] [--format f32] [--out profiles/resample_bench.json]
`--format`: what every row's new samples are stored as -- "f32" (the default: the f32 entry points, as before), "s16le", "mulaw"
or "alaw", decoded inside the same launch; `bytes_up_per_step` is what a listen round uploads for the step.

The kernel alone (the steps above are host-bound) comes from a kernel trace, taken in a run of its own and summarised by this tool:
    rocprofv3 --kernel-trace --stats -d DIR -o rs -- python tools/bench_resample.py --steps 1000 --warmup 50
    python tools/bench_resample.py --steps 1000 --warmup 50 --summarise-trace DIR/rs_results.db --out profiles/resample_kernel_trace.json
The second command needs no GPU: it reads the trace's `kernels` view, takes the launches of resample_rows_kernel in launch order, drops each
case's warm-up launches and prints the median, mean, minimum and maximum duration per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mlx_audio_amd import pcm as PCM  # noqa: E402
from mlx_audio_amd import resample as RS  # noqa: E402

SR, ROUND_SECONDS = 24000, 0.48  # 6 frames of 80 ms


def case(name, rates, rows, steps, warmup, fmt="f32"):
    rs = RS.RowResampler(rows, max(int(r * ROUND_SECONDS) for r in rates))
    n_in = [int(rates[b % len(rates)] * ROUND_SECONDS) for b in range(rows)]
    for b in range(rows):
        if fmt == "f32":
            rs.set_row(b, rates[b % len(rates)], SR)
        else:
            rs.set_row(b, rates[b % len(rates)], SR, in_format=fmt)
    g = torch.Generator().manual_seed(0)
    x = 0.3 * torch.randn((rows, -(-max(n_in) // 16) * 16), generator=g)
    if fmt != "f32":  # the rows' samples in their format, as bytes
        x = torch.from_numpy(np.stack([PCM.encode(r.numpy(), fmt) for r in x]).view(np.uint8))
    x = x.cuda()
    flush = [False] * rows
    n_out = None
    for _ in range(warmup):
        _, n_out = rs.step(x, n_in, flush)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(steps):
        rs.step(x, n_in, flush)
    end.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    rs.close()
    ratios = sorted({RS.ratio(r, SR) for r in rates})
    return dict(case=name, format=fmt, bytes_up_per_step=PCM.bytes_per_sample(fmt) * sum(n_in), rows=rows, ratios=[f"{L}/{M}" for L, M in ratios], taps_per_output=[RS.taps_per_output(L, M) for L, M in ratios],
                samples_in_per_row=n_in, samples_out_per_row=n_out, steps=steps, warmup=warmup,
                stream_us_per_step=round(start.elapsed_time(end) * 1e3 / steps, 2), host_us_per_step=round(host * 1e6 / steps, 2),
                bytes_in_out_per_step=PCM.bytes_per_sample(fmt) * sum(n_in) + 4 * sum(n_out))


CASES = (("8k", [8000]), ("16k", [16000]), ("44k1", [44100]), ("mixed", [8000, 16000, 44100]))


def summarise_trace(db, steps, warmup):
    """Per case: the durations (ns -> us) of the timed launches of resample_rows_kernel in a rocprofv3 kernel-trace database of one run of
    this tool with the same --steps / --warmup."""
    import sqlite3
    import statistics

    rows = sqlite3.connect(db).execute("select grid_x, grid_y, workgroup_x, (end - start) from kernels where name like '%resample_rows_kernel%' "
                                       "order by start").fetchall()
    per = steps + warmup
    if len(rows) != per * len(CASES):
        raise SystemExit(f"{db} holds {len(rows)} launches of resample_rows_kernel, {per * len(CASES)} were expected for --steps {steps} --warmup {warmup}")
    out = []
    for i, (name, _) in enumerate(CASES):
        seg = rows[i * per + warmup : (i + 1) * per]
        d = [r[3] * 1e-3 for r in seg]
        out.append(dict(case=name, launches=len(d), grid=[seg[0][0] // seg[0][2], seg[0][1]], workgroup=seg[0][2],
                        kernel_us_median=round(statistics.median(d), 2), kernel_us_mean=round(sum(d) / len(d), 2), kernel_us_min=round(min(d), 2),
                        kernel_us_max=round(max(d), 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--format", default="f32", choices=PCM.FORMATS)
    ap.add_argument("--summarise-trace", default=None, metavar="DB")
    a = ap.parse_args()
    if a.summarise_trace:
        results = summarise_trace(a.summarise_trace, a.steps, a.warmup)
        for r in results:
            print(json.dumps(r))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(source="rocprofv3 --kernel-trace --stats, a run of its own", steps=a.steps, warmup=a.warmup, results=results), f, indent=1)
                f.write("\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a GPU: a time taken elsewhere says nothing")
    results = [case(name, rates, a.rows, a.steps, a.warmup, a.format)
               for name, rates in CASES]
    for r in results:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
