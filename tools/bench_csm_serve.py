"""CSM-1B serving throughput on a mixed-length workload: static batches (`generate_batch`, groups of --batch in arrival order, every group runs
until its longest stream is done) against continuous batching (`csm_serve.CSMBatcher`: a finished stream's row goes to the next request).
python tools/bench_csm_serve.py [--mode both|static|continuous] [--requests 32] [--batch 8] [--weights bfloat16] [--max-seq-len 512] [--seed 0]
Synthetic weights as tools/bench_csm.py uses; stream lengths are IMPOSED (EOS ignored) and, like the prompt lengths, drawn with --seed from
fixed lists; all requests are queued at time 0; no codec (audio = 80 ms per frame).  Prints one JSON line and writes it to
profiles/csm_serve_bench.json: audio-seconds per wall-second of both modes, their ratio and the ratio the lengths alone allow (frame steps
of the static plan / of a FIFO row schedule, computed on the host), the row occupancy (live row-frames / computed row-frames), and the mean
cost of an admission and of a cache shift (a second, profiled continuous run: one sync around each).  --max-seq-len is small by default so
that the session passes the end of the cache and down-shifts happen.
--prefix N: instead, the same stream lengths with every request's prompt = one shared N-frame voice prefix (text + audio + EOS frames) followed by
its own 16-48 text frames, continuous batching only, admitted plain (the whole prompt per request) / on the prefix (`submit(prefix=)`) / plain
again; per run wall, audio-s/s, frame steps and (a second, profiled run) the mean admission ms.  Written to profiles/csm_serve_prefix_bench.json.
--stream-chunk N: instead, continuous batching WITH the codec (synthetic mimi_202407 weights), the same workload twice: plain `submit` (one
offline Mimi.decode per finished stream; time to first audio = submit -> result) and `submit_stream` in chunks of N frames (time to first
audio = submit -> first chunk); p50 / p95 of both over the requests, audio-s/s of both, and the cost of one row-mode decode step at --batch rows
against a Mimi.decode_step of the same batch and F.  Written to profiles/csm_serve_stream_bench.json.
--sessions N --turns K: instead, N dialogues of K turns (24 text frames and 25 imposed frames per turn) through one batcher of N rows, turn k of
all dialogues queued together: as sessions (`submit(session=)`: a turn is admitted on the K / V captured at the end of the one before) / with
every turn resubmitted as a plain request whose `prompt` is the full history frames (what a caller does without sessions, minus Mimi.encode) /
as sessions again; per run wall, audio-s/s and (a second, profiled run) the mean admission ms BY TURN NUMBER.  Written to
profiles/csm_serve_session_bench.json.
--overlap [--lanes N]: instead, the mixed workload three times in one process: continuous / with `overlap_admission=True` (every request prefilled in
a lane on a side stream and committed by one copy) / continuous again; per run wall, audio-s/s, occupancy and (a second, profiled run) the mean
stall of the batch's stream per admission -- the admission itself, or the commit --, the lanes' device time per prefill, and the frame step's time
while a prefill was in flight beside its time while none was.  Written to profiles/csm_serve_overlap_bench.json.
--stream-chunk N --abandon FRACTION: instead, the streamed workload (with the codec) three times in one process: every stream left to run to its
limit -- what happens to a stream whose listener has gone when nothing can stop it -- / a seeded FRACTION of the requests interrupted
(`CSMAudioStream.interrupt(played_frames=)`) once a seeded number of their chunks has come out / left to run again; per run finished requests per
second, the mean submit -> first audio of the requests that were queued behind a full batch, and the occupancy.  Written to
profiles/csm_serve_interrupt_bench.json.
--listen K: instead, the mixed workload (with the codec's encoder, synthetic mimi_202407 weights) with K session listeners that are each fed a 5 s
clip in 80 ms slices, one slice per scheduling round, while the requests run, against the same workload with `listen_rows=0`: finished requests
per second of both (untimed rounds), the scheduling round's time with and without a listen round in it (a second run, one sync around each
round), and the time from `end()` to its result against `sess.hear(segment)` with the whole-clip `Mimi.encode`.  Written to
profiles/csm_serve_listen_bench.json.
--listen K --vad: the same K listeners made with `vad=` over 5 s clips with a second of near-silence in front of and behind 3 s of
noise speech, against the same clips heard by plain listeners: requests per second and the scheduling round's time of both, and the detector
step's device time (events around `RowVad.step`) for 8 rows of 16 new 720-sample frames and for one 30 s clip, beside the time a float4 copy
of the same bytes takes at the part's measured 6.29 TB/s.  Recorded in profiles/csm_vad_bench.json.
--listen K --vad --continuous: K always-open microphones, each fed three such clips back to back on ONE listener and each
utterance ended with its transcript when its endpoint resolves, against the one-shot VAD listeners over one clip: requests per second, the
scheduling round's time, the library calls per listen round of both, the time from `end()` to the result, and the device time of one ring
detector step and of the two ring copies at a round's size.  Recorded in profiles/csm_continuous_bench.json."""
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
from mlx_audio_amd.sesame import Model, make_sampler  # noqa: E402

PROMPTS = [32, 48, 64, 96]
LENGTHS = [25, 30, 40, 50, 60, 90, 125, 250]

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="both", choices=["both", "static", "continuous"])
ap.add_argument("--requests", type=int, default=32)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--weights", default="bfloat16", choices=["float32", "bfloat16"])
ap.add_argument("--max-seq-len", type=int, default=512)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--prefix", type=int, default=0, help="frames of a voice prefix shared by every request (0: the static / continuous comparison)")
ap.add_argument("--stream-chunk", type=int, default=0, help="frames per audio chunk: time to first audio of submit_stream against plain submit")
ap.add_argument("--abandon", type=float, default=0.0, help="with --stream-chunk: share of the requests whose listener leaves (interrupted against left to run)")
ap.add_argument("--sessions", type=int, default=0, help="dialogues run as sessions against full-history resubmission (with --turns)")
ap.add_argument("--turns", type=int, default=4)
ap.add_argument("--overlap", action="store_true", help="continuous batching with admissions prefilled on a side stream against plain continuous batching")
ap.add_argument("--lanes", type=int, default=1, help="prefill lanes of --overlap")
ap.add_argument("--listen", type=int, default=0, help="listeners fed a 5 s clip in 80 ms slices beside the mixed workload, against none")
ap.add_argument("--listen-chunk", type=int, default=6, help="listen_chunk_frames of --listen")
ap.add_argument("--vad", action="store_true", help="with --listen: listeners with a voice-activity detector against plain ones, and the detector step's time")
ap.add_argument("--continuous", action="store_true", help="with --listen K --vad: always-open microphones fed three clips back to back, against one-shot VAD listeners")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.out is None:
    name = "csm_continuous_bench.json" if a.listen and a.vad and a.continuous else "csm_vad_bench.json" if a.listen and a.vad else "csm_serve_listen_bench.json" if a.listen else "csm_serve_overlap_bench.json" if a.overlap else "csm_serve_session_bench.json" if a.sessions else "csm_serve_interrupt_bench.json" if a.abandon else "csm_serve_stream_bench.json" if a.stream_chunk else "csm_serve_prefix_bench.json" if a.prefix else "csm_serve_bench.json"
    a.out = os.path.join(ROOT, "profiles", name)

cfg = dict(P.csm_config(), max_seq_len=a.max_seq_len)
mimi = None
if a.stream_chunk or a.listen:
    from mlx_audio_amd.mimi import Mimi, MimiConfig

    mcfg = P.mimi_config(cfg["audio_num_codebooks"])
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 0, encode=True) if a.listen else P.mimi_synth_checkpoint(mcfg, 0))
loop = Model(cfg, mimi=mimi, weights=P.csm_synth_checkpoint(cfg, 0), weight_dtype=a.weights)
n, B = cfg["audio_num_codebooks"], a.batch
rng = np.random.default_rng(a.seed)
plen = rng.choice(PROMPTS, a.requests).tolist()
flen = rng.choice(LENGTHS, a.requests).tolist()
prompts = []
for L in plen:
    tok, msk = np.zeros((L, n + 1), np.int32), np.zeros((L, n + 1), np.float32)
    tok[:, -1], msk[:, -1] = rng.integers(0, cfg["text_vocab_size"], L), 1
    prompts.append((tok, msk))
sampler = make_sampler(temp=0.9, top_k=50)
audio_s = 0.08 * sum(flen)
groups = [list(range(i, min(i + B, a.requests))) for i in range(0, a.requests, B)]


def fifo_steps():
    """frame steps of a FIFO row schedule on the lengths alone (a stream of f frames holds its row for f - 1 single-token steps)"""
    rows, queue, steps, live_rf = [0] * B, [f - 1 for f in flen], 0, 0
    while queue or any(rows):
        for r in range(B):
            if rows[r] == 0 and queue:
                rows[r] = queue.pop(0)
        live = sum(1 for r in rows if r > 0)
        if live == 0:
            break
        steps, live_rf, rows = steps + 1, live_rf + live, [max(0, r - 1) for r in rows]
    return steps, live_rf


def run_static():
    torch.cuda.synchronize()
    t = time.perf_counter()
    for g in groups:
        loop.generate_batch([prompts[i] for i in g], max_audio_length_ms=80 * max(flen[i] for i in g), sampler=sampler, seed=a.seed, stop_on_eos=False,
                            decode=False, rng="device")
    torch.cuda.synchronize()
    return time.perf_counter() - t


def run_continuous(profile, **kw):
    bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, decode=False, profile=profile, **kw)
    torch.cuda.synchronize()
    t = time.perf_counter()
    futs = [bat.submit(None, None, prompt=prompts[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
    bat.run_until_idle()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert [f.result(timeout=0).frames for f in futs] == flen
    bat.close()
    return dt, bat


def bench_overlap():
    def both(overlap):
        kw = dict(overlap_admission=True, prefill_lanes=a.lanes) if overlap else {}
        dt, bat = run_continuous(False, **kw)
        st = bat.stats
        _, prof = run_continuous(True, **kw)
        ps = prof.stats
        n = max(1, ps["admissions"])
        r = {"wall_s": dt, "xrt": audio_s / dt, "occupancy": bat.occupancy, "frame_steps": st["frames"], "admissions": st["admissions"],
             "overlapped_admissions": st["overlapped_admissions"], "shifts_down": st["shifts_down"], "shifts_up": st["shifts_up"],
             "main_stream_stall_ms_per_admission": 1e3 * (ps["commit_seconds"] if overlap else ps["admit_seconds"]) / n,
             "shift_ms_mean": 1e3 * ps["shift_seconds"] / max(1, ps["shifts"]), "profiled_wall_note": "stall, shift, prefill and frame-step times are of the profiled run"}
        if overlap:
            r["prefill_seconds"] = ps["prefill_seconds"]
            r["prefill_ms_mean"] = 1e3 * ps["prefill_seconds"] / n
            r["frame_step_ms"] = {"prefill_in_flight": 1e3 * ps["frame_seconds_prefill_in_flight"] / max(1, ps["frames_prefill_in_flight"]),
                                  "frames_prefill_in_flight": ps["frames_prefill_in_flight"],
                                  "no_prefill": 1e3 * ps["frame_seconds_no_prefill"] / max(1, ps["frames_no_prefill"]),
                                  "frames_no_prefill": ps["frames_no_prefill"]}
        return r

    run_continuous(False), run_continuous(False, overlap_admission=True, prefill_lanes=a.lanes)  # warm-up: kernel loading, workspaces, graph capture
    cont_steps, cont_rf = fifo_steps()
    res = {"metric": "CSM-1B serving, admissions prefilled on a side stream vs on the batch's stream, " + a.weights, "requests": a.requests, "batch": B,
           "lanes": a.lanes, "max_seq_len": a.max_seq_len, "prompt_frames": plen, "stream_frames": flen, "audio_s": audio_s,
           "ideal_continuous_steps": cont_steps, "order": ["continuous_first", "overlapped", "continuous_last"],
           "data": "synthetic (random-init CSM-1B weights, random text prompts, imposed stream lengths, device uniforms, no codec)"}
    res["continuous_first"], res["overlapped"], res["continuous_last"] = both(False), both(True), both(False)
    plain = [res["continuous_first"]["xrt"], res["continuous_last"]["xrt"]]
    res["value"] = res["overlapped"]["xrt"] / (0.5 * sum(plain))
    res["value_is"] = "overlapped / continuous audio-sec/sec (continuous: mean of the two runs; they differ by %.3f xRT)" % abs(plain[0] - plain[1])
    return res


def bench_listen():
    from mlx_audio_amd.sesame import Segment

    K, spf = a.listen, 1920
    clips = [(0.3 * rng.standard_normal(5 * 24000)).astype(np.float32) for _ in range(K)]
    if a.vad:  # a second of near-silence, 3 s of speech, a second of near-silence: the detector drops the first and ends within the last
        for c in clips:
            c[:24000] *= 0.01
            c[4 * 24000 :] *= 0.01
    heard = rng.integers(0, cfg["text_vocab_size"], 12).tolist()

    def run(k, timed, vad=None):
        """The workload beside k listeners; timed: one sync around every scheduling round (its time booked by whether a listen round ran)."""
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, decode=False, listen_rows=k,
                         listen_chunk_frames=a.listen_chunk)
        ls = [bat.session().listen(1, vad=vad) for _ in range(k)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        futs = [bat.submit(None, None, prompt=prompts[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
        book = {True: [0, 0.0], False: [0, 0.0]}
        fed, ends, t_end, lat = 0, [], None, []
        while True:
            if k and fed < clips[0].shape[0]:
                for lis, c in zip(ls, clips):
                    lis.feed(c[fed : fed + spf])
                fed += spf
                if fed >= clips[0].shape[0]:  # the speaker stops: the transcript arrives with the end
                    t_end = time.perf_counter()
                    ends = [lis.end(heard) for lis in ls]
            before = (bat.stats["frames"], bat.stats.get("listen_rounds", 0))
            if timed:
                torch.cuda.synchronize()
                t = time.perf_counter()
            more = bat.step()
            if timed:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                if bat.stats["frames"] > before[0]:  # (rounds that ran a frame step)
                    b = book[bat.stats.get("listen_rounds", 0) > before[1]]
                    b[0], b[1] = b[0] + 1, b[1] + dt
            for f in [f for f in ends if f.done()]:
                ends.remove(f)
                lat.append(time.perf_counter() - t_end)
            if not more and not bat._queue and not ends and (not k or fed >= clips[0].shape[0]):
                break
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert [f.result(timeout=0).frames for f in futs] == flen
        st = dict(bat.stats)
        bat.close()
        r = {"wall_s": wall, "requests_per_s": a.requests / wall, "frame_steps": st["frames"], "listen_rounds": st.get("listen_rounds", 0),
             "listen_frames": st.get("listen_frames", 0)}
        if k:
            r["end_to_result_ms"] = {"mean": 1e3 * float(np.mean(lat)), "max": 1e3 * float(np.max(lat))}
        if timed:
            r["round_ms"] = {"with_listen_round": 1e3 * book[True][1] / max(1, book[True][0]), "rounds_with": book[True][0],
                             "without_listen_round": 1e3 * book[False][1] / max(1, book[False][0]), "rounds_without": book[False][0]}
        return r

    def hear_ms():
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, decode=False)
        out = []
        for c in clips + clips[:1]:
            sess = bat.session()
            torch.cuda.synchronize()
            t = time.perf_counter()
            sess.hear(Segment(speaker=1, text=heard, audio=c))  # whole-clip Mimi.encode on the caller's thread
            out.append(1e3 * (time.perf_counter() - t))
        bat.close()
        return out[1:]  # (the first call sizes the workspace)

    if a.vad and a.continuous:
        return bench_continuous(run, clips, heard)
    if a.vad:
        return bench_vad(run)
    run(0, False), run(K, False)  # warm-up: kernel loading, workspaces, graph capture
    res = {"metric": "CSM-1B serving with live listeners (row-mode streaming Mimi encoder) vs without, " + a.weights, "requests": a.requests, "batch": B,
           "listeners": K, "listen_chunk_frames": a.listen_chunk, "clip_seconds": 5.0, "slice_ms": 80, "order": ["plain_first", "listening", "plain_last"],
           "data": "synthetic (random-init CSM-1B and mimi_202407 weights, random prompts and clips, imposed stream lengths, device uniforms)"}
    res["plain_first"], res["listening"], res["plain_last"] = run(0, False), run(K, False), run(0, False)
    res["listening_timed"], res["plain_timed"] = run(K, True), run(0, True)
    h = hear_ms()
    res["hear_whole_clip_ms"] = {"mean": float(np.mean(h)), "max": float(np.max(h))}
    plain = [res["plain_first"]["requests_per_s"], res["plain_last"]["requests_per_s"]]
    res["value"] = res["listening"]["requests_per_s"] / (0.5 * sum(plain))
    res["value_is"] = "requests/s with listeners / without (without: mean of the two runs; they differ by %.3f)" % abs(plain[0] - plain[1])
    return res


def vad_step_us():
    """Device time of one `RowVad.step` (events around it, so the launch is in it): 8 rows of 16 new 720-sample frames per step, and one
    row's 30 s clip in one step.  Threshold 0: every frame is speech and no row ends."""
    from mlx_audio_amd.vad import RowVad

    fl, reps, out = 720, 60, {}
    hbm = 6.29e12  # bytes/s of a float4 copy on the part (measured; the spec is 8 TB/s)

    def series(rv, x, rows, new):
        for b in range(rows):
            rv.set_row(b, fl, 0.0, 50)
        ev = []
        for i in range(x.shape[1] // new):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rv.step(x, [new * (i + 1)] * rows)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [1e3 * e0.elapsed_time(e1) for e0, e1 in ev]

    for name, rows, new, steps in (("rows8_frames16", 8, 16 * fl, reps), ("one_clip_30s", 1, 30 * 24000, 1)):
        rv = RowVad(rows)
        x = (0.3 * torch.randn((rows, new * steps), device="cuda")).contiguous()
        t = []
        for _ in range(1 if steps > 1 else reps):
            series(rv, x, rows, new)  # (warm, and for the clip: one step per series)
            t += series(rv, x, rows, new)
        nbytes = 4 * rows * new
        out[name] = {"rows": rows, "new_frames_per_row": new // fl, "bytes_read": nbytes, "steps_timed": len(t), "median_us": float(np.median(t)),
                     "min_us": float(np.min(t)), "max_us": float(np.max(t)), "float4_copy_us_at_6.29TBps": 1e6 * nbytes / hbm}
        rv.close()
    return out


class Calls:
    """Counts the library calls a listen round makes (each is one launch, the encoder step its own fixed series): patched at the classes."""

    def __init__(self):
        from mlx_audio_amd import mimi as MI, pcm as PC, resample as RSM, ring as RG, vad as VD

        self.n, self._undo = {}, []
        for owner, name in ((RSM.RowResampler, "step"), (PC.RowConverter, "convert"), (VD.RowVad, "step"), (VD.RingVad, "step"), (RG, "write_rows"),
                            (RG, "read_rows"), (MI.MimiRowEncoder, "step")):
            self._wrap(owner, name, f"{getattr(owner, '__name__', 'ring').split('.')[-1]}.{name}")

    def _wrap(self, owner, name, key):
        fn = getattr(owner, name)

        def counted(*args, **kw):
            self.n[key] = self.n.get(key, 0) + 1
            return fn(*args, **kw)

        setattr(owner, name, counted)
        self._undo.append((owner, name, fn))

    def close(self):
        for owner, name, fn in self._undo:
            setattr(owner, name, fn)
        return dict(self.n)


def ring_step_us():
    """Device time (events around each call, so the launch is in it) of one `RingVad.step`, one `ring.write_rows` and one `ring.read_rows`
    at a round's size: 8 rows, 16 new 720-sample frames per row and step, a ring of 30 s; the read is an encode step's 6 codec frames."""
    from mlx_audio_amd import ring as RG
    from mlx_audio_amd.vad import RingVad

    fl, rows, new, reps, ring_len = 720, 8, 16 * 720, 60, 30 * 24000
    x = (0.3 * torch.randn((rows, ring_len), device="cuda")).contiguous()
    src = (0.3 * torch.randn((rows, new), device="cuda")).contiguous()
    dst = torch.zeros((rows, 6 * 1920), device="cuda")
    rv = RingVad(rows)
    out = {}

    def series(fn):
        ev = []
        for i in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [1e3 * e0.elapsed_time(e1) for e0, e1 in ev]

    def detector(i):
        if i == 0:
            for b in range(rows):
                rv.set_row(b, fl, 0.0, 50, 1 << 40, ring_len)
        rv.step(x, [new * (i + 1)] * rows, [0] * rows)

    cases = (("ring_vad_step_rows8_frames16", detector, 4 * rows * new),
             ("ring_write_rows8_11520", lambda i: RG.write_rows(src, x, ring_len, [new * i + 4 * b for b in range(rows)], [new] * rows), 8 * rows * new),
             ("ring_read_rows8_11520", lambda i: RG.read_rows(x, ring_len, dst, [new * i + 3 * b for b in range(rows)], [6 * 1920 - 100] * rows, [6 * 1920] * rows),
              8 * rows * 6 * 1920))
    for name, fn, nbytes in cases:
        series(fn)  # warm
        t = series(fn)
        out[name] = {"rows": rows, "bytes_moved": nbytes, "steps_timed": len(t), "median_us": float(np.median(t)), "min_us": float(np.min(t)),
                     "max_us": float(np.max(t)), "float4_copy_us_at_6.29TBps": 1e6 * nbytes / 6.29e12}
    rv.close()
    return out


def bench_continuous(run, clips, heard):
    from mlx_audio_amd.vad import VadConfig

    K, vcfg, spf, reps = a.listen, VadConfig(silence_ms=300), 1920, 3
    streams = [np.concatenate([c] * reps) for c in clips]  # three utterances per microphone, back to back

    def run_cont(timed):
        """The workload beside K always-open microphones; every utterance is ended with its transcript once its endpoint has resolved."""
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, decode=False, listen_rows=K,
                         listen_chunk_frames=a.listen_chunk)
        ls = [bat.session().listen(1, vad=vcfg, continuous=True) for _ in range(K)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        futs = [bat.submit(None, None, prompt=prompts[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
        book = {True: [0, 0.0], False: [0, 0.0]}
        fed, open_utts, ends, lat, done = 0, [], [], [], 0
        while True:
            if fed < streams[0].shape[0]:
                for lis, c in zip(ls, streams):
                    lis.feed(c[fed : fed + spf])
                fed += spf
                if fed >= streams[0].shape[0]:
                    for lis in ls:
                        lis.close()
            before = (bat.stats["frames"], bat.stats.get("listen_rounds", 0))
            if timed:
                torch.cuda.synchronize()
                t = time.perf_counter()
            more = bat.step()
            if timed:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                if bat.stats["frames"] > before[0]:
                    b = book[bat.stats.get("listen_rounds", 0) > before[1]]
                    b[0], b[1] = b[0] + 1, b[1] + dt
            for lis in ls:
                while True:
                    try:
                        u = lis.next_utterance(0)
                    except Exception:  # noqa: BLE001  (queue.Empty)
                        break
                    if u is None:
                        break
                    open_utts.append(u)
            for u in [u for u in open_utts if u.endpoint.done()]:  # the speaker has stopped: the transcript arrives with the end
                open_utts.remove(u)
                ends.append((u.end(heard), time.perf_counter()))
            for f, t_end in [e for e in ends if e[0].done()]:
                ends.remove((f, t_end))
                f.result(timeout=0)
                lat.append(time.perf_counter() - t_end)
                done += 1
            if not more and not bat._queue and not ends and not open_utts and fed >= streams[0].shape[0]:
                break
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        assert [f.result(timeout=0).frames for f in futs] == flen and done == reps * K, (done, reps * K)
        st = dict(bat.stats)
        bat.close()
        r = {"wall_s": wall, "requests_per_s": a.requests / wall, "frame_steps": st["frames"], "listen_rounds": st.get("listen_rounds", 0),
             "listen_frames": st.get("listen_frames", 0), "utterances": done,
             "end_to_result_ms": {"mean": 1e3 * float(np.mean(lat)), "max": 1e3 * float(np.max(lat))}}
        if timed:
            r["round_ms"] = {"with_listen_round": 1e3 * book[True][1] / max(1, book[True][0]), "rounds_with": book[True][0],
                             "without_listen_round": 1e3 * book[False][1] / max(1, book[False][0]), "rounds_without": book[False][0]}
        return r

    def counted(fn):
        c = Calls()
        try:
            r = fn()
        finally:
            n = c.close()
        r["library_calls"] = n
        r["library_calls_per_listen_round"] = sum(n.values()) / max(1, r["listen_rounds"])
        return r

    run(K, False, vcfg), run_cont(False)  # warm-up: kernel loading, workspaces, graph capture
    res = {"metric": "CSM-1B serving, always-open microphones (ring + re-arming detector) vs one-shot VAD listeners, " + a.weights, "requests": a.requests,
           "batch": B, "listeners": K, "listen_chunk_frames": a.listen_chunk, "clip_seconds": 5.0, "clips_per_microphone": reps, "slice_ms": 80,
           "vad_config": {"frame_ms": vcfg.frame_ms, "threshold": vcfg.threshold, "silence_ms": vcfg.silence_ms},
           "order": ["vad_first", "continuous", "vad_last"],
           "library_calls_note": "calls of RowResampler.step, RowConverter.convert, RowVad.step, RingVad.step, ring.write_rows, ring.read_rows and "
                                 "MimiRowEncoder.step; the one-shot path's torch slice copies (one per listener and upload, one per listener and encode "
                                 "step) are not among them, the continuous path has none",
           "data": "synthetic (random-init CSM-1B and mimi_202407 weights, random prompts, noise clips, imposed stream lengths, device uniforms)"}
    res["vad_first"], res["continuous"], res["vad_last"] = run(K, False, vcfg), run_cont(False), run(K, False, vcfg)
    res["continuous_timed"], res["vad_timed"] = run_cont(True), run(K, True, vcfg)
    res["continuous_counted"], res["vad_counted"] = counted(lambda: run_cont(False)), counted(lambda: run(K, False, vcfg))
    res["ring_step_us"] = ring_step_us()
    one = [res["vad_first"]["requests_per_s"], res["vad_last"]["requests_per_s"]]
    res["value"] = res["continuous"]["requests_per_s"] / (0.5 * sum(one))
    res["value_is"] = "requests/s with always-open microphones (3 utterances each) / with one-shot VAD listeners (1 utterance each; mean of the two runs; they differ by %.3f)" % abs(one[0] - one[1])
    return res


def bench_vad(run):
    from mlx_audio_amd.vad import VadConfig

    K, vcfg = a.listen, VadConfig(silence_ms=300)
    run(K, False), run(K, False, vcfg)  # warm-up: kernel loading, workspaces, graph capture
    res = {"metric": "CSM-1B serving, listeners with a voice-activity detector vs plain listeners, " + a.weights, "requests": a.requests, "batch": B,
           "listeners": K, "listen_chunk_frames": a.listen_chunk, "clip_seconds": 5.0, "speech_seconds": [1.0, 4.0], "slice_ms": 80,
           "vad_config": {"frame_ms": vcfg.frame_ms, "threshold": vcfg.threshold, "silence_ms": vcfg.silence_ms}, "order": ["plain_first", "vad", "plain_last"],
           "data": "synthetic (random-init CSM-1B and mimi_202407 weights, random prompts, noise clips, imposed stream lengths, device uniforms)"}
    res["plain_first"], res["vad"], res["plain_last"] = run(K, False), run(K, False, vcfg), run(K, False)
    res["vad_timed"], res["plain_timed"] = run(K, True, vcfg), run(K, True)
    res["vad_step_us"] = vad_step_us()
    plain = [res["plain_first"]["requests_per_s"], res["plain_last"]["requests_per_s"]]
    res["value"] = res["vad"]["requests_per_s"] / (0.5 * sum(plain))
    res["value_is"] = "requests/s with VAD listeners / with plain listeners (plain: mean of the two runs; they differ by %.3f)" % abs(plain[0] - plain[1])
    return res


def bench_prefix():
    from mlx_audio_amd.sesame import VoicePrefix

    N, nt = a.prefix, min(32, a.prefix // 4)
    ptok, pmsk = np.zeros((N, n + 1), np.int32), np.zeros((N, n + 1), np.float32)
    ptok[:nt, -1], pmsk[:nt, -1] = rng.integers(0, cfg["text_vocab_size"], nt), 1
    ptok[nt:N - 1, :n] = rng.integers(0, cfg["audio_vocab_size"], (N - 1 - nt, n))  # the clip's frames, then the all-zero EOS frame
    pmsk[nt:, :n] = 1
    texts = [rng.integers(0, cfg["text_vocab_size"], int(L)).tolist() for L in rng.integers(16, 49, a.requests)]
    vp = VoicePrefix(prefix=loop.model.make_prefix(ptok, pmsk), tokens=ptok, mask=pmsk, length=N, root=loop.model.weights_root())
    whole = [tuple(np.concatenate([p, t], 0) for p, t in zip((ptok, pmsk), loop._tokenize_text_segment(x, 0))) for x in texts]

    def run(prefixed, profile):
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, decode=False, profile=profile)
        torch.cuda.synchronize()
        t = time.perf_counter()
        if prefixed:
            futs = [bat.submit(prefix=vp, text=texts[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
        else:
            futs = [bat.submit(None, None, prompt=whole[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
        bat.run_until_idle()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert [f.result(timeout=0).frames for f in futs] == flen
        return dt, bat.stats

    def both(prefixed):
        dt, st = run(prefixed, False)
        _, ps = run(prefixed, True)
        return {"wall_s": dt, "xrt": audio_s / dt, "frame_steps": st["frames"], "admissions": st["admissions"],
                "prefixed_admissions": st["prefixed_admissions"], "admit_ms_mean": 1e3 * ps["admit_seconds"] / max(1, ps["admissions"]),
                "shifts_down": st["shifts_down"], "shifts_up": st["shifts_up"]}

    run(False, False), run(True, False)  # warm-up: kernel loading, workspaces, graph capture
    res = {"metric": "CSM-1B serving on a shared voice prefix, plain vs prefixed admission, " + a.weights, "requests": a.requests, "batch": B,
           "max_seq_len": a.max_seq_len, "prefix_frames": N, "prefix_bytes": vp.prefix.nbytes, "text_frames": [len(x) for x in texts],
           "stream_frames": flen, "audio_s": audio_s, "order": ["plain_first", "prefixed", "plain_last"],
           "data": "synthetic (random-init CSM-1B weights, random prefix and text frames, imposed stream lengths, device uniforms, no codec)"}
    res["plain_first"], res["prefixed"], res["plain_last"] = both(False), both(True), both(False)
    plain = [res["plain_first"]["admit_ms_mean"], res["plain_last"]["admit_ms_mean"]]
    res["value"] = res["prefixed"]["admit_ms_mean"] / (0.5 * sum(plain))
    res["value_is"] = "prefixed / plain mean admission ms (plain: mean of the two runs; their spread %.3f ms)" % abs(plain[0] - plain[1])
    return res


def bench_stream():
    N = a.stream_chunk

    def pct(v, q):
        return float(np.percentile(np.asarray(v, np.float64), q))

    def run(streamed):
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, stream_chunk_frames=N if streamed else None,
                         stream_max_frames=max(LENGTHS))
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn = bat.submit_stream if streamed else bat.submit
        hs = [fn(None, None, prompt=prompts[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
        bat.run_until_idle()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        res = [h.result(timeout=0) for h in hs]
        assert [r.frames for r in res] == flen
        first = [h.first_audio_seconds for h in hs] if streamed else [r.processing_time_seconds for r in res]
        st = dict(bat.stats)
        bat.close()
        return {"wall_s": dt, "xrt": audio_s / dt, "first_audio_s_p50": pct(first, 50), "first_audio_s_p95": pct(first, 95), "frame_steps": st["frames"],
                "polls": st["polls"], "chunks": st.get("chunks", 0), "chunk_rounds": st.get("chunk_rounds", 0)}

    def step_ms(fn, reps=40):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / reps

    run(False), run(True)  # warm-up: kernel loading, workspaces, graph capture
    res = {"metric": "CSM-1B serving with the codec: time to first audio, plain submit vs submit_stream, " + a.weights, "requests": a.requests, "batch": B,
           "max_seq_len": a.max_seq_len, "chunk_frames": N, "stream_frames": flen, "audio_s": audio_s, "order": ["plain_first", "streamed", "plain_last"],
           "note": "all requests are queued at time 0, so a request's time to first audio includes its wait for a row",
           "data": "synthetic (random-init CSM-1B and mimi_202407 weights, random text prompts, imposed stream lengths, device uniforms)"}
    res["plain_first"], res["streamed"], res["plain_last"] = run(False), run(True), run(False)
    codes = torch.randint(0, 2048, (B, n, N), dtype=torch.int32, device="cuda")
    dec = mimi.row_decoder(B, 64 * N, N)
    rows_ms = step_ms(lambda: dec.step(codes, [True] * B))  # (41 steps of N frames: inside the 64 N the decoder was made for)
    dec.close()
    mimi.close_stream()
    solo_ms = step_ms(lambda: mimi.decode_step(codes, max_frames=64 * N))
    mimi.close_stream()
    res["decode_step_ms"] = {"rows_mode": rows_ms, "decode_step": solo_ms, "batch": B, "frames": N}
    plain = 0.5 * (res["plain_first"]["xrt"] + res["plain_last"]["xrt"])
    res["value"] = res["streamed"]["first_audio_s_p50"] / (0.5 * (res["plain_first"]["first_audio_s_p50"] + res["plain_last"]["first_audio_s_p50"]))
    res["value_is"] = "streamed / plain p50 time to first audio; audio-s/s streamed / plain = %.3f (plain runs differ by %.3f xRT)" % (
        res["streamed"]["xrt"] / plain, abs(res["plain_first"]["xrt"] - res["plain_last"]["xrt"]))
    return res


def bench_abandon():
    N = a.stream_chunk
    pick = np.random.default_rng(a.seed + 1)
    gone = sorted(pick.choice(a.requests, max(1, int(round(a.abandon * a.requests))), replace=False).tolist())
    played = {i: int(pick.integers(1, (flen[i] - 1) // N + 1)) for i in gone}  # chunks that came out before the listener left: fewer than the stream has

    def run(interrupt):
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, stream_chunk_frames=N, stream_max_frames=max(LENGTHS))
        torch.cuda.synchronize()
        t = time.perf_counter()
        hs = [bat.submit_stream(None, None, prompt=prompts[i], max_audio_length_ms=80 * flen[i]) for i in range(a.requests)]
        waiting = dict(played) if interrupt else {}
        while bat.step() or bat._queue:
            for i in [i for i, c in waiting.items() if hs[i]._q.qsize() >= c]:
                hs[i].interrupt(played_frames=waiting.pop(i) * N)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        res = [h.result(timeout=0) for h in hs]
        assert [r.frames for r in res] == [played[i] * N if interrupt and i in played else flen[i] for i in range(a.requests)]
        behind = [hs[i].first_audio_seconds for i in range(B, a.requests)]  # all are queued at time 0: the first B get a row at once
        st, occ = dict(bat.stats), bat.occupancy
        bat.close()
        return {"wall_s": dt, "finished_requests_per_s": a.requests / dt, "first_audio_s_mean_queued_behind_full_batch": float(np.mean(behind)) if behind else None,
                "occupancy": occ, "frame_steps": st["frames"], "polls": st["polls"], "interrupted": st["interrupted"],
                "audio_s_delivered": 0.08 * sum(r.frames for r in res), "audio_s_generated": 0.08 * (st["live_row_frames"] + st["admissions"])}

    run(False), run(True)  # warm-up: kernel loading, workspaces, graph capture
    res = {"metric": "CSM-1B serving with the codec: abandoned streams interrupted vs left to run to their limit, " + a.weights, "requests": a.requests,
           "batch": B, "max_seq_len": a.max_seq_len, "chunk_frames": N, "abandon": a.abandon, "abandoned_requests": gone,
           "played_chunks": [played[i] for i in gone], "stream_frames": flen, "order": ["left_first", "interrupted", "left_last"],
           "note": "all requests are queued at time 0; an interrupt is issued between two scheduling rounds once the stream's played chunks have come out",
           "data": "synthetic (random-init CSM-1B and mimi_202407 weights, random text prompts, imposed stream lengths, device uniforms)"}
    res["left_first"], res["interrupted"], res["left_last"] = run(False), run(True), run(False)
    left = [res["left_first"]["finished_requests_per_s"], res["left_last"]["finished_requests_per_s"]]
    res["value"] = res["interrupted"]["finished_requests_per_s"] / (0.5 * sum(left))
    res["value_is"] = "interrupted / left finished requests per second (left: mean of the two runs; they differ by %.3f requests/s)" % abs(left[0] - left[1])
    return res


def bench_sessions():
    N, K, T, F = a.sessions, a.turns, 24, 25
    texts = [[rng.integers(0, cfg["text_vocab_size"], T).tolist() for _ in range(K)] for _ in range(N)]

    def run(form, profile, histories=None):
        """form "session" or "history"; returns wall, stats, per-turn admission seconds and (session form) every turn's prompt as a plain request"""
        bat = loop.serve(max_batch=N, rng="device", sampler=sampler, seed=a.seed, stop_on_eos=False, decode=False, profile=profile)
        sess = [bat.session() for _ in range(N)] if form == "session" else None
        admit, prompts_of = [], []
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(K):
            before = bat.stats["admit_seconds"]
            if form == "session":
                prompts_of.append([tuple(np.concatenate([h, x], 0) for h, x in zip(s.history, loop._tokenize_text_segment(texts[i][k], 0)))
                                   for i, s in enumerate(sess)])
                futs = [s.submit(texts[i][k], max_audio_length_ms=80 * F, stream_id=i) for i, s in enumerate(sess)]
            else:
                futs = [bat.submit(None, None, prompt=histories[k][i], max_audio_length_ms=80 * F, stream_id=i) for i in range(N)]
            bat.run_until_idle()
            assert [f.result(timeout=0).frames for f in futs] == [F] * N
            admit.append((bat.stats["admit_seconds"] - before) / N)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st = dict(bat.stats)
        for s in sess or []:
            s.close()
        bat.close()
        return dt, st, admit, prompts_of

    _, _, _, histories = run("session", False)  # warm-up; its turns' prompts are what the history form resubmits
    run("history", False, histories)

    def both(form):
        dt, st, _, _ = run(form, False, histories)
        _, _, admit, _ = run(form, True, histories)
        return {"wall_s": dt, "xrt": 0.08 * F * N * K / dt, "frame_steps": st["frames"], "admissions": st["admissions"],
                "session_admissions": st["session_admissions"], "captures": st["captures"], "admit_ms_by_turn": [1e3 * x for x in admit],
                "shifts_down": st["shifts_down"], "shifts_up": st["shifts_up"]}

    res = {"metric": "CSM-1B serving, multi-turn dialogues: sessions vs full-history resubmission, " + a.weights, "sessions": N, "turns": K, "batch": N,
           "max_seq_len": a.max_seq_len, "text_frames_per_turn": T, "frames_per_turn": F, "prompt_frames_by_turn": [int(h[0][0].shape[0]) for h in histories],
           "audio_s": 0.08 * F * N * K, "order": ["session_first", "history", "session_last"],
           "data": "synthetic (random-init CSM-1B weights, random text frames, imposed stream lengths, device uniforms, no codec)"}
    res["session_first"], res["history"], res["session_last"] = both("session"), both("history"), both("session")
    last = [res[k]["admit_ms_by_turn"][-1] for k in ("session_first", "session_last")]
    res["value"] = 0.5 * sum(last) / res["history"]["admit_ms_by_turn"][-1]
    res["value_is"] = "session / history mean admission ms of the last turn (session: mean of the two runs; their spread %.3f ms)" % abs(last[0] - last[1])
    return res


if a.overlap:
    if a.prefix or a.stream_chunk or a.sessions or a.lanes < 1:
        sys.exit("--overlap excludes --prefix / --stream-chunk / --sessions and needs --lanes >= 1")
    out = bench_overlap()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0)

if a.sessions:
    if a.prefix or a.stream_chunk or a.turns < 1 or a.turns * 50 + 25 >= a.max_seq_len:
        sys.exit(f"--sessions excludes --prefix / --stream-chunk and needs turns * 50 + 25 < --max-seq-len {a.max_seq_len}")
    out = bench_sessions()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0)

if a.abandon and not a.stream_chunk:
    sys.exit("--abandon needs --stream-chunk N")

if a.stream_chunk:
    if a.prefix or not 1 <= a.stream_chunk <= min(LENGTHS):
        sys.exit(f"--stream-chunk must be in [1, {min(LENGTHS)}] and excludes --prefix")
    if a.abandon and not (0.0 < a.abandon <= 1.0 and a.stream_chunk < min(LENGTHS)):
        sys.exit(f"--abandon must be in (0, 1] and needs --stream-chunk below {min(LENGTHS)}")
    out = bench_abandon() if a.abandon else bench_stream()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0)

if a.listen:
    out = bench_listen()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0)

if a.prefix:
    if not 8 <= a.prefix < a.max_seq_len - 48 - max(LENGTHS):
        sys.exit(f"--prefix must be in [8, {a.max_seq_len - 48 - max(LENGTHS)}) at --max-seq-len {a.max_seq_len}")
    out = bench_prefix()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0)

static_steps = sum(max(flen[i] for i in g) - 1 for g in groups)
static_rf = sum(sum(flen[i] - 1 for i in g) for g in groups)
cont_steps, cont_rf = fifo_steps()
out = {"metric": "audio-sec/sec (xRT), CSM-1B serving, mixed-length workload, " + a.weights, "requests": a.requests, "batch": B,
       "max_seq_len": a.max_seq_len, "prompt_frames": plen, "stream_frames": flen, "audio_s": audio_s,
       "ideal": {"static_steps": static_steps, "continuous_steps": cont_steps, "ratio": static_steps / cont_steps,
                 "static_occupancy": static_rf / (static_steps * B), "continuous_occupancy": cont_rf / (cont_steps * B)},
       "data": "synthetic (random-init CSM-1B weights, random text prompts, imposed stream lengths, device uniforms, no codec)"}
if a.mode in ("both", "static"):
    run_static()  # warm-up: kernel loading, workspaces, graph capture
    dt = run_static()
    out["static"] = {"wall_s": dt, "xrt": audio_s / dt, "occupancy": static_rf / (static_steps * B)}
if a.mode in ("both", "continuous"):
    run_continuous(False)  # warm-up
    dt, bat = run_continuous(False)
    st = bat.stats
    out["continuous"] = {"wall_s": dt, "xrt": audio_s / dt, "occupancy": bat.occupancy, "frame_steps": st["frames"], "admissions": st["admissions"],
                         "shifts_down": st["shifts_down"], "shifts_up": st["shifts_up"]}
    _, prof = run_continuous(True)
    ps = prof.stats
    out["continuous"].update(admit_ms_mean=1e3 * ps["admit_seconds"] / max(1, ps["admissions"]), shift_ms_mean=1e3 * ps["shift_seconds"] / max(1, ps["shifts"]),
                             shifts_profiled=ps["shifts"])
if "static" in out and "continuous" in out:
    out["value"] = out["continuous"]["xrt"] / out["static"]["xrt"]
    out["value_is"] = "continuous / static audio-sec/sec"
print(json.dumps(out))
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
