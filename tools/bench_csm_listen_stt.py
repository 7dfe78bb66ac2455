"""Times of speech to text at the listening edge of CSM serving (mlx-audio_amd/csm_listen.py, kk_op_log_mel_spans in csrc/kk_whisper.hip)
in ONE process, at the production window (W = 3000 frames, 128 mels) on synthetic weights: the whisper-large-v3-turbo shapes of
tools/bench_whisper_text.py, CSM-1B and mimi_202407 of tools/bench_csm_serve.py.

 (a) `whisper.span_windows` for 8 rows of 2 .. 10 s utterances in a ring at 24 kHz, next to the composition it replaces -- ONE ring read, ONE resampler
     step (its rows set first: every utterance is a new stream), ONE ragged log-mel, ONE `mel_windows`, with the host arithmetic that sizes their three
     intermediate buffers -- sampled in turn, each the median of `--steps` samples of `--inner` calls between two device events.  The two results are
     compared with torch.equal first.
 (b) With a full CSM batch generating (8 streams), K listeners with a detector close their utterances in the same round: the wall time from the
     start of the round that cuts their windows to the last transcript (`sample_len` tokens each; synthetic weights never sample eot), K = 1 and 8,
     `--repeats` runs each.
 (c) The scheduling round of that batch (8 live streams, nobody listening) with `stt=` given but idle next to the same round without `stt=`: wall time
     of `--rounds` rounds between two synchronisations, the two kinds of batcher in turn, `--repeats` runs each.

Usage:  python tools/bench_csm_listen_stt.py [--steps 20] [--warmup 3] [--inner 5] [--repeats 3] [--rounds 150] [--sample-len 24]
                                            [--out profiles/csm_listen_stt_bench.json]"""
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

SR, W, N_MELS, ROWS = 24000, 3000, 128, 8
SECONDS = [2, 3, 4, 5, 6, 7, 8, 10]


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=150)
    ap.add_argument("--sample-len", type=int, default=24)
    ap.add_argument("--only", default="abc", help="which of the three measurements to take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csm_listen_stt_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_csm_listen_stt.py needs a GPU: a time taken elsewhere says nothing")
    from bench_whisper_text import synthetic_model
    from mlx_audio_amd import resample as RS, ring as RING, whisper

    res = {"metric": "CSM serving, listeners' utterances transcribed on a Whisper batch (DESIGN 8d-15)", "window_frames": W, "n_mels": N_MELS,
           "data": "synthetic (random-init whisper-large-v3-turbo shapes with 4 decoder layers, CSM-1B and mimi_202407 weights; noise clips; device uniforms)"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    # ---- (a) one launch pair against the four-launch composition ---------------------------------------------------------------------------------
    if "a" in a.only:
        g = torch.Generator().manual_seed(7)
        ring_len = 30 * SR
        ring = (0.1 * torch.randn((ROWS, ring_len), generator=g)).cuda()
        n = [s * SR for s in SECONDS]
        pos = [2 ** 32 + 100003 * (r + 1) + ring_len - 5000 * r for r in range(ROWS)]  # stream positions above 2^32; some spans wrap
        spans = [whisper.Span(ring[r], ring_len, pos[r], n[r]) for r in range(ROWS)]
        L, M = RS.ratio(SR, 16000)
        rs = RS.RowResampler(ROWS, max(n))

        def fused():
            return whisper.span_windows(spans, W, N_MELS, src_rate=SR)

        def composed():
            x = torch.empty((ROWS, max(n)), dtype=torch.float32, device="cuda")
            RING.read_rows(ring, ring_len, x, pos, n, n)
            for r in range(ROWS):
                rs.set_row(r, SR, 16000)
            y, n16 = rs.step(x, n, [True] * ROWS)
            mel = whisper.log_mel_rows(y, n16, N_MELS, W * 160)
            return whisper.mel_windows([mel[r] for r in range(ROWS)], [0] * ROWS, [W] * ROWS, W)

        same = bool(torch.equal(fused(), composed()))
        for _ in range(a.warmup):
            fused(), composed()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(a.steps):
            for k, fn in enumerate((fused, composed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.inner)
        frames = [min(W, -(-(RS.out_len(k, L, M) + 200) // 160)) for k in n]
        res["a_span_windows"] = {"rows": ROWS, "utterance_seconds": SECONDS, "frames_computed_per_row": frames, "bit_equal_to_composition": same,
                                 "span_windows_ms": spread(ms[0]), "composition_ms": spread(ms[1]),
                                 "composition_is": "ring.read_rows + 8 x set_row + RowResampler.step + log_mel_rows (padding 480000) + mel_windows, buffers sized on the host",
                                 "speedup_median": round(statistics.median(ms[1]) / statistics.median(ms[0]), 3), "steps": a.steps, "inner": a.inner}
        rs.close()
        del ring
        print(json.dumps(res["a_span_windows"]), flush=True)
        save()
    if "b" not in a.only and "c" not in a.only:
        return

    # ---- the two models -------------------------------------------------------------------------------------------------------------------------
    import mlx_audio_amd.params as P
    from mlx_audio_amd.mimi import Mimi, MimiConfig
    from mlx_audio_amd.sesame import Model, make_sampler
    from mlx_audio_amd.vad import VadConfig

    d, wm = synthetic_model()
    cfg = dict(P.csm_config(), max_seq_len=1024)
    mcfg = P.mimi_config(cfg["audio_num_codebooks"])
    mimi = Mimi(MimiConfig.from_dict(mcfg), P.mimi_synth_checkpoint(mcfg, 0, encode=True))
    loop = Model(cfg, mimi=mimi, weights=P.csm_synth_checkpoint(cfg, 0), weight_dtype="bfloat16")
    ncb, B = cfg["audio_num_codebooks"], 8
    rng = np.random.default_rng(0)
    sampler = make_sampler(temp=0.9, top_k=50)

    def prompt(Lp=48):
        tok, msk = np.zeros((Lp, ncb + 1), np.int32), np.zeros((Lp, ncb + 1), np.float32)
        tok[:, -1], msk[:, -1] = rng.integers(0, cfg["text_vocab_size"], Lp), 1
        return tok, msk

    def batcher(frames, **kw):
        bat = loop.serve(max_batch=B, rng="device", sampler=sampler, seed=0, stop_on_eos=False, decode=False, **kw)
        futs = [bat.submit(None, None, prompt=prompt(), max_audio_length_ms=80 * frames) for _ in range(B)]
        for _ in range(12):  # admissions, graph capture, the first polls
            bat.step()
        return bat, futs

    # ---- (c) the scheduling round with an idle stt next to the round without ---------------------------------------------------------------------------
    if "c" in a.only:
        ms = {"without_stt": [], "with_idle_stt": []}
        for rep in range(a.repeats + 1):  # (the first pair is the warm-up)
            for kind in ("without_stt", "with_idle_stt"):
                stt = wm.serve(max_rows=8) if kind == "with_idle_stt" else None
                bat, futs = batcher(a.rounds + 40, **({"stt": stt, "listen_rows": 8} if stt is not None else {"listen_rows": 8}))
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.rounds):
                    bat.step()
                torch.cuda.synchronize()
                dt = 1e3 * (time.perf_counter() - t) / a.rounds
                assert len(bat._live()) == B, "the batch must be full for the whole window"
                bat.close()
                if stt is not None:
                    assert stt.stats.rounds == 0
                    stt.close()
                if rep:
                    ms[kind].append(dt)
        lo, hi = min(ms["without_stt"]), max(ms["without_stt"])
        res["c_round_ms"] = {"live_streams": B, "rounds": a.rounds, "without_stt": spread(ms["without_stt"]), "with_idle_stt": spread(ms["with_idle_stt"]),
                             "with_idle_stt_within_spread_of_without": bool(lo <= statistics.median(ms["with_idle_stt"]) <= hi),
                             "order": "the two kinds in turn, a fresh batcher each, one warm-up pair"}
        print(json.dumps(res["c_round_ms"]), flush=True)
        save()

    # ---- (b) from the round that cuts the windows to the transcripts ---------------------------------------------------------------------------------
    if "b" in a.only:
        vcfg = VadConfig(silence_ms=300)
        fl = vcfg.frame_len(SR)
        clip = np.concatenate([0.002 * rng.standard_normal(10 * fl), 0.3 * rng.standard_normal(60 * fl), 0.002 * rng.standard_normal(20 * fl)]).astype(np.float32)
        out = {}
        for K in (1, 8):
            lat, rounds = [], []
            for rep in range(a.repeats + 1):
                stt = wm.serve(max_rows=8)
                bat, futs = batcher(400, stt=stt, listen_rows=8, listen_max_frames=375)
                mics = [bat.listen(vad=vcfg, transcribe=dict(language=0, sample_len=a.sample_len)) for _ in range(K)]
                t0 = r0 = None
                for i in range(0, 100000):
                    for lis in mics:
                        if i * 1920 < clip.shape[0]:
                            lis.feed(clip[i * 1920 : (i + 1) * 1920])  # 80 ms per round: what the round generates
                    cuts = bat.stats["stt_cuts"]
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    bat.step()
                    if t0 is None and bat.stats["stt_cuts"] > cuts:
                        t0, r0 = t, i
                    if all(lis.transcript.done() for lis in mics):
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        break
                    assert i < 400
                assert bat.stats["stt_cuts"] == 1 and bat.stats["stt_windows"] == K and len(bat._live()) == B
                tokens = [len(lis.transcript.result(timeout=0).tokens) for lis in mics]
                bat.close()
                stt.close()
                if rep:
                    lat.append(1e3 * (t1 - t0))
                    rounds.append(i - r0 + 1)
            out[f"listeners_{K}"] = {"endpoint_round_to_transcript_ms": spread(lat), "scheduling_rounds": rounds, "transcript_tokens": tokens}
        res["b_endpoint_to_transcript"] = {"live_streams": B, "utterance_seconds": round(70 * fl / SR, 2), "sample_len": a.sample_len, "stt_rounds_per_round": 4,
                                          "note": "one synchronisation per round (the clock), so the rounds do not overlap the host", **out}
        print(json.dumps(res["b_endpoint_to_transcript"]), flush=True)
        save()


if __name__ == "__main__":
    main()
