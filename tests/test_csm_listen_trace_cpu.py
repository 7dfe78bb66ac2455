"""The engine-call sequence of the listening edge (DESIGN 8d-9 ... 8d-13), pinned: the result-level tests say what a listener resolves with,
this one says which calls the scheduler makes on the engine and its row objects, in which order and with which arguments.  Two small fixed
scenarios on the scripted engines of test_csm_continuous_cpu.py (detectors, converter, ring) and test_csm_formats_cpu.py (resampler,
converter), each beside one generating request, with `listen_rows=3`; `eng.calls`, the encoder's own `calls` and every result are compared
with tests/golden/csm_listen_trace.json.  CSM_LISTEN_TRACE_RECORD=1 writes that file instead of comparing: it is recorded on the commit
BEFORE a change to the listening edge, never on the changed code."""
import json
import os
import queue
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_csm_continuous_cpu as C  # noqa: E402
import test_csm_formats_cpu as F  # noqa: E402
from test_csm_interrupt_cpu import _req  # noqa: E402
from test_csm_vad_cpu import LOUD, QUIET, _clip  # noqa: E402

from mlx_audio_amd import pcm  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "csm_listen_trace.json")


def _plain_json(x):
    """Tuples, numpy scalars and tensors as what JSON holds: lists, ints, floats."""
    if isinstance(x, dict):
        return {str(k): _plain_json(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain_json(v) for v in x]
    if isinstance(x, (np.integer, np.bool_)):
        return x.item()
    if isinstance(x, np.floating):
        return float(x)
    if hasattr(x, "__dataclass_fields__"):
        return {k: _plain_json(getattr(x, k)) for k in x.__dataclass_fields__}
    if hasattr(x, "tolist"):
        return x.tolist()
    return x


def _result(res):
    return _plain_json(dict(codes=res.codes.cpu().numpy(), frames=res.frames, samples=res.samples, steps=res.steps, sample_rate=res.sample_rate,
                            format=res.format, speech_start=res.speech_start, speech_stop=res.speech_stop))


def _detectors():
    """A one-shot VAD listener fed s16le, a plain listener on the host path and an always-open microphone that yields two utterances --
    the first is ended, the second dropped when the stream needs its room in the ring -- beside one generating request; ticket lag 1."""
    cfg = C._cfg()
    eng = C.Engine(lag=1)
    bat = C._listen_batcher(eng, rows=3)
    req = _req(bat, 1, 40)
    a, b = bat.listen(vad=cfg, format="s16le"), bat.listen()
    mic = bat.listen(vad=cfg, continuous=True)
    ca = pcm.encode(_clip([(2, QUIET), (2, LOUD), (5, QUIET)], 2), "s16le").tobytes()
    cb = _clip([(8, LOUD)], 4)
    S = _clip([(2, QUIET), (2, LOUD), (6, QUIET), (2, LOUD), (16, QUIET)], 9)
    utts, ends = [], []

    def drain():
        while True:
            try:
                u = mic.next_utterance(0)
            except queue.Empty:
                return
            if u is None:
                return
            utts.append(u)
            if len(utts) == 1:
                ends.append(u.end())

    for r in range(-(-S.shape[0] // 100)):
        if ca[200 * r : 200 * r + 200]:
            a.feed(ca[200 * r : 200 * r + 200])
        if cb[100 * r : 100 * r + 100].shape[0]:
            b.feed(cb[100 * r : 100 * r + 100])
        while True:
            try:
                mic.feed(S[100 * r : 100 * r + 100])
                break
            except ValueError:  # the host queue is full while the gate holds the stream back: a full queue is waited for, never overrun
                assert bat.step()
                drain()
        bat.step()
        drain()
    fa, fb = a.end(), b.end()
    mic.close()
    bat.run_until_idle()
    drain()
    assert len(utts) == 2 and utts[1].dropped and not utts[0].dropped and mic.next_utterance(0) is None
    out = dict(calls=eng.calls, enc_calls=eng.enc.calls,
               results=dict(vad=_result(fa.result(timeout=0)), plain=_result(fb.result(timeout=0)), utterance=_result(ends[0].result(timeout=0))),
               spans=dict(vad=a.endpoint.result(timeout=0), vad_onset=a.onset.result(timeout=0),
                          utterances=[u.endpoint.result(timeout=0) for u in utts], onsets=[u.onset for u in utts]),
               request=dict(frames=req.result(timeout=0).frames, codes=req.result(timeout=0).codes.cpu().numpy()))
    bat.close()
    return _plain_json(out)


def _rates():
    """The rated path, which the detectors' engine has no resampler for: a 16 kHz s16le listener, a 48 kHz float32 listener and a plain
    one on the host path, beside one generating request."""
    eng = F.Engine()
    bat = F._listen_batcher(eng, rows=3)
    req = _req(bat, 1, 20)
    a, b, c = bat.listen(sample_rate=16000, format="s16le"), bat.listen(sample_rate=48000), bat.listen()
    ca = pcm.encode(F._wave(1, 70), "s16le").tobytes()
    cb, cc = F._wave(2, 200), F._wave(3, 100)
    for r in range(2):
        a.feed(ca[70 * r : 70 * r + 70])
        b.feed(cb[100 * r : 100 * r + 100])
        c.feed(cc[50 * r : 50 * r + 50])
        bat.step()
    futs = [a.end(), b.end(), c.end()]
    bat.run_until_idle()
    out = dict(calls=eng.calls, enc_calls=eng.enc.calls, results=[_result(f.result(timeout=0)) for f in futs],
               request=dict(frames=req.result(timeout=0).frames, codes=req.result(timeout=0).codes.cpu().numpy()))
    bat.close()
    return _plain_json(out)


def test_the_engine_calls_and_results_are_the_recorded_ones():
    have = {"detectors": _detectors(), "rates": _rates()}
    if os.environ.get("CSM_LISTEN_TRACE_RECORD") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(have, f, separators=(",", ":"))
    with open(GOLDEN) as f:
        want = json.load(f)
    for name in ("detectors", "rates"):
        assert want[name]["calls"] and set(have[name]) == set(want[name])
        for key in want[name]:
            if key in ("calls", "enc_calls"):
                for i, (h, w) in enumerate(zip(have[name][key], want[name][key])):
                    assert h == w, f"{name}: {key}[{i}] is {h}, recorded {w}"
                assert len(have[name][key]) == len(want[name][key])
            else:
                assert have[name][key] == want[name][key], f"{name}: {key}"
