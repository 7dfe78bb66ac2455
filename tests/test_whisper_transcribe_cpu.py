"""Long-form transcription without a GPU: whisper_transcribe.FileState against the plain restatement of the reference's loop
(tests/_whisper_transcribe_ref.py) on scripted DecodingResults, branch by branch and over a seeded sweep; the stall guard; the decode-only tokenizer
on a synthetic rank file; `compression_ratio`; the scheduler `drive` on a fake backend; `WhisperBatcher.submit_sampled` on the fake engine of
tests/test_whisper_serve_cpu.py; and the argument checks of `transcribe`, kk_whisper_text_rows_set_draw and kk_op_mel_windows."""
import base64
import ctypes as C
import os
import sys
import types
import zlib
from concurrent.futures import Future
from dataclasses import replace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_text_ref as T  # noqa: E402
from _whisper_transcribe_ref import transcribe_ref  # noqa: E402
from test_whisper_serve_cpu import FakeEngine, window  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_transcribe as WT  # noqa: E402
from mlx_audio_amd.whisper_decoding import DecodingResult  # noqa: E402
from mlx_audio_amd.whisper_serve import WhisperBatcher  # noqa: E402
from mlx_audio_amd.whisper_tokenizer import Tokenizer  # noqa: E402

DIMS = T.dims(128, 2, 2, 51865, 100)
TOK = whisper.special_tokens(DIMS)
TB, EOT, W = TOK.timestamp_begin, TOK.eot, 200
MODEL = dict(W=W, n_audio_ctx=100, timestamp_begin=TB, eot=EOT)
NO_TEXT = dict(compression_ratio_threshold=None)


def res(tokens, lp=-0.5, ns=0.1, t=0.0):
    return DecodingResult(audio_features=None, language=None, tokens=list(tokens), avg_logprob=lp, no_speech_prob=ns, temperature=t)


def run_state(content_frames, script, **kw):
    st = WT.FileState(content_frames, **MODEL, **kw)
    calls = []
    while True:
        req = st.next_window()
        if req is None:
            break
        assert st.next_window() is req  # asking twice asks for the same window
        calls.append((req.seek, req.size, req.prompt, req.temperature))
        st.feed(script(req.seek, req.size, list(req.prompt), req.temperature))
    return st.result(None), calls


def both(content_frames, script, **kw):
    """-> (the state machine's result, its calls) after checking both against the restatement"""
    want = transcribe_ref(content_frames, script, **MODEL, **kw)
    got, calls = run_state(content_frames, script, **kw)
    assert calls == want["calls"]
    assert got.segments == want["segments"] and got.tokens == want["tokens"] and got.text == want["text"]
    return got, calls


def table(rows, default=None):
    """a script from {(seek, temperature): result}; the result's temperature is filled in"""
    def script(seek, size, prompt, t):
        r = rows.get((seek, t), default)
        assert r is not None, (seek, t)
        return r if r.temperature == t else replace(r, temperature=t)
    return script


# ---- the three segmentation cases and the seek advance -------------------------------------------------------------------------------------------
def test_consecutive_pairs_with_a_single_timestamp_ending():
    toks = [TB, 5, 6, TB + 10, TB + 10, 7, 8, TB + 30]
    got, calls = both(150, table({(0, 0.0): res(toks)}), **NO_TEXT)
    assert [(s["id"], s["seek"], s["start"], s["end"], s["tokens"]) for s in got.segments] == \
        [(0, 0, 0.0, 10 * 0.02, toks[:4]), (1, 0, 10 * 0.02, 30 * 0.02, toks[4:])]
    assert calls == [(0, 150, (), 0.0)] and got.tokens == toks and got.text is None  # seek moved by the window's size: one window
    assert set(got.segments[0]) == {"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}


def test_consecutive_pairs_without_one_seek_to_the_last_timestamp():
    first = [TB, 5, TB + 20, TB + 20, 7]  # the unfinished tail [TB + 20, 7] is dropped
    second = [TB, 9, TB + 40]
    got, calls = both(150, table({(0, 0.0): res(first), (40, 0.0): res(second)}), **NO_TEXT)
    assert calls == [(0, 150, (), 0.0), (40, 110, tuple(first[:3]), 0.0)]  # 20 timestamps = 40 frames; the prompt is the previous text
    assert [s["tokens"] for s in got.segments] == [first[:3], second] and got.segments[1]["start"] == 0.4 and got.segments[1]["end"] == 0.4 + 40 * 0.02


@pytest.mark.parametrize("toks,duration", [([5, 6], 1.5), ([TB, 5, 6, TB + 50], 1.0), ([5, TB], 1.5), ([], 1.5)])
def test_no_pair_at_all_takes_the_last_nonzero_timestamp_as_the_duration(toks, duration):
    got, calls = both(150, table({(0, 0.0): res(toks)}), **NO_TEXT)
    assert len(calls) == 1 and len(got.segments) == 1 and got.segments[0]["end"] == duration and got.segments[0]["tokens"] == toks


def test_windows_of_W_frames_and_the_tail():
    got, calls = both(450, table({}, default=res([TB, 5, TB + 90])), **NO_TEXT)
    assert [(c[0], c[1]) for c in calls] == [(0, 200), (200, 200), (400, 50)]
    assert [s["start"] for s in got.segments] == [0.0, 2.0, 4.0]


# ---- fallback, no-speech ------------------------------------------------------------------------------------------------------------------------
def test_the_temperature_fallback_on_the_log_probability():
    rows = {(0, 0.0): res([5], lp=-2.0), (0, 0.2): res([6], lp=-1.5), (0, 0.4): res([7], lp=-0.9)}
    got, calls = both(100, table(rows), **NO_TEXT)
    assert [c[3] for c in calls] == [0.0, 0.2, 0.4] and got.segments[0]["temperature"] == 0.4 and got.tokens == [7]
    got, calls = both(100, table(rows), logprob_threshold=None, **NO_TEXT)  # no threshold, no fallback
    assert [c[3] for c in calls] == [0.0] and got.tokens == [5]


def test_an_exhausted_ladder_keeps_the_last_result_and_a_hot_window_resets_the_prompt():
    bad = {(0, t): res([5, 6], lp=-3.0) for t in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)}
    bad[(100, 0.0)] = res([8])
    got, calls = both(200, table(bad), clip_timestamps=[0.0, 1.0, 1.0, 2.0], **NO_TEXT)
    assert [c[3] for c in calls] == [0.0, 0.2, 0.4, 0.6, 0.8, 1.0, 0.0] and calls[-1][2] == ()  # temperature 1.0 > 0.5: the next window gets no prompt
    warm = {(0, 0.0): res([5, 6], lp=-3.0), (0, 0.2): res([5, 6], lp=-0.2), (100, 0.0): res([8])}
    got, calls = both(200, table(warm), clip_timestamps=[0.0, 1.0, 1.0, 2.0], **NO_TEXT)
    assert calls[-1][2] == (5, 6)  # 0.2 <= 0.5: the prompt stays


def test_silence_cancels_the_fallback_and_skips_the_window_unless_its_log_probability_is_high():
    rows = {(0, 0.0): res([5], lp=-2.0, ns=0.9), (200, 0.0): res([6], lp=-0.3, ns=0.9), (400, 0.0): res([7])}
    got, calls = both(500, table(rows), **NO_TEXT)
    assert [c[:2] + c[3:] for c in calls] == [(0, 200, 0.0), (200, 200, 0.0), (400, 100, 0.0)]  # no second temperature for the silent window
    assert [s["tokens"] for s in got.segments] == [[6], [7]] and got.segments[0]["seek"] == 200  # the first window left nothing
    rows.update({(0, t): res([5], lp=-2.0, ns=0.9) for t in (0.2, 0.4, 0.6, 0.8, 1.0)})
    got, calls = both(500, table(rows), no_speech_threshold=None, **NO_TEXT)  # without the threshold the first window falls back to the end and stays
    assert [c[3] for c in calls[:6]] == [0.0, 0.2, 0.4, 0.6, 0.8, 1.0] and [s["tokens"] for s in got.segments] == [[5], [6], [7]]
    got, calls = both(500, table(rows), logprob_threshold=None, **NO_TEXT)  # without the log-probability exception both silent windows go
    assert [s["tokens"] for s in got.segments] == [[7]]


# ---- prompts, clips ---------------------------------------------------------------------------------------------------------------------------------
def test_the_prompt_is_the_previous_text_unless_conditioning_is_off_and_the_initial_prompt_leads_it():
    script = table({}, default=res([TB, 5, TB + 100]))
    got, calls = both(400, script, initial_prompt=[11, 12], **NO_TEXT)
    assert [c[2] for c in calls] == [(11, 12), (11, 12, TB, 5, TB + 100)] and got.tokens == [TB, 5, TB + 100] * 2
    got, calls = both(400, script, initial_prompt=[11, 12], condition_on_previous_text=False, **NO_TEXT)
    assert [c[2] for c in calls] == [(11, 12), ()]
    with pytest.raises(ValueError, match="list of token ids"):
        WT.FileState(100, **MODEL, initial_prompt="hello", **NO_TEXT)


def test_clip_timestamps():
    assert WT.parse_clip_timestamps("0", 450) == [(0, 450)] and WT.parse_clip_timestamps("", 450) == [(0, 450)]
    assert WT.parse_clip_timestamps("1.5", 450) == [(150, 450)] and WT.parse_clip_timestamps([0.5, 2.0], 450) == [(50, 200)]
    assert WT.parse_clip_timestamps("0,1,2,99", 450) == [(0, 100), (200, 450)] and WT.parse_clip_timestamps([0.0, 1.0, 2.0], 450) == [(0, 100), (200, 450)]
    script = table({}, default=res([5]))
    got, calls = both(450, script, clip_timestamps=[0.5, 2.0], **NO_TEXT)
    assert [(c[0], c[1]) for c in calls] == [(50, 150)]
    got, calls = both(450, script, clip_timestamps="1.5", **NO_TEXT)
    assert [(c[0], c[1]) for c in calls] == [(150, 200), (350, 100)]
    got, calls = both(450, script, clip_timestamps="0,1,2,99", **NO_TEXT)  # ONE seek across the clips, as the reference keeps it
    assert [(c[0], c[1]) for c in calls] == [(0, 100), (100, 200), (300, 150)]
    got, calls = both(450, script, clip_timestamps="9", **NO_TEXT)  # behind the content: nothing to do
    assert calls == [] and got.segments == [] and got.tokens == []


# ---- clearing, the tokenizer, the compression ratio ---------------------------------------------------------------------------------------------
def rank_file(tmp_path, pieces):
    p = tmp_path / "vocab.tiktoken"
    p.write_bytes(b"".join(base64.b64encode(b) + b" " + str(i).encode() + b"\n" for i, b in enumerate(pieces)))
    return str(p)


EURO = "€".encode()  # three bytes
PIECES = [b"hello", b" world", b" ", EURO[:2], EURO[2:], b"\x80", b"ab", b"\n"]


def test_the_tokenizer_on_a_synthetic_rank_file(tmp_path):
    tk = Tokenizer.from_file(rank_file(tmp_path, PIECES), DIMS)
    assert tk.eot == EOT and tk.decode([0, 1]) == "hello world"
    assert tk.decode([3, 4]) == "€" and tk.decode([0, 3, 4, 1]) == "hello€ world"  # a character split across two tokens
    assert tk.decode([3]) == "�" and tk.decode([0, 5, 1]) == "hello� world"        # a truncated character, a lone continuation byte
    assert tk.decode([TOK.sot, 0, TB + 3, EOT, 1]) == "hello world" and tk.decode([]) == ""   # ids from eot on carry no text
    with pytest.raises(ValueError, match="not in the vocabulary"):
        tk.decode([len(PIECES)])
    bad = tmp_path / "bad.tiktoken"
    bad.write_bytes(b"aGVsbG8= 0\nnot-base64!! 1\n")
    with pytest.raises(ValueError, match="line 2"):
        Tokenizer.from_file(str(bad), DIMS)
    bad.write_bytes(b"aGVsbG8= 0\naGVsbG8= 0\n")
    with pytest.raises(ValueError, match="twice"):
        Tokenizer.from_file(str(bad), DIMS)


def test_compression_ratio():
    for text in ("", "hello world", "ab" * 200, "€" * 50):
        b = text.encode("utf-8")
        assert WT.compression_ratio(text) == len(b) / len(zlib.compress(b))
    assert WT.compression_ratio("ab" * 200) > 2.4 > WT.compression_ratio("hello world")


def test_with_a_tokenizer_texts_ratios_the_repetition_fallback_and_blank_clearing(tmp_path):
    tk = Tokenizer.from_file(rank_file(tmp_path, PIECES), DIMS)
    rep = [TB] + [6] * 200 + [TB + 50]  # "ab" x 200: too repetitive
    rows = {(0, 0.0): res(rep), (0, 0.2): res([TB, 0, 1, TB + 50, TB + 50, 2, 7, TB + 60, TB + 70, 0, TB + 70]),
            (200, 0.0): res([TB + 5, 0, TB + 5])}
    got, calls = both(300, table(rows), tokenizer=tk)
    assert [c[3] for c in calls] == [0.0, 0.2, 0.0]
    assert [s["text"] for s in got.segments] == ["hello world", "", "", "hello"]  # " \n" is blank: cleared
    assert [s["tokens"] for s in got.segments][1:3] == [[], []] and got.text == "hello worldhello"
    assert got.segments[2]["start"] == got.segments[2]["end"] == 70 * 0.02  # [TB + 70, 0, TB + 70]: instantaneous, cleared with its text
    text = "hello world \nhello"  # ids 0 1 2 7 0
    assert got.segments[0]["compression_ratio"] == WT.compression_ratio(text)  # of the WINDOW's text, stripped
    assert calls[2][2] == tuple(t for s in got.segments[:3] for t in s["tokens"])  # cleared segments leave the prompt
    with pytest.raises(ValueError, match="no tokenizer"):
        WT.FileState(100, **MODEL)
    got, _ = both(300, table(rows), **NO_TEXT)  # without one: no text, no blank clearing, the instantaneous one still goes
    assert [s["text"] for s in got.segments] == [None, None] and got.segments[0]["compression_ratio"] is None and got.segments[0]["tokens"] == rep
    inst = both(150, table({(0, 0.0): res([TB + 5, 0, TB + 5, TB + 5, 1, TB + 9])}), **NO_TEXT)[0]
    assert [s["tokens"] for s in inst.segments] == [[], [TB + 5, 1, TB + 9]] and inst.segments[0]["text"] is None
    blank = {(0, 0.0): res([TB, 2, 7, TB + 60])}
    assert both(150, table(blank), **NO_TEXT)[0].tokens == [TB, 2, 7, TB + 60] and both(150, table(blank), tokenizer=tk)[0].tokens == []


# ---- the stall guard ----------------------------------------------------------------------------------------------------------------------------
def test_a_window_that_leaves_seek_where_it_was_raises():
    with pytest.raises(RuntimeError, match="stalled"):
        run_state(150, table({(0, 0.0): res([TB, TB])}), **NO_TEXT)  # the last timestamp is 0: the reference would decode this window for ever
    with pytest.raises(RuntimeError, match="does not end"):
        transcribe_ref(150, table({(0, 0.0): res([TB, TB])}), **MODEL, max_windows=50, **NO_TEXT)
    with pytest.raises(RuntimeError, match="stalled"):
        run_state(150, table({}, default=res([5])), clip_timestamps=[0.0, 1.0, 3.0, 4.0, 5.0], **NO_TEXT)  # a middle clip behind the content


# ---- a seeded sweep: every branch against the restatement -----------------------------------------------------------------------------------------
def random_script(seed, hits):
    def script(seek, size, prompt, t):
        g = np.random.default_rng([seed, seek, int(round(t * 10))])
        kind = int(g.integers(0, 6))
        hits.add(kind)
        n = max(size // 2, 2)  # timestamps the window can hold
        a, b = sorted(int(x) for x in g.integers(1, n + 1, 2))
        text = [int(x) for x in g.integers(0, 8, int(g.integers(1, 4)))]
        toks = {0: [TB, *text, TB + a, TB + a, *text, TB + b],        # pairs, single ending
                1: [TB, *text, TB + a, TB + a, *text],                # pairs, no single ending: seek to a
                2: [TB, *text, TB + b],                               # no pair, a last timestamp
                3: text,                                              # no timestamp
                4: [TB + a, *text, TB + a, TB + a, 2, TB + b],        # an instantaneous and a blank segment
                5: []}[kind]
        lp = float(g.choice([-0.2, -1.5, -3.0, -3.0]))  # mostly too low, mostly not silent: about one window in twenty walks the whole ladder
        ns = float(g.choice([0.05, 0.05, 0.5, 0.95]))
        return res(toks, lp=lp, ns=ns, t=t)
    return script


@pytest.mark.parametrize("with_tokenizer", [False, True])
def test_a_seeded_sweep_equals_the_restatement(tmp_path, with_tokenizer):
    tk = Tokenizer.from_file(rank_file(tmp_path, PIECES), DIMS) if with_tokenizer else None
    hits, temps, skipped = set(), set(), 0
    for seed in range(40):
        g = np.random.default_rng(seed)
        kw = dict(tokenizer=tk, compression_ratio_threshold=2.4 if with_tokenizer else None,
                  logprob_threshold=[-1.0, None, -2.0][seed % 3], no_speech_threshold=[0.6, 0.6, None][seed % 3 if seed % 2 else 0],
                  condition_on_previous_text=bool(seed % 4), initial_prompt=[1, 2] if seed % 5 == 0 else None,
                  clip_timestamps=["0", [0.3, 4.1], "1.0", [0.0, 2.0, 2.0, 5.0]][seed % 4])
        frames = int(g.integers(520, 900))  # (behind every clip end: a middle clip that ends behind the content stalls the reference)
        got, calls = both(frames, random_script(seed, hits), **kw)
        temps |= {c[3] for c in calls}
        skipped += len({c[0] for c in calls}) - len({s["seek"] for s in got.segments})
    assert hits == set(range(6)) and temps == {0.0, 0.2, 0.4, 0.6, 0.8, 1.0} and skipped > 0


# ---- the scheduler ------------------------------------------------------------------------------------------------------------------------------
class FakeBackend:
    """a window's request takes 1 + (file + seek // 50) % 3 rounds; every call is logged"""

    def __init__(self, scripts):
        self.scripts, self.encoded, self.submitted, self.flying, self.peak = scripts, [], [], {}, 0

    def encode(self, batch):
        self.encoded.append(list(batch))
        return [("features", i, seek, size) for i, seek, size in batch]

    def submit(self, i, features, req):
        assert i not in self.flying, "two windows of one file in flight"
        assert features == ("features", i, req.seek, req.size)
        self.submitted.append((i, req))
        f = Future()
        self.flying[i] = [1 + (i + req.seek // 50) % 3, f, req]
        self.peak = max(self.peak, len(self.flying))
        return f

    def step(self):
        assert self.flying
        for i in list(self.flying):
            self.flying[i][0] -= 1
            if self.flying[i][0] == 0:
                _, f, req = self.flying.pop(i)
                f.set_result(self.scripts[i](req.seek, req.size, list(req.prompt), req.temperature))


def test_the_driver_runs_five_files_on_two_rows_each_as_it_runs_alone():
    frames = [450, 130, 700, 260, 390]
    scripts = [random_script(100 + i, set()) for i in range(5)]
    kw = dict(compression_ratio_threshold=None)
    states = [WT.FileState(n, **MODEL, **kw) for n in frames]
    be = FakeBackend(scripts)
    WT.drive(states, be, max_rows=2)
    assert be.peak == 2 and not be.flying and all(1 <= len(b) <= 2 for b in be.encoded)
    for i in range(5):
        solo_state = WT.FileState(frames[i], **MODEL, **kw)
        solo = FakeBackend([scripts[i]])
        WT.drive([solo_state], solo, 1)
        mine = [r for j, r in be.submitted if j == i]
        assert mine == [r for _, r in solo.submitted] and len(mine) > 0  # the same requests in the same order
        assert states[i].result(None) == solo_state.result(None)
        assert states[i].result(None).segments == transcribe_ref(frames[i], scripts[i], **MODEL, **kw)["segments"]
        windows = [(j, s, n) for b in be.encoded for j, s, n in b if j == i]
        assert windows == list(dict.fromkeys((i, r.seek, r.size) for r in mine))  # a window is encoded once, whatever its fallback passes
    for _, r in be.submitted:
        assert r.stream == (r.seek * 16 + r.temperature_index) & 0xFFFFFFFF and r.temperature == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)[r.temperature_index]
    assert any(r.temperature_index > 0 for _, r in be.submitted)
    assert WT.WindowRequest(2 ** 28 + 3, 200, (), 5, 1.0).stream == (3 * 16 + 5)  # the id wraps at 32 bits
    with pytest.raises(ValueError, match="at most 16"):
        WT.FileState(100, **MODEL, temperature=[0.0] + [0.05 * k for k in range(1, 17)], **kw)
    with pytest.raises(ValueError, match="max_rows"):
        WT.drive([], be, 0)


# ---- submit_sampled behind the engine seam ------------------------------------------------------------------------------------------------------
class DrawEngine(FakeEngine):
    def admit(self, rows, x, init, options, beam=False, max_candidates=1, draws=None):
        self.log.append(("draw", rows[0], draws[0] if draws else None))
        return super().admit(rows, x, init, options, beam, max_candidates, draws)


def test_submit_sampled_hands_the_draw_to_admit_and_submit_keeps_refusing():
    eng = DrawEngine()
    s = WhisperBatcher(engine=eng, max_rows=2, eos_check_interval=2)
    a = s.submit_sampled(window(3, 0), language=0, temperature=0.2, seed=7, stream=41)
    b = s.submit(window(3, 1), language=0)
    c = s.submit_sampled(window(2, 2), whisper.DecodingOptions(language=0, temperature=1.0, best_of=1), stream=2 ** 32 - 1)
    s.run_until_idle()
    assert [e for e in eng.log if e[0] == "draw"] == [("draw", 0, (0.2, 7, 41)), ("draw", 1, None), ("draw", 0, (1.0, 0, 2 ** 32 - 1))]
    assert a.result(1).temperature == 0.2 and b.result(1).temperature == 0.0 and c.result(1).temperature == 1.0 and len(a.result(1).tokens) == 2
    with pytest.raises(NotImplementedError, match="best_of groups are not built in the batcher"):
        s.submit_sampled(window(), language=0, temperature=0.5, best_of=2)
    with pytest.raises(ValueError, match="temperature 0 is greedy decoding"):
        s.submit_sampled(window(), language=0, temperature=0.0)
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
        s.submit_sampled(window(), language=0, temperature=0.5, beam_size=2)
    with pytest.raises(ValueError, match="stream"):
        s.submit_sampled(window(), language=0, temperature=0.5, stream=2 ** 32)
    with pytest.raises(NotImplementedError, match="temperature > 0 is not yet implemented"):
        s.submit(window(), temperature=0.5)
    s2 = WhisperBatcher(engine=FakeEngine(), max_rows=1)  # a greedy request has no draws
    f = s2.submit(window(2, 0), language=0)
    s2.run_until_idle()
    assert len(f.result(1).tokens) == 1


# ---- argument checks without a GPU ----------------------------------------------------------------------------------------------------------------
def test_transcribe_checks_its_arguments_before_anything_runs():
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        whisper.Model(DIMS).transcribe(np.zeros(16000, np.float32))
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        whisper.Model(DIMS).generate(np.zeros(16000, np.float32))
    stub = types.SimpleNamespace(_text=object(), dims=DIMS)
    x = np.zeros(16000, np.float32)
    for kw, exc, msg in [(dict(word_timestamps=True), NotImplementedError, "word_timestamps"),
                         (dict(hallucination_silence_threshold=2.0), NotImplementedError, "hallucination_silence_threshold"),
                         (dict(beam_size=5), NotImplementedError, "beam search"),
                         (dict(best_of=5), NotImplementedError, "best_of"),
                         (dict(), ValueError, "no tokenizer"),
                         (dict(compression_ratio_threshold=None, temperature=()), ValueError, "at least one"),
                         (dict(compression_ratio_threshold=None, temperature=(0.0, -1.0)), ValueError, "finite and >= 0"),
                         (dict(compression_ratio_threshold=None, initial_prompt="hi"), ValueError, "list of token ids"),
                         (dict(compression_ratio_threshold=None, prompt=[1]), ValueError, "initial_prompt"),
                         (dict(compression_ratio_threshold=None, task="lang_id"), ValueError, "task"),
                         (dict(compression_ratio_threshold=None, seed=1.5), ValueError, "seed"),
                         (dict(compression_ratio_threshold=None, no_such_option=1), TypeError, "no_such_option")]:
        with pytest.raises(exc, match=msg):
            WT.transcribe(stub, x, **kw)
    assert WT.transcribe(stub, [], compression_ratio_threshold=None) == []


def test_the_new_entries_of_the_library_without_a_gpu():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 25
    cfg = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=1, n_audio_ctx=1500, n_audio_state=384)
    h = C.c_void_p()
    assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**cfg)), C.byref(h)) == 0
    for t in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        assert lib.kk_whisper_text_rows_set_draw(h, None, 0, t, 0, 0) != 0 and b"temperature must be finite and > 0" in lib.kk_last_error()
    assert lib.kk_whisper_text_rows_set_draw(h, None, 0, 0.5, 0, 0) != 0 and b"row mode not opened" in lib.kk_last_error()
    assert lib.kk_whisper_text_rows_set_draw(None, None, 0, 0.5, 0, 0) != 0 and b"null model" in lib.kk_last_error()
    small = lib.kk_whisper_text_rows_state_bytes(h, 1)
    assert lib.kk_whisper_text_rows_state_bytes(h, 2) - small >= 16  # a draw per row
    lib.kk_whisper_text_destroy(h)

    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 15) & ~15

    def windows(R, src, frames, first, size, Wn=200, n_mels=80, out=base):
        arr = lambda v: (C.c_int32 * max(len(v), 1))(*v)  # noqa: E731
        return lib.kk_op_mel_windows(None, R, (C.c_void_p * max(len(src), 1))(*src), arr(frames), arr(first), arr(size), Wn, n_mels, C.c_void_p(out))

    for args, msg in [((0, [], [], [], []), b"R = 0"), ((33, [base] * 33, [9] * 33, [0] * 33, [1] * 33), b"R = 33"),
                      ((1, [base], [300], [0], [201]), b"size = 201"), ((1, [base], [300], [0], [-1]), b"size = -1"),
                      ((1, [base], [300], [101], [200]), b"outside the source's 300"), ((1, [base], [300], [-1], [10]), b"outside the source"),
                      ((1, [base + 4], [300], [0], [10]), b"16-byte aligned"), ((1, [None], [300], [0], [10]), b"16-byte aligned")]:
        assert windows(*args) != 0 and msg in lib.kk_last_error(), (args, lib.kk_last_error())
    assert windows(1, [base], [300], [0], [10], n_mels=64) != 0 and b"n_mels" in lib.kk_last_error()
    assert windows(1, [base], [300], [0], [10], out=base + 8) != 0 and b"out must be 16-byte aligned" in lib.kk_last_error()
    assert windows(1, [base], [300], [0], [0], Wn=0) != 0 and b"W = 0" in lib.kk_last_error()
