"""The scheduler of whisper_serve.WhisperBatcher on a fake engine behind its seam (no GPU): admission order, row reuse, the poll cadence, per-request
limits, the prefill cap, the detection round, cancellation, close; the option checks at submit; and the row-mode entries of the C ABI on a handle
that has no device state."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _whisper_text_ref as T  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd.whisper_serve import GroupRead, WhisperBatcher  # noqa: E402

DIMS = T.dims(128, 2, 2, 51865, 100)
TOK = whisper.special_tokens(DIMS)


def window(end_at=0, tag=0):
    """a features window for the fake: [0, 0] = the pick at which the row samples eot (0: never), [0, 1] = a tag to tell requests apart"""
    x = np.zeros((DIMS.n_audio_ctx, DIMS.n_audio_state), np.float32)
    x[0, 0], x[0, 1] = end_at, tag
    return x


class FakeEngine:
    """Every request is a group of rows; a row samples 1000 + k at pick k and eot from pick `end_at` on.  A beam group is complete -- every row flagged --
    from the pick `end_at` on, and its finished store then holds ONE sequence per beam: [1000 + 1 .. 1000 + end_at - 1] + [slot].  Every call is logged;
    a plain group of one row is logged as that row ("admit", "detect", "read"), any other by its rows ("admit_group", "detect_group", "read_group")."""

    def __init__(self):
        self.dims, self.log, self.rows, self.counts = DIMS, [], {}, {}  # counts: request tag -> the picks it got
        self.groups = {}  # leader -> dict(rows, beam, max_candidates, draws)

    def check_window(self, x):
        if len(x.shape) != 2:
            raise ValueError("submit takes ONE window")

    def open(self, max_rows):
        self.max_rows = max_rows

    def _entry(self, what, rows, *more):
        single = len(rows) == 1 and not self.groups[rows[0]]["beam"]
        self.log.append((what, rows[0]) + more[:1] if single else (what + "_group", tuple(rows)) + more)

    def admit(self, rows, x, init, options, beam=False, max_candidates=1, draws=None):
        for r in rows:
            assert r not in self.rows, "a row is handed on only after its group was read"
            self.rows[r] = dict(end_at=int(x[0, 0]), tag=int(x[0, 1]), tokens=[], init=init)
        self.groups[rows[0]] = dict(rows=tuple(rows), beam=beam, max_candidates=max_candidates, draws=draws)
        self._entry("admit", rows, int(x[0, 1]), beam)
        return x

    def forward(self, items, out_rows):
        for row, pos, count, frm, keep, slot in items:
            assert row in self.rows and pos + count <= DIMS.n_text_ctx
        self.log.append(("forward", tuple(items), tuple(out_rows)))

    def detect(self, rows, out_index, token_index):
        self._entry("detect", rows, token_index)

    def pick(self, rows):
        for r in rows:
            s = self.rows[r]
            k = len(s["tokens"]) + 1
            s["tokens"].append(TOK.eot if s["end_at"] and k >= s["end_at"] else 1000 + k)
        self.log.append(("pick", tuple(rows)))

    def flags(self):
        self.log.append(("flags",))
        return [r in self.rows and TOK.eot in self.rows[r]["tokens"] for r in range(self.max_rows)]

    def read(self, rows, detected, sot_index):
        self._entry("read", rows, self.rows[rows[0]]["tag"])
        g = self.groups.pop(rows[0])
        assert tuple(rows) == g["rows"]
        states = [self.rows.pop(r) for r in rows]
        self.counts[states[0]["tag"]] = len(states[0]["tokens"])
        live = [(list(s["tokens"]), -float(len(s["tokens"]) + k)) for k, s in enumerate(states)]
        finished = []
        if g["beam"]:
            end = states[0]["end_at"]
            if end and len(states[0]["tokens"]) >= end:
                finished = [([1000 + i for i in range(1, end)] + [k], -float(k + 1)) for k in range(len(rows))]
            live = [([t for t in s["tokens"] if t != TOK.eot], -10.0 - k) for k, s in enumerate(states)]
        return GroupRead(finished=finished, live=live, no_speech_prob=0.25,
                        language_probs={t: (0.5 if t == TOK.language_tokens[3] else 0.0) for t in TOK.language_tokens} if detected else None)

    def close(self):
        self.log.append(("close",))


def serve(**kw):
    eng = FakeEngine()
    return eng, WhisperBatcher(engine=eng, **kw)


def test_admission_is_fifo_and_a_row_is_reused_only_after_it_was_retired():
    eng, s = serve(max_rows=2, eos_check_interval=2)
    ends = [3, 1, 5, 2, 4]
    futs = [s.submit(window(e, i), language=0, sample_len=8) for i, e in enumerate(ends)]
    s.run_until_idle()
    assert [e[2] for e in eng.log if e[0] == "admit"] == [0, 1, 2, 3, 4]
    assert s.stats.admissions == 5 and s.stats.retired == 5 and not eng.rows
    for i, f in enumerate(futs):
        r = f.result(timeout=1)
        assert r.tokens == [1000 + k for k in range(1, ends[i])] and r.language == TOK.language_tokens[0] and r.no_speech_prob == 0.25
        assert r.avg_logprob == -float(eng.counts[i]) / (len(r.tokens) + 1) and r.temperature == 0.0 and r.language_probs is None
    # (FakeEngine.admit asserts that the row's previous occupant was read back first)
    assert s.stats.ended_row_rounds == sum(eng.counts[i] - e for i, e in enumerate(ends)) > 0
    assert not s.step()


def test_the_poll_runs_every_interval_rounds_and_not_between():
    eng, s = serve(max_rows=2, eos_check_interval=3)
    for i in range(4):
        s.submit(window(2, i), language=0, sample_len=50)
    s.run_until_idle()
    kinds = [e[0] for e in eng.log if e[0] in ("forward", "flags")]
    gaps = "".join("F" if k == "forward" else "|" for k in kinds).split("|")
    assert gaps[-1] == "" and all(g == "FFF" for g in gaps[:-1]) and len(gaps) == 3, kinds  # 3 rounds, a poll, 3 rounds, a poll
    assert s.stats.polls == 2 and s.stats.rounds == 6


def test_each_request_keeps_its_own_limit():
    """sample_len picks exactly; and decode's `sample_begin + i > n_ctx` rule for a prompt that fills the context"""
    eng, s = serve(max_rows=3, eos_check_interval=4)
    a = s.submit(window(0, 0), language=0, sample_len=5)
    b = s.submit(window(0, 1), language=0, sample_len=9)
    c = s.submit(window(0, 2), language=0, prompt=list(range(300)))  # the prompt is cut to n_ctx // 2 - 1 tokens
    s.run_until_idle()
    assert len(a.result(1).tokens) == 5 and len(b.result(1).tokens) == 9 and s.stats.polls > 0
    n_ctx = DIMS.n_text_ctx
    begin = len(WD.initial_tokens(TOK, WD.DecodingOptions(language=0, prompt=list(range(300))), n_ctx, n_ctx // 2))
    solo = 1 + sum(1 for i in range(1, n_ctx // 2) if begin + i <= n_ctx)  # decode's loop, pick by pick
    assert begin == 1 + 223 + 3 and solo == 222 and len(c.result(1).tokens) == solo
    last = [e for e in eng.log if e[0] == "forward"][-1][1]
    assert last == ((2, n_ctx - 1, 1, -1, -1, 0),)  # its last step sits at the last position


def test_the_prefill_cap_spreads_two_long_prompts_over_two_rounds():
    eng, s = serve(max_rows=4, eos_check_interval=8, max_round_tokens=150)
    for i in range(2):
        s.submit(window(0, i), language=0, sample_len=2, prompt=list(range(100)))
    s.submit(window(0, 2), language=0, sample_len=2)
    s.run_until_idle()
    fw = [e[1] for e in eng.log if e[0] == "forward"]
    assert [[it[2] for it in items] for items in fw[:3]] == [[104], [1, 104, 3], [1, 1]]  # the short third request rides with the second prompt
    assert [e[2] for e in eng.log if e[0] == "admit"] == [0, 1, 2]


def test_the_detection_round_precedes_the_prefill_and_lang_id_retires_after_it():
    eng, s = serve(max_rows=3, eos_check_interval=8)
    a = s.submit(window(0, 0), sample_len=2, prompt=[5, 6])          # language None: detect, then decode
    b = s.submit(window(0, 1), task="lang_id", language=7)           # lang_id with a language given: detect only, nothing written
    c = s.submit(window(0, 2), language=2, sample_len=2)
    s.run_until_idle()
    fw = [e[1] for e in eng.log if e[0] == "forward"]
    assert fw[0] == ((0, 0, 1, 3, 0, 0), (1, 0, 1, 0, 0, 0), (2, 0, 3, 0, 0, 1))  # [sot] at position 0 for a and b, c's prefill
    assert fw[1] == ((0, 0, 6, 0, 3, 1), (2, 3, 1, -1, -1, 0))                    # a's prefill keeps its sot position; b is gone
    assert [e for e in eng.log if e[0] == "detect"] == [("detect", 0, 4), ("detect", 1, None)]
    rb = b.result(1)
    assert rb.tokens == [] and rb.language == TOK.language_tokens[3] and rb.language_probs[TOK.language_tokens[3]] == 0.5 and np.isnan(rb.avg_logprob)
    ra = a.result(1)
    assert ra.language == TOK.language_tokens[3] and ra.language_probs is None and len(ra.tokens) == 2
    assert c.result(1).language == TOK.language_tokens[2] and s.stats.detections == 2


def test_a_cancelled_queued_request_is_never_admitted():
    eng, s = serve(max_rows=1, eos_check_interval=2)
    a = s.submit(window(2, 0), language=0)
    b = s.submit(window(2, 1), language=0)
    c = s.submit(window(2, 2), language=0)
    assert s.step() and b.cancel() and not a.cancel()  # a is running
    s.run_until_idle()
    assert [e[2] for e in eng.log if e[0] == "admit"] == [0, 2] and b.cancelled() and len(c.result(1).tokens) == 1


def test_close_fails_what_is_pending_and_racing_submits_never_hang():
    eng, s = serve(max_rows=2, eos_check_interval=2)
    s.start()
    futs, errors = [], []

    def client(k):
        for i in range(200):
            try:
                futs.append(s.submit(window(3, 1000 * k + i), language=0))
            except RuntimeError as e:
                errors.append(e)
                return

    threads = [threading.Thread(target=client, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    while len(futs) < 20:
        pass
    s.close()
    for t in threads:
        t.join(timeout=10)
        assert not t.is_alive()
    done = failed = 0
    for f in futs:
        try:
            f.result(timeout=10)  # every future is settled: a result, or "closed"
            done += 1
        except RuntimeError as e:
            assert "closed" in str(e)
            failed += 1
    assert done + failed == len(futs)
    with pytest.raises(RuntimeError, match="closed"):
        s.submit(window(), language=0)
    s.close()  # twice is fine
    # without a thread: queued and live requests are failed by close
    eng, s = serve(max_rows=1)
    a, b = s.submit(window(), language=0), s.submit(window(), language=0)
    s.step()
    s.close()
    for f in (a, b):
        with pytest.raises(RuntimeError, match="closed"):
            f.result(timeout=1)


def test_submit_checks_the_options_with_decodes_own_messages():
    eng, s = serve(max_rows=1)
    with pytest.raises(NotImplementedError, match="temperature > 0 is not yet implemented"):
        s.submit(window(), temperature=0.5)
    with pytest.raises(NotImplementedError, match="Beam search decoder is not yet implemented"):
        s.submit(window(), beam_size=4)
    with pytest.raises(ValueError, match="prompt must be a list of token ids"):
        s.submit(window(), prompt="hello")
    with pytest.raises(ValueError, match="leave no room"):
        s.submit(window(), language=0, prefix=list(range(300)), prompt=list(range(300)), sample_len=1)
    with pytest.raises(ValueError, match="ONE window"):
        s.submit(np.zeros((2, 100, 128), np.float32), language=0)
    assert not eng.log and not s.step()
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        whisper.Model(DIMS).serve()


def test_the_row_entries_of_the_library_without_a_gpu():
    from mlx_audio_amd import _lib

    lib = _lib.load()
    assert lib.kk_abi_minor() >= 17
    cfg = dict(n_vocab=51865, n_text_ctx=448, n_text_state=384, n_text_head=6, n_text_layer=1, n_audio_ctx=1500, n_audio_state=384)
    h = C.c_void_p()
    assert lib.kk_whisper_text_create(C.byref(_lib.KKWhisperTextConfig(**cfg)), C.byref(h)) == 0
    assert lib.kk_whisper_text_rows_state_bytes(h, 0) == 0 and lib.kk_whisper_text_rows_state_bytes(h, _lib.WHISPER_MAX_ROWS + 1) == 0
    assert lib.kk_whisper_text_rows_state_bytes(h, 2) > 2 * 1500 * 2 * 384 * 2
    assert lib.kk_whisper_text_rows_workspace_bytes(h, 0, 1) == 0 and lib.kk_whisper_text_rows_workspace_bytes(h, 24, 3) > 24 * 384 * 4
    item = (_lib.KKWhisperRowsItem * 1)(_lib.KKWhisperRowsItem(0, 0, 1, 0, -1, 0))
    z = np.zeros(4, np.int32)
    buf = C.create_string_buffer(64)
    assert lib.kk_whisper_text_rows_forward(h, None, C.cast(item, C.c_void_p), 1, z.ctypes.data_as(C.c_void_p), 1, C.cast(buf, C.c_void_p),
                                            C.cast(buf, C.c_void_p), 64) != 0
    assert b"row mode not opened" in lib.kk_last_error()
    assert lib.kk_whisper_text_rows_open(h, None, 2, C.cast(buf, C.c_void_p), 64) != 0 and b"not finalized" in lib.kk_last_error()
    for call in (lambda: lib.kk_whisper_text_rows_pick(h, None, z.ctypes.data_as(C.c_void_p), 1),
                 lambda: lib.kk_whisper_text_rows_flags(h, None, z.ctypes.data_as(C.c_void_p)),
                 lambda: lib.kk_whisper_text_rows_set_token(h, None, 0, 0, C.cast(buf, C.c_void_p))):
        assert call() != 0 and b"row mode not opened" in lib.kk_last_error()
    lib.kk_whisper_text_destroy(h)
