"""Whisper serving: 30-second windows join and leave ONE running decoder batch.  `Model.decode` is a static batch -- one set of options,
one shared position, every row stepped until the last has ended; a voice service's listeners close utterances at different moments, each with its own
language, prompt, prefix and length limit.  `WhisperBatcher` keeps `max_rows` decoder rows of the text handle's row mode (kk_whisper_text_rows_*,
whisper_decoding.RowRuntime) busy: a request is admitted into a free row, prefilled in the round that steps the other rows, picked with its own
parameters, and retired when it has ended or reached its own limit.

The contract: every request's `DecodingResult` equals, field by field (`tokens`, `avg_logprob`, `no_speech_prob`, `language`, `language_probs`,
`temperature`), what `model.decode(the same 2-D input, the same options)` returns alone -- whatever else the batch runs, in whatever order requests
arrive, whichever row they land in.  The kernels give a row the bits of its solo run (a row's bits depend on that row's inputs alone); the two
probabilities are the torch expressions of `decode` / `detect_language` on the same (1, V) / (1, n_languages) shapes of bit-identical logits.

One round (`step`):
  1. rows that cannot go on are retired: a row at its own limit (its `sample_len` and decode's `sample_begin + i > n_ctx` rule -- a row is never picked
     more often than its solo run), a `lang_id` row after its detection round and, every `eos_check_interval` rounds, the rows whose ended flag the
     poll finds set.  Retiring reads the row back and synchronises; between polls the host reads nothing from the device.
  2. queued requests are admitted FIFO into free rows, `max_round_tokens` of prefill per round at the most.
  3. ONE rows_forward over every live row: a fresh row carries its initial tokens, a row in detection `[sot]` at position 0, the others one token.
  4. ONE rows_pick over the rows that were prefilled or stepped.
A row that has ended keeps stepping and emits eot until the next poll notices, as in `decode`.  A request with `language=None` (or `task="lang_id"`)
spends one extra round first; the arg-maximum over the language tokens goes into its initial tokens on the device, with no synchronisation.

A request submitted with `submit_sampled` decodes at its own temperature: its row carries a draw (1 / T, Philox key, stream id) and the round's ONE
pick launch samples it while it picks the greedy rows; its result is `model.sample`'s for that window alone.  `submit` itself keeps
refusing a temperature.  `Model.transcribe` (whisper_transcribe.py) is the long-form loop on top of this batcher.

The scheduler talks to the model through an engine (`ModelEngine`); a fake engine tests it without a GPU.  Out of scope: best_of groups and beam
search inside the batcher, `generate` (see `Model.transcribe`), text-to-id encoding, hipGraph capture of the round, prefill on a side stream."""
from __future__ import annotations

import threading
from collections import deque
from concurrent.futures import Future
from dataclasses import dataclass, replace
from typing import Deque, Dict, List, Optional, Sequence, Tuple

from .whisper_decoding import (NOT_BUILT, DecodingOptions, DecodingResult, initial_tokens, special_tokens, verify_options)

NO_LANGUAGE_TOKENS = "This model doesn't have language tokens so it can't perform lang id"


@dataclass
class RowRead:
    """what retiring a row reads back"""
    tokens: Sequence[int]                 # the sampled tokens, `count` of them
    count: int
    sum_logprob: float
    no_speech_prob: float = float("nan")
    language_probs: Optional[Dict[int, float]] = None


@dataclass
class ServeStats:
    rounds: int = 0            # rows_forward calls
    admissions: int = 0
    polls: int = 0             # reads of the ended flags
    detections: int = 0        # detection rounds of single rows
    retired: int = 0
    row_rounds: int = 0        # rows over all rounds
    ended_row_rounds: int = 0  # of them, picks of rows that had already sampled eot (the price of polling every eos_check_interval rounds)


class ModelEngine:
    """The seam between the scheduler and the device: whisper.Model's encoder and the row mode of its text handle."""

    def __init__(self, model):
        if getattr(model, "_text", None) is None:
            raise NotImplementedError(NOT_BUILT)
        self.model, self.dims = model, model.dims
        self.tok = special_tokens(self.dims)
        self._rows = None

    def check_window(self, x) -> None:
        d = self.dims
        if len(tuple(x.shape)) != 2:
            raise ValueError("submit takes ONE window: a 2-D mel spectrogram or audio features")
        if tuple(x.shape) not in ((d.n_audio_ctx, d.n_audio_state), (2 * d.n_audio_ctx, d.n_mels)):
            raise ValueError(f"expected a mel ({2 * d.n_audio_ctx}, {d.n_mels}) or audio features ({d.n_audio_ctx}, {d.n_audio_state})")

    def open(self, max_rows: int) -> None:
        from .whisper_decoding import RowRuntime

        self._rows = RowRuntime(self.model._text, max_rows)

    def admit(self, row: int, x, init: Tuple[int, ...], options: DecodingOptions, draw: Optional[Tuple[float, int, int]] = None):
        """-> the window's audio features (n_audio_ctx, n_audio_state); a mel goes through the encoder as the solo call's would.  draw: None (the row
        picks greedily) or (temperature, seed, stream id) of a sampled row"""
        import torch

        from .whisper_decoding import _features, pick_params

        feats, _ = _features(self.model, x)
        params, bits = pick_params(self.dims, self.tok, options)
        with torch.cuda.device(self.model.device):
            self._rows.admit(row, feats[0], init, params, bits)
            if draw is not None:
                self._rows.set_draw(row, *draw)
        return feats[0]

    def forward(self, items, out_rows) -> None:
        import torch

        with torch.cuda.device(self.model.device):
            self._rows.forward(items, out_rows)

    def detect(self, row: int, out_index: int, token_index: Optional[int]) -> None:
        """detect_language's arg-maximum on row `out_index` of the round's logits, written into the row's initial tokens on the device"""
        import torch

        if token_index is None:
            return
        lo, hi = self.tok.language_tokens[0], self.tok.language_tokens[-1] + 1
        with torch.cuda.device(self.model.device):
            ids = self._rows._logits[out_index:out_index + 1][:, lo:hi].argmax(dim=-1) + lo
            self._rows.set_token(row, token_index, ids.to(torch.int32))

    def pick(self, rows: Sequence[int]) -> None:
        import torch

        with torch.cuda.device(self.model.device):
            self._rows.pick(rows)

    def flags(self) -> List[bool]:
        import torch

        with torch.cuda.device(self.model.device):
            return self._rows.flags()

    def read(self, row: int, detected: bool, sot_index: Optional[int]) -> RowRead:
        """The probabilities are decode's and detect_language's own expressions on (1, n_languages) and (1, V).  sot_index: where the prefill kept
        its logits (None: nothing was decoded).  torch's softmax over a long row reduces in an order that depends on where the row starts within 16
        bytes, so the kept row is placed as decode's view `pre[:, sot_index]` of its (1, S, V) prefill logits lies: sot_index * V floats behind an
        aligned base."""
        import torch

        tok, V = self.tok, self.dims.n_vocab
        with torch.cuda.device(self.model.device):
            toks, st, kept = self._rows.read(row, kept=True)
            out = RowRead(tokens=[int(t) for t in toks[: st.count]], count=int(st.count), sum_logprob=float(st.sum_logprob))
            if detected:
                lo, hi = tok.language_tokens[0], tok.language_tokens[-1] + 1
                probs = torch.softmax(kept[0:1][:, lo:hi], dim=-1).cpu().numpy()
                out.language_probs = {t: float(probs[0, t - lo]) for t in tok.language_tokens}
            if sot_index is not None:
                shift = sot_index * V % 4
                at_sot = torch.empty(shift + V, dtype=torch.float32, device=kept.device)[shift:].view(1, V)
                at_sot.copy_(kept[1:2])
                out.no_speech_prob = float(torch.softmax(at_sot, dim=-1)[:, tok.no_speech].cpu().numpy()[0])
        return out

    def close(self) -> None:
        self._rows = None


class _Request:
    def __init__(self, x, options: DecodingOptions, init: Tuple[int, ...], sot_index: int, limit: int, future: Future, draw=None):
        self.x, self.options, self.init, self.sot_index, self.limit, self.future = x, options, init, sot_index, limit, future
        self.draw = draw  # None: greedy; (temperature, seed, stream id): submit_sampled
        self.detect = options.language is None or options.task == "lang_id"
        self.row: Optional[int] = None
        self.phase = "detect" if self.detect else "prefill"  # -> "prefill" -> "step" -> "retire"
        self.picks = 0
        self.features = None


class WhisperBatcher:
    def __init__(self, model=None, max_rows: int = 8, eos_check_interval: int = 8, max_round_tokens: int = 256, engine=None):
        if eos_check_interval < 1:
            raise ValueError("eos_check_interval must be >= 1")
        if max_round_tokens < 1:
            raise ValueError("max_round_tokens must be >= 1")
        self.engine = engine if engine is not None else ModelEngine(model)
        self.max_rows, self.interval, self.max_round_tokens = max_rows, eos_check_interval, max_round_tokens
        self.engine.open(max_rows)
        self.stats = ServeStats()
        self._rows: List[Optional[_Request]] = [None] * max_rows
        self._queue: Deque[_Request] = deque()
        self._since_poll = 0
        self._lock = threading.Lock()       # the queue and the closed flag
        self._wake = threading.Condition(self._lock)
        self._round = threading.RLock()     # one round at a time
        self._thread: Optional[threading.Thread] = None
        self.closed = False

    # ---- submitting (any thread) ---------------------------------------------------------------------------------------------------------
    def submit(self, mel_or_features, options: DecodingOptions = DecodingOptions(), **overrides) -> Future:
        """One window (2-D) -> Future[DecodingResult].  The option checks of `decode` run here, in the caller's thread, with decode's exceptions."""
        if overrides:
            options = replace(options, **overrides)
        return self._submit(mel_or_features, verify_options(options), None)

    def submit_sampled(self, mel_or_features, options: DecodingOptions = DecodingOptions(temperature=1.0), seed: int = 0, stream: int = 0, **overrides) -> Future:
        """One window (2-D) decoded at temperature > 0 -> Future[DecodingResult]: what `model.sample(window, options, seed=seed, streams=[stream])` returns
        for it alone (`tokens`, `avg_logprob`, `no_speech_prob`, `language`, `temperature`; `language_probs` stays None), whatever else the batch runs.
        The row draws by Gumbel-max on the Philox key `seed` and the stream id `stream` in the round's ONE pick launch (kk_whisper_text_rows_set_draw,
        DESIGN 8n).  The option checks are whisper_sampling.verify_sampling_options'; `best_of` must be None or 1: groups are not built here."""
        from .whisper_sampling import verify_sampling_options

        if overrides:
            options = replace(options, **overrides)
        options = verify_sampling_options(options)
        if options.best_of not in (None, 1):
            raise NotImplementedError("best_of groups are not built in the batcher: submit_sampled takes best_of None or 1 (Model.sample runs groups)")
        if isinstance(seed, bool) or not isinstance(seed, int) or isinstance(stream, bool) or not isinstance(stream, int) or not 0 <= stream <= 0xFFFFFFFF:
            raise ValueError("seed must be an int and stream an int in 0 .. 2**32 - 1")
        return self._submit(mel_or_features, options, (float(options.temperature), seed, stream))

    def _submit(self, mel_or_features, options: DecodingOptions, draw) -> Future:
        d = self.engine.dims
        tok = special_tokens(d)
        n_ctx = d.n_text_ctx
        sample_len = options.sample_len or n_ctx // 2
        init = initial_tokens(tok, options, n_ctx, sample_len)
        sample_begin, sot_index = len(init), init.index(tok.sot)
        if sample_begin >= n_ctx:
            raise ValueError(f"{sample_begin} initial tokens leave no room in n_text_ctx = {n_ctx}")
        self.engine.check_window(mel_or_features)
        if (options.language is None or options.task == "lang_id") and not tok.multilingual:
            raise ValueError(NO_LANGUAGE_TOKENS)
        # decode picks once after the prefill and once per step i = 1 .. sample_len - 1 while sample_begin + i <= n_ctx
        limit = min(sample_len, n_ctx - sample_begin + 1)
        req = _Request(mel_or_features, options, init, sot_index, limit, Future(), draw)
        with self._lock:
            if self.closed:
                raise RuntimeError("WhisperBatcher is closed")
            self._queue.append(req)
            self._wake.notify_all()
        return req.future

    # ---- one round -------------------------------------------------------------------------------------------------------------------------
    def _live(self) -> List[_Request]:
        return [r for r in self._rows if r is not None]

    def _free(self, r: _Request) -> None:
        self._rows[r.row] = None

    def _result(self, r: _Request, rd: RowRead) -> DecodingResult:
        tok = special_tokens(self.engine.dims)
        language = None if not tok.multilingual else r.init[r.sot_index + 1]
        if r.detect:
            language = max(rd.language_probs, key=rd.language_probs.get)
        if r.options.task == "lang_id":
            return DecodingResult(audio_features=r.features, language=language, language_probs=rd.language_probs)
        seq = list(rd.tokens)
        if tok.eot in seq:
            seq = seq[: seq.index(tok.eot)]
        return DecodingResult(audio_features=r.features, language=language, tokens=seq, avg_logprob=rd.sum_logprob / (len(seq) + 1),
                              no_speech_prob=rd.no_speech_prob, temperature=r.options.temperature)

    def _retire(self, r: _Request) -> None:
        try:
            rd = self.engine.read(r.row, r.detect, r.sot_index if r.options.task != "lang_id" else None)
            res = self._result(r, rd)
        except BaseException as e:  # noqa: BLE001  (the caller sits in Future.result())
            r.future.set_exception(e)
        else:
            self.stats.ended_row_rounds += max(0, rd.count - len(res.tokens) - 1)  # picks behind the row's eot
            r.future.set_result(res)
        self.stats.retired += 1
        self._free(r)

    def _admit(self, busy_tokens: int) -> None:
        """FIFO into free rows.  A request costs its prefill in the round that runs it: this round, or the next after a detection round (which
        costs one token now); a round always takes the head of the queue when nothing else is prefilled in it."""
        now, nxt = busy_tokens, 0
        while True:
            free = [i for i, r in enumerate(self._rows) if r is None]
            with self._lock:
                if not free or not self._queue:
                    return
                r = self._queue[0]
                cost_now, cost_next = (1, len(r.init)) if r.detect else (len(r.init), 0)
                if (now and now + cost_now > self.max_round_tokens) or (nxt and nxt + cost_next > self.max_round_tokens):
                    return
                self._queue.popleft()
            if not r.future.set_running_or_notify_cancel():
                continue  # cancelled while it was queued
            try:
                if r.draw is None:
                    r.features = self.engine.admit(free[0], r.x, r.init, r.options)
                else:
                    r.features = self.engine.admit(free[0], r.x, r.init, r.options, draw=r.draw)
            except BaseException as e:  # noqa: BLE001
                r.future.set_exception(e)
                continue
            r.row, r.x = free[0], None
            self._rows[r.row] = r
            self.stats.admissions += 1
            now, nxt = now + cost_now, nxt + cost_next

    def step(self) -> bool:
        """One scheduling round; False when there was nothing to do (no live row, empty queue)."""
        with self._round:
            retired = False
            for r in self._live():
                if r.phase == "retire":
                    self._retire(r)
                    retired = True
            if self._since_poll >= self.interval and any(r.picks for r in self._live()):
                flags = self.engine.flags()
                self.stats.polls += 1
                self._since_poll = 0
                for r in self._live():
                    if r.picks and flags[r.row]:
                        self._retire(r)
                        retired = True
            self._admit(sum(len(r.init) for r in self._live() if r.phase == "prefill"))
            live = self._live()
            if not live:
                return retired
            items, out_rows, picks, detects, at = [], [], [], [], 0
            for r in live:
                n = len(r.init)
                if r.phase == "detect":  # [sot] at position 0, its logits kept in slot 0
                    items.append((r.row, 0, 1, r.sot_index, 0, 0))
                    detects.append((r, len(out_rows)))
                    out_rows.append(at)
                    at += 1
                elif r.phase == "prefill":  # the initial tokens; the logits of the sot position kept in slot 1
                    items.append((r.row, 0, n, 0, r.sot_index, 1))
                    out_rows += [at + r.sot_index] + ([at + n - 1] if r.sot_index != n - 1 else [])
                    picks.append(r)
                    at += n
                else:  # the token of the last pick at the row's own position
                    items.append((r.row, n + r.picks - 1, 1, -1, -1, 0))
                    out_rows.append(at)
                    picks.append(r)
                    at += 1
            self.engine.forward(items, out_rows)
            for r, j in detects:
                self.engine.detect(r.row, j, r.sot_index + 1 if r.options.language is None else None)
                r.phase = "retire" if r.options.task == "lang_id" else "prefill"
                self.stats.detections += 1
            if picks:
                self.engine.pick([r.row for r in picks])
            for r in picks:
                r.picks += 1
                r.phase = "retire" if r.picks >= r.limit else "step"
            self.stats.rounds += 1
            self.stats.row_rounds += len(live)
            self._since_poll += 1
            return True

    def run_until_idle(self) -> None:
        while self.step() or self._queue:
            pass

    # ---- background thread -----------------------------------------------------------------------------------------------------------------
    def start(self) -> "WhisperBatcher":
        with self._lock:
            if self.closed:
                raise RuntimeError("WhisperBatcher is closed")
            if self._thread is None:
                self._thread = threading.Thread(target=self._worker, name="whisper-batcher", daemon=True)
                self._thread.start()
        return self

    def _worker(self) -> None:
        while True:
            with self._lock:
                while not self.closed and not self._queue and not self._live():
                    self._wake.wait()
                if self.closed:
                    return
            try:
                self.step()
            except Exception as e:  # noqa: BLE001  (a failed round fails the rows in flight, the thread lives on)
                with self._round:
                    for r in self._live():
                        if not r.future.done():
                            r.future.set_exception(e)
                        self._free(r)

    def close(self) -> None:
        """Stop the worker and FAIL every request still queued or in a row (their callers sit in Future.result()).  The closed flag and the queue
        change under one lock: a submit that races close either lands in the queue before the flag, and is failed here, or sees the flag."""
        with self._lock:
            if self.closed:
                return
            self.closed = True
            self._wake.notify_all()
            thread, self._thread = self._thread, None
        if thread is not None:
            thread.join()
        with self._round:
            with self._lock:
                pending = list(self._queue)
                self._queue.clear()
            for r in pending + self._live():
                if r.future.cancelled() or r.future.done():
                    continue
                if r.row is None and not r.future.set_running_or_notify_cancel():
                    continue
                r.future.set_exception(RuntimeError("WhisperBatcher is closed"))
            self._rows = [None] * self.max_rows
            self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
