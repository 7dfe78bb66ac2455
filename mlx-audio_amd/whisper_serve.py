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

Groups: `submit_beam` runs a window's beam search, and `submit_group` its `best_of` samples, on G rows of the same batch -- admitted together
when G rows are free (strictly FIFO: the head of the queue waits and nothing overtakes it), on ONE projection of the window's cross K/V, stepped and
picked in the rounds and the launches of the single rows beside them, and retired together at the poll that finds a beam group complete or every row
of a plain group ended, or at the group's own limit.  The results are `model.beam_search`'s and `model.sample`'s for that window alone;
`Model.beam_transcribe` is the long-form loop that uses them.

The scheduler talks to the model through an engine (`ModelEngine`); a fake engine tests it without a GPU.  Out of scope: `generate` (see
`Model.transcribe`), text-to-id encoding, hipGraph capture of the round, prefill on a side stream, prefilling a group's leader alone."""
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
class GroupRead:
    """what retiring a group reads back: TextRuntime.beam_read's lists for one window (a plain group: nothing finished, its rows as the live ones)"""
    finished: List[Tuple[List[int], float]]
    live: List[Tuple[List[int], float]]
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
    groups: int = 0            # of the admissions, groups (submit_beam, submit_group) ...
    group_rows: int = 0        # ... and the rows they took
    groups_retired: int = 0


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

    def _probabilities(self, out, kept, detected: bool, sot_index: Optional[int]) -> None:
        """The probabilities are decode's and detect_language's own expressions on (1, n_languages) and (1, V).  sot_index: where the prefill kept
        its logits (None: nothing was decoded).  torch's softmax over a long row reduces in an order that depends on where the row starts within 16
        bytes, so the kept row is placed as decode's view `pre[:, sot_index]` of its (1, S, V) prefill logits lies: sot_index * V floats behind an
        aligned base."""
        import torch

        tok, V = self.tok, self.dims.n_vocab
        if detected:
            lo, hi = tok.language_tokens[0], tok.language_tokens[-1] + 1
            probs = torch.softmax(kept[0:1][:, lo:hi], dim=-1).cpu().numpy()
            out.language_probs = {t: float(probs[0, t - lo]) for t in tok.language_tokens}
        if sot_index is not None:
            shift = sot_index * V % 4
            at_sot = torch.empty(shift + V, dtype=torch.float32, device=kept.device)[shift:].view(1, V)
            at_sot.copy_(kept[1:2])
            out.no_speech_prob = float(torch.softmax(at_sot, dim=-1)[:, tok.no_speech].cpu().numpy()[0])

    def read(self, row: int, detected: bool, sot_index: Optional[int]) -> RowRead:
        import torch

        with torch.cuda.device(self.model.device):
            toks, st, kept = self._rows.read(row, kept=True)
            out = RowRead(tokens=[int(t) for t in toks[: st.count]], count=int(st.count), sum_logprob=float(st.sum_logprob))
            self._probabilities(out, kept, detected, sot_index)
        return out

    # ---- groups ------------------------------------------------------------------------------------------------------------------
    def admit_group(self, rows: Sequence[int], x, init: Tuple[int, ...], options: DecodingOptions, beam: bool, max_candidates: int = 1,
                    draws: Optional[Sequence[Tuple[float, int, int]]] = None):
        """`admit` for a group on rows[0]'s cross K/V.  beam: a beam group (len(rows) = beam_size); else a plain one whose row g draws on draws[g]"""
        import torch

        from .whisper_decoding import _features, pick_params

        feats, _ = _features(self.model, x)
        params, bits = pick_params(self.dims, self.tok, options)
        with torch.cuda.device(self.model.device):
            self._rows.admit_group(rows, beam, feats[0], init, params, bits, max_candidates)
            for row, draw in zip(rows, draws or ()):
                self._rows.set_draw(row, *draw)
        return feats[0]

    def detect_group(self, rows: Sequence[int], out_index: int, token_index: Optional[int]) -> None:
        """`detect` on the leader's logits; the id goes into the initial tokens of EVERY row of the group, on the device"""
        import torch

        if token_index is None:
            return
        lo, hi = self.tok.language_tokens[0], self.tok.language_tokens[-1] + 1
        with torch.cuda.device(self.model.device):
            ids = (self._rows._logits[out_index:out_index + 1][:, lo:hi].argmax(dim=-1) + lo).to(torch.int32)
            for row in rows:
                self._rows.set_token(row, token_index, ids)

    def read_group(self, rows: Sequence[int], detected: bool, sot_index: Optional[int]) -> GroupRead:
        """reads the group back (the probabilities on the leader's kept rows, as `read` takes them) and releases its rows"""
        import torch

        with torch.cuda.device(self.model.device):
            finished, live, kept = self._rows.group_read(rows[0], len(rows), kept=True)
            out = GroupRead(finished=finished, live=live)
            self._probabilities(out, kept, detected, sot_index)
            self._rows.group_release(rows[0])
        return out

    def close(self) -> None:
        self._rows = None


class _Request:
    def __init__(self, x, options: DecodingOptions, init: Tuple[int, ...], sot_index: int, limit: int, future: Future, draw=None):
        self.x, self.options, self.init, self.sot_index, self.limit, self.future = x, options, init, sot_index, limit, future
        self.draw = draw  # None: greedy; (temperature, seed, stream id): submit_sampled
        self.kind: Optional[str] = None  # "beam" (submit_beam) or "plain" (submit_group): a group of G rows; None: one row
        self.G, self.max_candidates, self.draws = 1, 1, None
        self.rows: List[int] = []
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

    def submit_beam(self, mel_or_features, options: DecodingOptions = DecodingOptions(beam_size=5), **overrides) -> Future:
        """One window (2-D) searched with a beam -> Future[DecodingResult]: what `model.beam_search(window, options)` returns for it alone, field by
        field, on `beam_size` rows of the batch.  The option checks are whisper_beam.verify_beam_options'.  A patience below 1 that leaves
        fewer finished sequences than beams is refused: such a window completes before `beam_size` sequences have finished, the live prefixes top its
        candidates up, and they go on changing with every step behind completion -- the solo result then depends on `eos_check_interval`, so there
        is no one result to equal."""
        from .whisper_beam import max_candidates, verify_beam_options

        if overrides:
            options = replace(options, **overrides)
        options = verify_beam_options(options)
        mc = max_candidates(options.beam_size, options.patience)
        if mc < options.beam_size:
            raise ValueError(f"round(beam_size * patience) = {mc} finished sequences are fewer than beam_size = {options.beam_size}: the live prefixes that "
                             "top the candidates up change with every step after completion, so the result depends on when the poll runs "
                             "(Model.beam_search takes such a patience)")
        return self._submit(mel_or_features, options, None, kind="beam", G=options.beam_size, max_candidates=mc)

    def submit_group(self, mel_or_features, options: DecodingOptions = DecodingOptions(temperature=1.0, best_of=5), seed: int = 0, stream: int = 0,
                     **overrides) -> Future:
        """One window (2-D) sampled `best_of` >= 2 times at temperature > 0 -> Future[DecodingResult]: what `model.sample(window, options, seed=seed,
        streams=[stream])` returns for it alone, on `best_of` rows of the batch; row g draws on the stream id `stream * best_of + g`, which must fit 32
        bits.  The option checks are whisper_sampling.verify_sampling_options'."""
        from .whisper_sampling import verify_sampling_options

        if overrides:
            options = replace(options, **overrides)
        options = verify_sampling_options(options)
        if options.best_of is None or options.best_of < 2:
            raise ValueError("submit_group takes best_of >= 2 (one sample per window is submit_sampled)")
        if isinstance(seed, bool) or not isinstance(seed, int) or isinstance(stream, bool) or not isinstance(stream, int) or stream < 0:
            raise ValueError("seed must be an int and stream an int >= 0")
        G = options.best_of
        if stream * G + G - 1 > 0xFFFFFFFF:
            raise ValueError("a stream id times best_of must fit 32 bits")
        draws = [(float(options.temperature), seed, stream * G + g) for g in range(G)]
        return self._submit(mel_or_features, options, None, kind="plain", G=G, draws=draws)

    def _submit(self, mel_or_features, options: DecodingOptions, draw, kind=None, G: int = 1, max_candidates: int = 1, draws=None) -> Future:
        if G > self.max_rows:
            raise ValueError(f"a group of {G} rows does not fit max_rows = {self.max_rows}")
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
        req.kind, req.G, req.max_candidates, req.draws = kind, G, max_candidates, draws
        with self._lock:
            if self.closed:
                raise RuntimeError("WhisperBatcher is closed")
            self._queue.append(req)
            self._wake.notify_all()
        return req.future

    # ---- one round -------------------------------------------------------------------------------------------------------------------------
    def _live(self) -> List[_Request]:
        """the requests in flight, each once (a group sits in G rows), by their first row"""
        out: List[_Request] = []
        for r in self._rows:
            if r is not None and not any(r is o for o in out):
                out.append(r)
        return out

    def _free(self, r: _Request) -> None:
        for row in r.rows:
            self._rows[row] = None

    def _group_result(self, r: _Request, rd: GroupRead) -> DecodingResult:
        """whisper_beam.finalize / whisper_sampling.rank and results on what the group read back: the solo calls' own host steps"""
        from .whisper_beam import finalize
        from .whisper_sampling import SampledWindows, results

        tok = special_tokens(self.engine.dims)
        language = None if not tok.multilingual else r.init[r.sot_index + 1]
        if r.detect:
            language = max(rd.language_probs, key=rd.language_probs.get)
        if r.kind == "beam":
            cands = finalize(rd.finished, rd.live, r.G)
        else:
            cands = [(seq[: seq.index(tok.eot)] if tok.eot in seq else list(seq), total) for seq, total in rd.live]
        win = SampledWindows(candidates=[cands], languages=[language], language_probs=[rd.language_probs], no_speech_probs=[rd.no_speech_prob],
                             audio_features=[r.features], single=True, temperature=float(r.options.temperature))
        return results(win, r.options.length_penalty)

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

    def _retire_group(self, r: _Request) -> None:
        try:
            res = self._group_result(r, self.engine.read_group(r.rows, r.detect, r.sot_index))
        except BaseException as e:  # noqa: BLE001  (the caller sits in Future.result())
            r.future.set_exception(e)
        else:
            r.future.set_result(res)
        self.stats.retired += 1
        self.stats.groups_retired += 1
        self._free(r)  # all its rows, in this round

    def _retire(self, r: _Request) -> None:
        if r.kind is not None:
            return self._retire_group(r)
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
                if r.future.cancelled():  # (a cancelled group must not hold the queue up while it waits for rows it will never take)
                    self._queue.popleft()
                    r.future.set_running_or_notify_cancel()
                    continue
                if len(free) < r.G:
                    return  # a group needs its G rows at once; the head of the queue waits and nothing overtakes it
                prefill = len(r.init) * r.G  # every row of a group prefills; the detection round runs on the leader alone
                cost_now, cost_next = (1, prefill) if r.detect else (prefill, 0)
                if (now and now + cost_now > self.max_round_tokens) or (nxt and nxt + cost_next > self.max_round_tokens):
                    return
                self._queue.popleft()
            if not r.future.set_running_or_notify_cancel():
                continue  # cancelled while it was queued
            rows = free[: r.G]
            try:
                if r.kind is not None:
                    r.features = self.engine.admit_group(rows, r.x, r.init, r.options, r.kind == "beam", r.max_candidates, r.draws)
                elif r.draw is None:
                    r.features = self.engine.admit(free[0], r.x, r.init, r.options)
                else:
                    r.features = self.engine.admit(free[0], r.x, r.init, r.options, draw=r.draw)
            except BaseException as e:  # noqa: BLE001
                r.future.set_exception(e)
                continue
            r.row, r.rows, r.x = rows[0], list(rows), None
            for row in rows:
                self._rows[row] = r
            self.stats.admissions += 1
            if r.kind is not None:
                self.stats.groups += 1
                self.stats.group_rows += r.G
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
                    # (a beam group's rows all carry its complete flag; a plain group is over when every row has ended)
                    if r.picks and all(flags[row] for row in r.rows):
                        self._retire(r)
                        retired = True
            self._admit(sum(len(r.init) * r.G for r in self._live() if r.phase == "prefill"))
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
                elif r.phase == "prefill":  # the initial tokens; the logits of the sot position kept in slot 1 (a group: of its leader)
                    for row in r.rows:
                        lead = row == r.row
                        items.append((row, 0, n, 0, r.sot_index if lead else -1, 1 if lead else 0))
                        out_rows += ([at + r.sot_index] if lead else []) + ([at + n - 1] if r.sot_index != n - 1 or not lead else [])
                        at += n
                    picks.append(r)
                else:  # the token of the last pick at the row's own position
                    for row in r.rows:
                        items.append((row, n + r.picks - 1, 1, -1, -1, 0))
                        out_rows.append(at)
                        at += 1
                    picks.append(r)
            self.engine.forward(items, out_rows)
            for r, j in detects:
                token_index = r.sot_index + 1 if r.options.language is None else None
                if r.kind is not None:
                    self.engine.detect_group(r.rows, j, token_index)
                else:
                    self.engine.detect(r.row, j, token_index)
                r.phase = "retire" if r.options.task == "lang_id" else "prefill"
                self.stats.detections += 1
            if picks:
                self.engine.pick([row for r in picks for row in r.rows])
            for r in picks:
                r.picks += 1
                r.phase = "retire" if r.picks >= r.limit else "step"
            self.stats.rounds += 1
            self.stats.row_rounds += sum(len(r.rows) for r in live)
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
