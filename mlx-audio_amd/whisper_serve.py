"""Whisper serving: 30-second windows join and leave ONE running decoder batch.  `Model.decode` is a static batch -- one set of options,
one shared position, every row stepped until the last has ended; a voice service's listeners close utterances at different moments, each with its own
language, prompt, prefix and length limit.  `WhisperBatcher` keeps `max_rows` decoder rows of the text handle's row mode (kk_whisper_text_rows_*,
whisper_decoding.RowRuntime) busy.

One lifecycle.  Every request is a GROUP of G >= 1 rows on ONE projection of its window's cross K/V: a beam group (`submit_beam`, G = beam_size), or a plain
one whose rows each pick for themselves -- `submit_group`'s `best_of` rows, and the one row of `submit` (greedy) and `submit_sampled` (its row carries a
draw: 1 / T, Philox key, stream id).  A group is admitted when G rows are free (strictly FIFO: the head of the queue waits and nothing overtakes
it), prefilled in the round that steps the other rows, picked with its own parameters in the round's ONE pick launch, and retired whole -- read back,
released, all its rows free in that round -- when it has ended or reached its own limit.  The groups buffer of row mode is bound when the engine opens.

The contract: every request's `DecodingResult` equals, field by field (`tokens`, `avg_logprob`, `no_speech_prob`, `language`, `language_probs`,
`temperature`), what the solo window-mode call returns for the same 2-D input and options alone -- `model.decode` (`submit`), `model.sample(...,
streams=[stream])` (`submit_sampled`, `submit_group`), `model.beam_search` (`submit_beam`) -- whatever else the batch runs, in whatever order requests
arrive, whichever rows they land in.  The kernels give a row the bits of its solo run (a row's bits depend on that row's inputs alone); the two
probabilities are the torch expressions of `decode` / `detect_language` on the same (1, V) / (1, n_languages) shapes of bit-identical logits.  The result
is formed from the one read-back record in the solo call's own way: `submit` and `submit_sampled` as `decode` forms it from the row (`language_probs`
stays None but for `lang_id`), `submit_beam` and `submit_group` through whisper_beam.finalize, whisper_sampling.rank and results.

One round (`step`):
  1. requests that cannot go on are retired: one at its own limit (its `sample_len` and decode's `sample_begin + i > n_ctx` rule -- a row is never picked
     more often than its solo run), a `lang_id` request after its detection round and, every `eos_check_interval` rounds, those the poll finds over: every
     row's ended flag set (a beam group's rows all carry its complete flag).  Retiring reads the group back and synchronises; between polls the host
     reads nothing from the device.
  2. queued requests are admitted FIFO into free rows, `max_round_tokens` of prefill per round at the most (every row of a group prefills).
  3. ONE rows_forward over every live row: a fresh row carries its initial tokens, a leader in detection `[sot]` at position 0, the others one token.
  4. ONE rows_pick over the rows that were prefilled or stepped.
A row that has ended keeps stepping and emits eot until the next poll notices, as in `decode`.  A request with `language=None` (or `task="lang_id"`)
spends one extra round first, on its leader alone; the arg-maximum over the language tokens goes into the initial tokens of every row of the group on the
device, with no synchronisation.  `submit` keeps refusing a temperature and `submit_sampled` a `best_of` above 1, as their tests pin.
`Model.transcribe` and `Model.beam_transcribe` (whisper_transcribe.py) are the long-form loops on top of this batcher.

The scheduler talks to the model through an engine (`ModelEngine`: one entry per job, each taking the group's rows); a fake engine tests it without a
GPU.  Out of scope: `generate` (see `Model.transcribe`), text-to-id encoding, hipGraph capture of the round, prefill on a side stream, prefilling a group's
leader alone."""
from __future__ import annotations

import threading
from collections import deque
from concurrent.futures import Future
from dataclasses import dataclass, replace
from typing import Deque, Dict, List, Optional, Sequence, Tuple

from .whisper_decoding import (NOT_BUILT, DecodingOptions, DecodingResult, cut_at_eot, initial_tokens, special_tokens, verify_options)

NO_LANGUAGE_TOKENS = "This model doesn't have language tokens so it can't perform lang id"


@dataclass
class GroupRead:
    """what retiring a request reads back: TextRuntime.beam_read's lists for one window.  A plain group has nothing finished and its rows as the live
    ones, each with every token it sampled (eot and what it emitted behind it included) and its sum"""
    finished: List[Tuple[List[int], float]]
    live: List[Tuple[List[int], float]]
    no_speech_prob: float = float("nan")
    language_probs: Optional[Dict[int, float]] = None


RowRead = GroupRead  # a single row's read-back is its group's: the row is live[0]


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

    def embed_audio(self, mel):
        """Windows (R, 2 n_audio_ctx, n_mels) -> their audio features (R, n_audio_ctx, n_audio_state) in ONE encoder call; a row has the bits of
        its own B = 1 call"""
        return self.model.embed_audio(mel)

    def open(self, max_rows: int) -> None:
        from .whisper_decoding import RowRuntime

        self._rows = RowRuntime(self.model._text, max_rows)

    def admit(self, rows: Sequence[int], x, init: Tuple[int, ...], options: DecodingOptions, beam: bool = False, max_candidates: int = 1,
              draws: Optional[Sequence[Tuple[float, int, int]]] = None):
        """The window into the group `rows` on rows[0]'s cross K/V -> its audio features (n_audio_ctx, n_audio_state); a mel goes through the encoder
        as the solo call's would.  beam: a beam group (len(rows) = beam_size); else a plain one, whose row g picks greedily (draws None) or draws on
        draws[g] = (temperature, seed, stream id)"""
        import torch

        from .whisper_decoding import _features, pick_params

        feats, _ = _features(self.model, x)
        params, bits = pick_params(self.dims, self.tok, options)
        with torch.cuda.device(self.model.device):
            self._rows.admit_group(rows, beam, feats[0], init, params, bits, max_candidates)
            for row, draw in zip(rows, draws or ()):
                self._rows.set_draw(row, *draw)
        return feats[0]

    def forward(self, items, out_rows) -> None:
        import torch

        with torch.cuda.device(self.model.device):
            self._rows.forward(items, out_rows)

    def detect(self, rows: Sequence[int], out_index: int, token_index: Optional[int]) -> None:
        """detect_language's arg-maximum on row `out_index` of the round's logits (the leader's), written into the initial tokens of EVERY row of the
        group on the device"""
        import torch

        if token_index is None:
            return
        lo, hi = self.tok.language_tokens[0], self.tok.language_tokens[-1] + 1
        with torch.cuda.device(self.model.device):
            ids = (self._rows._logits[out_index:out_index + 1][:, lo:hi].argmax(dim=-1) + lo).to(torch.int32)
            for row in rows:
                self._rows.set_token(row, token_index, ids)

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

    def read(self, rows: Sequence[int], detected: bool, sot_index: Optional[int]) -> GroupRead:
        """reads the group back (the probabilities on the leader's kept rows) and releases its rows"""
        import torch

        with torch.cuda.device(self.model.device):
            finished, live, kept = self._rows.group_read(rows[0], len(rows), kept=True)
            out = GroupRead(finished=finished, live=live)
            self._probabilities(out, kept, detected, sot_index)
            self._rows.group_release(rows[0])
        return out

    def close(self) -> None:
        self._rows = None


def _checked(verify, options: DecodingOptions, overrides: dict) -> DecodingOptions:
    return verify(replace(options, **overrides) if overrides else options)


def _ints(*values) -> bool:
    return all(isinstance(v, int) and not isinstance(v, bool) for v in values)


class _Request:
    """a group of G rows: "beam" (submit_beam), or "plain" -- every row picks for itself: submit_group's best_of rows, submit's and submit_sampled's one"""

    def __init__(self, x, options: DecodingOptions, init: Tuple[int, ...], sot_index: int, limit: int, future: Future, kind: str, G: int, max_candidates: int,
                 draws, ranked: bool):
        self.x, self.options, self.init, self.sot_index, self.limit, self.future = x, options, init, sot_index, limit, future
        self.kind, self.G, self.max_candidates = kind, G, max_candidates
        self.draws = draws    # None: the rows pick greedily; else row g draws on draws[g] = (temperature, seed, stream id)
        self.ranked = ranked  # submit_beam, submit_group: the result is the ranker's choice among the group's candidates
        self.rows: List[int] = []  # once admitted; rows[0] leads
        self.detect = options.language is None or options.task == "lang_id"
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
        self.on_submit = None  # a scheduler that steps this batcher itself (csm_serve.CSMBatcher(stt=...)) is told of every new request

    # ---- submitting (any thread) ---------------------------------------------------------------------------------------------------------
    def submit(self, mel_or_features, options: DecodingOptions = DecodingOptions(), **overrides) -> Future:
        """One window (2-D) -> Future[DecodingResult].  The option checks of `decode` run here, in the caller's thread, with decode's exceptions."""
        return self._submit(mel_or_features, _checked(verify_options, options, overrides))

    def submit_sampled(self, mel_or_features, options: DecodingOptions = DecodingOptions(temperature=1.0), seed: int = 0, stream: int = 0, **overrides) -> Future:
        """One window (2-D) decoded at temperature > 0 -> Future[DecodingResult]: what `model.sample(window, options, seed=seed, streams=[stream])` returns
        for it alone (`tokens`, `avg_logprob`, `no_speech_prob`, `language`, `temperature`; `language_probs` stays None), whatever else the batch runs.
        The row draws by Gumbel-max on the Philox key `seed` and the stream id `stream` in the round's ONE pick launch (kk_whisper_text_rows_set_draw,
        DESIGN 8n).  The option checks are whisper_sampling.verify_sampling_options'; `best_of` must be None or 1: groups are not built here."""
        from .whisper_sampling import verify_sampling_options

        options = _checked(verify_sampling_options, options, overrides)
        if options.best_of not in (None, 1):
            raise NotImplementedError("best_of groups are not built in the batcher: submit_sampled takes best_of None or 1 (Model.sample runs groups)")
        if not _ints(seed, stream) or not 0 <= stream <= 0xFFFFFFFF:
            raise ValueError("seed must be an int and stream an int in 0 .. 2**32 - 1")
        return self._submit(mel_or_features, options, draws=[(float(options.temperature), seed, stream)])

    def submit_beam(self, mel_or_features, options: DecodingOptions = DecodingOptions(beam_size=5), **overrides) -> Future:
        """One window (2-D) searched with a beam -> Future[DecodingResult]: what `model.beam_search(window, options)` returns for it alone, field by
        field, on `beam_size` rows of the batch.  The option checks are whisper_beam.verify_beam_options'.  A patience below 1 that leaves
        fewer finished sequences than beams is refused: such a window completes before `beam_size` sequences have finished, the live prefixes top its
        candidates up, and they go on changing with every step behind completion -- the solo result then depends on `eos_check_interval`, so there
        is no one result to equal."""
        from .whisper_beam import max_candidates, verify_beam_options

        options = _checked(verify_beam_options, options, overrides)
        mc = max_candidates(options.beam_size, options.patience)
        if mc < options.beam_size:
            raise ValueError(f"round(beam_size * patience) = {mc} finished sequences are fewer than beam_size = {options.beam_size}: the live prefixes that "
                             "top the candidates up change with every step after completion, so the result depends on when the poll runs "
                             "(Model.beam_search takes such a patience)")
        return self._submit(mel_or_features, options, kind="beam", G=options.beam_size, max_candidates=mc, ranked=True)

    def submit_group(self, mel_or_features, options: DecodingOptions = DecodingOptions(temperature=1.0, best_of=5), seed: int = 0, stream: int = 0,
                     **overrides) -> Future:
        """One window (2-D) sampled `best_of` >= 2 times at temperature > 0 -> Future[DecodingResult]: what `model.sample(window, options, seed=seed,
        streams=[stream])` returns for it alone, on `best_of` rows of the batch; row g draws on the stream id `stream * best_of + g`, which must fit 32
        bits.  The option checks are whisper_sampling.verify_sampling_options'."""
        from .whisper_sampling import verify_sampling_options

        options = _checked(verify_sampling_options, options, overrides)
        if options.best_of is None or options.best_of < 2:
            raise ValueError("submit_group takes best_of >= 2 (one sample per window is submit_sampled)")
        if not _ints(seed, stream) or stream < 0:
            raise ValueError("seed must be an int and stream an int >= 0")
        G = options.best_of
        if stream * G + G - 1 > 0xFFFFFFFF:
            raise ValueError("a stream id times best_of must fit 32 bits")
        draws = [(float(options.temperature), seed, stream * G + g) for g in range(G)]
        return self._submit(mel_or_features, options, G=G, draws=draws, ranked=True)

    def _submit(self, mel_or_features, options: DecodingOptions, kind: str = "plain", G: int = 1, max_candidates: int = 1, draws=None, ranked: bool = False) -> Future:
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
        req = _Request(mel_or_features, options, init, sot_index, limit, Future(), kind, G, max_candidates, draws, ranked)
        with self._lock:
            if self.closed:
                raise RuntimeError("WhisperBatcher is closed")
            self._queue.append(req)
            self._wake.notify_all()
            poke = self.on_submit
        if poke is not None:
            poke()
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

    def _result(self, r: _Request, rd: GroupRead) -> DecodingResult:
        """The solo call's own host steps on what was read back.  A ranked request (submit_beam, submit_group): whisper_beam.finalize /
        whisper_sampling.rank and results.  submit's and submit_sampled's: decode's result of the one row, or lang_id's three fields."""
        from .whisper_beam import finalize
        from .whisper_sampling import SampledWindows, results

        tok = special_tokens(self.engine.dims)
        language = None if not tok.multilingual else r.init[r.sot_index + 1]
        if r.detect:
            language = max(rd.language_probs, key=rd.language_probs.get)
        if r.options.task == "lang_id":
            return DecodingResult(audio_features=r.features, language=language, language_probs=rd.language_probs)
        if r.kind == "beam":
            cands = finalize(rd.finished, rd.live, r.G)
        else:
            cands = [(cut_at_eot(seq, tok.eot), total) for seq, total in rd.live]
        if not r.ranked:
            seq, total = cands[0]
            return DecodingResult(audio_features=r.features, language=language, tokens=seq, avg_logprob=total / (len(seq) + 1),
                                  no_speech_prob=rd.no_speech_prob, temperature=r.options.temperature)
        win = SampledWindows(candidates=[cands], languages=[language], language_probs=[rd.language_probs], no_speech_probs=[rd.no_speech_prob],
                             audio_features=[r.features], single=True, temperature=float(r.options.temperature))
        return results(win, r.options.length_penalty)

    def _retire(self, r: _Request) -> None:
        try:
            rd = self.engine.read(r.rows, r.detect, r.sot_index if r.options.task != "lang_id" else None)
            res = self._result(r, rd)
        except BaseException as e:  # noqa: BLE001  (the caller sits in Future.result())
            r.future.set_exception(e)
        else:
            if not r.ranked:
                self.stats.ended_row_rounds += max(0, len(rd.live[0][0]) - len(res.tokens) - 1)  # picks behind the row's eot
            r.future.set_result(res)
        self.stats.retired += 1
        self.stats.groups_retired += r.ranked
        self._free(r)  # all its rows, in this round

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
                r.features = self.engine.admit(rows, r.x, r.init, r.options, r.kind == "beam", r.max_candidates, r.draws)
            except BaseException as e:  # noqa: BLE001
                r.future.set_exception(e)
                continue
            r.rows, r.x = list(rows), None
            for row in rows:
                self._rows[row] = r
            self.stats.admissions += 1
            if r.ranked:
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
                    items.append((r.rows[0], 0, 1, r.sot_index, 0, 0))
                    detects.append((r, len(out_rows)))
                    out_rows.append(at)
                    at += 1
                elif r.phase == "prefill":  # the initial tokens; the logits of the sot position kept in slot 1 (a group: of its leader)
                    for row in r.rows:
                        lead = row == r.rows[0]
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
                self.engine.detect(r.rows, j, token_index)
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
                if not r.rows and not r.future.set_running_or_notify_cancel():
                    continue
                r.future.set_exception(RuntimeError("WhisperBatcher is closed"))
            self._rows = [None] * self.max_rows
            self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
