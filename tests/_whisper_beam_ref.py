"""A numpy restatement of the beam search of mlx-audio_amd/whisper_beam.py (OpenAI's BeamSearchDecoder with the order of equal things fixed) in
float64 on tests/_whisper_text_ref.filter_logits, with the decision margin of every step; finalize; and the seeded inputs of the GPU kernel tests, so
that tests/test_whisper_beam_cpu.py can check the margin condition on exactly what tests/test_gpu_whisper_beam_kernels.py feeds the kernels."""
import math

import numpy as np

import _whisper_text_ref as T

NEG = -np.inf
MARGIN = 1e-3  # ten times the 1e-4 the project allows on a sum of log-probabilities


def top_offers(filtered, n, eot):
    """a row's n most probable tokens over its filtered logits -> ([(token, logprob)] descending, equal ones by the lower id, never a masked one; the
    gap between the n-th and the (n + 1)-th logprob, or None without an (n + 1)-th).  Everything masked: [(eot, 0.0)]."""
    x = np.asarray(filtered, np.float64)
    ids = np.flatnonzero(x > NEG)
    if len(ids) == 0:
        return [(eot, 0.0)], None
    lse = T.logsumexp(x)
    order = ids[np.lexsort((ids, -x[ids]))][: n + 1]
    offers = [(int(t), float(x[t] - lse)) for t in order[:n]]
    gap = float(x[order[n - 1]] - x[order[n]]) if len(order) > n else None
    return offers, gap


class BeamWindow:
    """one window: K live prefixes (prefix, sum; a dead slot's sum is -inf), the finished list, and per step the parents and the decision margin"""

    def __init__(self, K, max_candidates, eot):
        self.K, self.max_candidates, self.eot = K, max_candidates, eot
        self.prefix = [[] for _ in range(K)]
        self.sums = [0.0] * K
        self.finished = []  # (tokens before eot, sum), in the order they finished
        self.complete = False
        self.steps = 0
        self.parents, self.margins, self.completes = [], [], []  # per step: the slots' parents (-1: dead), the margin, complete after it

    def live(self, j):
        return self.sums[j] != NEG

    def update(self, filtered_rows):
        """filtered_rows[j]: row j's filtered logits (V,), ignored for a dead slot -> the step's decision margin"""
        offers, gaps = [], []
        for j in range(self.K):
            o, g = top_offers(filtered_rows[j], self.K + 1, self.eot) if self.live(j) else ([], None)
            offers.append(o)
            gaps.append(g)
        return self.update_offers(offers, gaps)

    def update_offers(self, offers, row_gaps=None):
        """offers[j]: row j's [(token, logprob)] in descending order; row_gaps[j]: the gap behind row j's last offer (None: it has no next)"""
        K, eot = self.K, self.eot
        cands = []
        for j in range(K):
            if not self.live(j) or (self.steps == 0 and j > 0):  # at the first sampled position the rows of a window are one prefix: row 0 offers for all
                continue
            for r, (t, lp) in enumerate(offers[j]):
                cands.append((self.sums[j] + float(lp), j, r, int(t)))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        saved, newly, stop = [], [], -1
        for idx, c in enumerate(cands):
            stop = idx
            if c[3] == eot:
                newly.append(c)
            else:
                saved.append(c)
                if len(saved) == K:
                    break
        for c in newly:  # (already in descending score)
            if len(self.finished) < self.max_candidates:
                self.finished.append((list(self.prefix[c[1]]), c[0]))
        self.complete = len(self.finished) >= self.max_candidates
        # the margin: every adjacent pair of the walk's order that has a visited member, and the next-best token behind a visited last offer
        margin = math.inf
        for i in range(min(stop, len(cands) - 2) + 1):
            margin = min(margin, cands[i][0] - cands[i + 1][0])
        if row_gaps is not None:
            for idx, c in enumerate(cands[: stop + 1]):
                if c[2] == len(offers[c[1]]) - 1 and row_gaps[c[1]] is not None:
                    margin = min(margin, row_gaps[c[1]])
        prefix, sums, parents = [], [], []
        for k in range(K):
            if k < len(saved):
                s, j, _, t = saved[k]
                prefix.append(self.prefix[j] + [t])
                sums.append(s)
                parents.append(j)
            else:  # a dead slot
                prefix.append(self.prefix[k] + [eot])
                sums.append(NEG)
                parents.append(-1)
        self.prefix, self.sums = prefix, sums
        self.parents.append(parents)
        self.margins.append(margin)
        self.completes.append(self.complete)
        self.steps += 1
        return margin

    def finalize(self):
        """-> [(tokens, sum)]: the finished sequences, topped up to K from the live prefixes in descending sum (equal sums by the lower slot)"""
        out = [(list(t), s) for t, s in self.finished]
        for k in sorted((k for k in range(self.K) if self.live(k)), key=lambda k: (-self.sums[k], k)):
            if len(out) >= self.K:
                break
            out.append((list(self.prefix[k]), self.sums[k]))
        return out


# ---- the seeded inputs of tests/test_gpu_whisper_beam_kernels.py ---------------------------------------------------------------------------------
SMALL = dict(n_vocab=777, eot=700, blank=220, no_timestamps=710, timestamp_begin=711)  # a small odd vocabulary below 1024 with every special id inside


def topk_params(n_vocab, without_timestamps, mi=None):
    if n_vocab == SMALL["n_vocab"]:
        return dict(SMALL, max_initial_timestamp_index=-1 if mi is None else mi, without_timestamps=int(without_timestamps), suppress_blank=1)
    from mlx_audio_amd import whisper

    tok = whisper.special_tokens(T.dims(128, 2, 1, n_vocab, 100))
    return T.pick_params(tok, n_vocab, without_timestamps=without_timestamps, max_initial_timestamp_index=mi)


TOPK_VOCABS = (51865, 51866, 777)
TOPK_K = 5
TOPK_SEED = {51865: 1, 51866: 1, 777: 0}  # chosen so that the margin condition of tests/test_whisper_beam_cpu.py holds


def topk_case(n_vocab):
    """-> (P by row kind, rows): ten rows [(name, timestamps?, sampled history, suppress ids, logits float32 (V,))] on one seeded draw of N(0, 2) logits:
    timestamps on and off, first position and later, a bitmask, planted equal logits, fewer than K + 1 unmasked tokens, everything masked"""
    g = np.random.default_rng(TOPK_SEED[n_vocab])
    V = n_vocab
    P = {True: topk_params(V, False, mi=50), False: topk_params(V, True)}
    tb, eot = P[True]["timestamp_begin"], P[True]["eot"]
    base = (2.0 * g.standard_normal((10, V))).astype(np.float32)
    sup = tuple(int(t) for t in g.choice(np.arange(0, eot), size=40, replace=False))
    rows = []
    rows.append(("first, timestamps", True, [], (), base[0]))
    rows.append(("first, no timestamps", False, [], (), base[1]))
    rows.append(("after text, timestamps", True, [tb + 3, 15, 16], (), base[2]))
    rows.append(("after a timestamp pair, timestamps", True, [tb + 3, 15, tb + 7, tb + 7], (), base[3]))
    rows.append(("after one timestamp, timestamps", True, [tb + 3, 15, tb + 7], (), base[4]))
    x = base[5].copy()
    x[list(sup[:3])] += np.float32(30.0)  # suppressed ids far above the rest
    rows.append(("a bitmask", False, [15], sup, x))
    x = base[6].copy()
    top = np.argsort(-x.astype(np.float64), kind="stable")[:4]
    hi, lo = sorted(int(t) for t in top[:2])
    x[[hi, lo]] = x[top[0]]  # the two best equal: the lower id first
    x[int(top[3])] = x[int(top[2])]  # and the third and fourth
    rows.append(("planted equal logits", False, [15, 16], (), x))
    few = tuple(t for t in range(V) if t not in (5, 9, 300))
    rows.append(("three unmasked tokens", False, [15], few, base[7]))
    rows.append(("everything masked", False, [15], tuple(range(V)), base[8]))
    rows.append(("everything masked at the first position but eot and the blank", False, [], tuple(t for t in range(V) if t not in (eot, 220)), base[9]))
    return P, rows


def topk_margin(x, K, planted=False):
    """the smallest gap among the K + 2 best filtered logits (the planted equal ones aside: their order is the lower id's by construction)"""
    v = np.sort(x[x > NEG])[::-1][: K + 2]
    d = -np.diff(v)
    if planted:
        d = d[d > 0]
    return float(d.min()) if len(d) else math.inf


SELECT_KS = (1, 3, 8)
SELECT_SEED = {1: 0, 3: 99, 8: 2}  # chosen for the margin condition and for what the scripts are there to exercise
SELECT_EOT = 500
SELECT_STEPS = 5
SELECT_MAXC = {1: 1, 3: 2, 8: 12}  # K 1 and 3: a window completes by the third step and keeps stepping; K 8 runs on patience 1.5


def select_script(K):
    """-> steps[s][w][j] = [(token, logprob float32)]: 2 windows, 5 steps of seeded offers with eot at ranks that move with the step, the window and the row;
    in step 2 window 1's rows offer one token or none, so dead slots follow"""
    g = np.random.default_rng(SELECT_SEED[K])
    steps = []
    for s in range(SELECT_STEPS):
        step = []
        for w in range(2):
            rows = []
            for j in range(K):
                n = K + 1
                if s == 2 and w == 1:
                    n = 1 if j % 2 == 0 else 0
                toks = [int(t) for t in g.choice(np.arange(1, 400), size=n, replace=False)]
                lps = [float(np.float32(v)) for v in -np.sort(g.uniform(0.05, 12.0, size=n))]
                if n and (s + w + j) % 3 == 0:
                    toks[(s + j) % n] = SELECT_EOT
                rows.append(list(zip(toks, lps)))
            step.append(rows)
        steps.append(step)
    return steps


def select_replay(K):
    """the restatement over select_script(K) -> the two BeamWindows"""
    wins = [BeamWindow(K, SELECT_MAXC[K], SELECT_EOT) for _ in range(2)]
    for step in select_script(K):
        for w in range(2):
            wins[w].update_offers([o if wins[w].live(j) else [] for j, o in enumerate(step[w])])
    return wins
