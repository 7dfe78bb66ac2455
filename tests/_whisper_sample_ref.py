"""The sampled pick of the Whisper text side (csrc/kk_whisper_text_kernels.hip, kk_op_whisper_pick_sampled) restated in numpy: Philox4x32-10 in exact
integer arithmetic (vectorised `_sampler_ref.philox4`), the uniform mapping `philox_open`, Gumbel scores in float64 on `_whisper_text_ref.filter_logits`,
the admissible set of a draw, a `SampledRow` mirroring `GreedyRow`, and the ranker.  Also the inputs of the GPU kernel tests, so that the CPU test can
evaluate the cap on draws with more than one admissible token on exactly those inputs.

The random contract: u_i = philox_open(word i & 3 of philox4(seed, stream << 32 | count, i >> 2)), philox_open(r) = ((r >> 9) + 0.5) 2^-23; the token is
argmax_i (l_i / T - log(-log u_i)) over the unmasked i, lowest index on ties; logprob = l[token] - logsumexp(l) on the untempered filtered logits."""
import math

import numpy as np

import _whisper_text_ref as T

M32 = np.uint64(0xFFFFFFFF)
CAP = 0.02  # at most this share of a test's draws may have more than one admissible token


def philox4_vec(seed, ctr, subs):
    """`_sampler_ref.philox4` for an array of `sub` words: -> uint64 (4, n) holding 32-bit words"""
    subs = np.asarray(subs, np.uint64)
    c = [np.full(subs.shape, (ctr >> s) & 0xFFFFFFFF, np.uint64) for s in (0, 32)] + [subs & M32, np.full(subs.shape, 0x4B4B5352, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]  # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c)


def philox_open(r):
    """((r >> 9) + 0.5) 2^-23 in float32: a 23-bit integer plus a half is exact, the value lies in [2^-24, 1 - 2^-24]"""
    r = np.asarray(r, np.uint64)
    return (((r >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)).astype(np.float32)


def philox_unit_f32(r):
    """kk_philox.h's philox_unit as float32 evaluates it (NOT used by the pick: it returns 1.0 for the top values of r)"""
    r = np.asarray(r, np.uint64)
    return (((r >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def uniforms(seed, stream, count, ids):
    """u_i of the draw (seed, stream, count) for the token ids `ids`, float32"""
    ids = np.asarray(ids, np.int64)
    w = philox4_vec(int(seed), ((int(stream) & 0xFFFFFFFF) << 32) | (int(count) & 0xFFFFFFFF), ids >> 2)
    return philox_open(w[ids & 3, np.arange(ids.size)])


def draw(filtered, temperature, seed, stream, count):
    """-> (admissible token ids as a sorted list, the float64 arg-maximum) of one draw on the filtered logits (float64, -inf at masked ids); ([], None) when
    every token is masked.  Admissible: every token whose float64 score is within delta = 64 2^-24 max(1, max|l| / T + 18) of the float64 maximum -- 64 units of
    float32 rounding at the scores' largest magnitude cover the device's 1 / T multiply and its two logf; 18 bounds |g| (-2.81 .. 16.64)."""
    x = np.asarray(filtered, np.float64)
    ids = np.nonzero(np.isfinite(x))[0]
    if ids.size == 0:
        return [], None
    t = float(np.float32(temperature))
    u = uniforms(seed, stream, count, ids).astype(np.float64)
    score = x[ids] / t - np.log(-np.log(u))
    best = score.max()
    delta = 64.0 * 2.0 ** -24 * max(1.0, float(np.abs(x[ids]).max()) / t + 18.0)
    return [int(i) for i in ids[score >= best - delta]], int(ids[int(np.argmax(score))])


class SampledRow:
    """GreedyDecoder.update (decoding.py:260-278) for one row at temperature > 0, following the tokens it is GIVEN (the device's), or its own arg-maximum"""

    def __init__(self, eot, temperature, seed, stream):
        self.eot, self.temperature, self.seed, self.stream = eot, temperature, seed, stream
        self.sampled, self.sum_logprob, self.ended = [], 0.0, False
        self.draws = self.multi = 0  # draws of the row while it had not ended, and those of them with more than one admissible token

    def draw(self, filtered):
        return draw(filtered, self.temperature, self.seed, self.stream, len(self.sampled))

    def update(self, filtered, token=None):
        """token None: the restatement's own choice.  -> the admissible set of this draw (None for an ended row, whose token is eot whatever was drawn)"""
        adm, best = self.draw(filtered)
        if token is None:
            token = self.eot if best is None else best
        lp = 0.0 if best is None else float(filtered[token] - T.logsumexp(filtered))
        was_ended = self.ended
        if self.ended:
            token = self.eot
        else:
            self.sum_logprob += lp
            self.draws += 1
            self.multi += len(adm) > 1
        self.sampled.append(int(token))
        self.ended = self.ended or token == self.eot
        return None if was_ended else (adm if best is not None else [self.eot])


def rank(candidates, length_penalty):
    """MaximumLikelihoodRanker (decoding.py:165-188), lowest index on ties; a zero-length candidate under None scores -inf"""
    scores = []
    for tokens, logprob in candidates:
        n = len(tokens)
        if length_penalty is None:
            scores.append(-math.inf if n == 0 else logprob / n)
        else:
            scores.append(logprob / ((5 + n) / 6) ** length_penalty)
    return int(np.argmax(scores))


# ---- the inputs of tests/test_gpu_whisper_sample_kernels.py ---------------------------------------------------------------------------------------
PICK_SEED, PICK_STREAMS = 11, (5, 0, 7, 123456)
PICK_CASES = [(51865, 50), (51866, None)]  # (n_vocab, max_initial_timestamp_index): the greedy pick test's
PICK_TEMPERATURES = (0.2, 1.0)


def pick_script(tok, n_vocab, mi):
    """the existing pick test's scripted 8-step walk of the timestamp branches (tests/test_gpu_whisper_text_kernels.py), with its generator and suppress list"""
    from test_gpu_whisper_text_kernels import _script

    sup = (tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm, tok.no_speech, 1500)
    return _script(tok, n_vocab, np.random.default_rng(n_vocab), mi), sup


DIST_V, DIST_ROWS, DIST_STEPS, DIST_SEED = 51865, 32, 64, 3
DIST_IDS = (17, 300, 1024, 4097, 20000, 33333, 50000, 51864)


def dist_logits():
    """fixed logits: the 8 ids that stay unmasked 0.3 apart (probabilities 0.04 .. 0.33 at T = 1 and 2e-5 .. 0.78 at T = 0.2), everything else N(0, 4) --
    thousands of ids above all eight -- and masked through the bitmask (eot and the blank among it)"""
    x = (4.0 * np.random.default_rng(DIST_SEED).standard_normal(DIST_V)).astype(np.float32)
    x[list(DIST_IDS)] = np.float32(0.3) * np.arange(len(DIST_IDS), dtype=np.float32)
    return x


def dist_suppress():
    return tuple(i for i in range(DIST_V) if i not in DIST_IDS)


def masked_logits(V, sup, seed):
    """N(0, 1) logits with the suppressed ids 30 above everything else"""
    x = np.random.default_rng(seed).standard_normal(V).astype(np.float32)
    x[list(sup)] += np.float32(30.0)
    return x
