"""Long-form transcription on the device (Model.transcribe, mlx-audio_amd/whisper_transcribe.py): a file's TranscribeResult is == the result of
transcribing it alone, whatever is transcribed with it, and == the plain restatement of the reference's loop (tests/_whisper_transcribe_ref.py) driven by
`model.decode` / `model.sample` per window on `embed_audio` of that window alone, with the same seed and stream ids.

A tiny model (SHAPE_A: W = 200 frames, 2-second windows) with seeded random weights on three noise clips of about 1, 3 and 5 seconds: one to three
windows.  With random weights the average log-probability of a window is near -log(n_vocab) = -10.9, far below the threshold of -1, so under the default
options every window walks the whole temperature ladder and ends on a sampled result: the sampled rows are exercised without contrivance."""
import base64
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import _whisper_ref as R  # noqa: E402
import _whisper_text_ref as T  # noqa: E402
from _whisper_transcribe_ref import transcribe_ref  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd.whisper_tokenizer import Tokenizer  # noqa: E402
from mlx_audio_amd.whisper_transcribe import TranscribeResult  # noqa: E402

SEED = 11
SAMPLE_LEN = 12
TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
_cache = {}


def _setup():
    if "m" not in _cache:
        d = T.dims(**T.SHAPE_A)
        m = whisper.Model(d).load_weights({**R.encoder_weights(d, 5), **T.decoder_weights(d, 21)})
        g = np.random.default_rng(3)
        clips = [(0.1 * g.standard_normal(n)).astype(np.float32) for n in (16000, 48000 + 800, 80000 - 1234)]
        _cache["m"] = (d, m, clips)
    return _cache["m"]


def _reference(m, audio, tokenizer=None, **kw):
    """the reference's loop for one file on the window-at-a-time entry points"""
    d = m.dims
    W = 2 * d.n_audio_ctx
    tok = whisper.special_tokens(d)
    mel = whisper.log_mel_spectrogram(audio, n_mels=d.n_mels, padding=W * whisper.HOP_LENGTH)
    _, probs = m.detect_language(whisper.pad_or_trim(mel, W, axis=-2))
    language = max(probs, key=probs.get)
    temps = kw.get("temperature", TEMPS)

    def decode_window(seek, size, prompt, t):
        feats = m.embed_audio(whisper.pad_or_trim(mel[seek:seek + size], W, axis=-2))
        if t > 0:
            return m.sample(feats, WD.DecodingOptions(language=language, prompt=prompt, sample_len=SAMPLE_LEN, temperature=t), seed=SEED,
                            streams=[(seek * 16 + list(temps).index(t)) & 0xFFFFFFFF])
        return m.decode(feats, WD.DecodingOptions(language=language, prompt=prompt, sample_len=SAMPLE_LEN))

    out = transcribe_ref(int(mel.shape[0]) - W, decode_window, W=W, n_audio_ctx=d.n_audio_ctx, timestamp_begin=tok.timestamp_begin, eot=tok.eot,
                         tokenizer=tokenizer, **kw)
    return TranscribeResult(text=out["text"], segments=out["segments"], language=language, tokens=out["tokens"])


def _check(kw, tokenizer=None, expect_sampled=None):
    """batch == solo == the reference loop, for the three clips under the options `kw`"""
    d, m, clips = _setup()
    batch = m.transcribe(clips, seed=SEED, max_rows=2, sample_len=SAMPLE_LEN, tokenizer=tokenizer, **kw)  # three files on two rows: one queues
    assert isinstance(batch, list) and len(batch) == 3
    for i, audio in enumerate(clips):
        solo = m.transcribe(audio, seed=SEED, sample_len=SAMPLE_LEN, tokenizer=tokenizer, **kw)
        assert isinstance(solo, TranscribeResult) and batch[i] == solo, i
        assert solo == _reference(m, audio, tokenizer=tokenizer, **kw), i
    temps = {s["temperature"] for r in batch for s in r.segments}
    if expect_sampled is not None:
        assert any(t > 0 for t in temps) == expect_sampled, temps
    return batch


def test_embed_audio_of_three_windows_equals_each_window_alone():
    import torch

    d, m, clips = _setup()
    W = 2 * d.n_audio_ctx
    mels = [whisper.log_mel_spectrogram(a, n_mels=d.n_mels, padding=W * whisper.HOP_LENGTH) for a in clips]
    w = whisper.mel_windows([mels[0], mels[1], mels[2]], [0, 200, 400], [100, 105, 92], W)
    together = m.embed_audio(w)
    for r in range(3):
        assert torch.equal(together[r], m.embed_audio(w[r].clone())), r


def test_the_default_ladder_walks_into_sampled_results():
    batch = _check(dict(compression_ratio_threshold=None), expect_sampled=True)
    assert [len({s["seek"] for s in r.segments}) >= 1 for r in batch] == [True] * 3 and all(r.text is None and r.language is not None for r in batch)
    assert all(len(r.tokens) > 0 for r in batch)


def test_greedy_only_keeps_the_previous_text_as_the_prompt():
    batch = _check(dict(compression_ratio_threshold=None, logprob_threshold=None), expect_sampled=False)
    assert len({s["seek"] for s in batch[2].segments}) >= 2  # several windows: the later ones were decoded on the earlier ones' tokens


def test_without_conditioning_on_previous_text():
    _check(dict(compression_ratio_threshold=None, logprob_threshold=None, condition_on_previous_text=False), expect_sampled=False)


def test_a_clip_of_the_files():
    batch = _check(dict(compression_ratio_threshold=None, clip_timestamps=[0.5, 2.0], temperature=(0.0, 0.4)))
    assert all(s["seek"] >= 50 for r in batch for s in r.segments)


def test_a_synthetic_tokenizer_with_every_threshold_on(tmp_path):
    d, m, clips = _setup()
    p = tmp_path / "vocab.tiktoken"
    eot = whisper.special_tokens(d).eot
    p.write_bytes(b"".join(base64.b64encode(bytes([32 + i % 95])) + b" " + str(i).encode() + b"\n" for i in range(eot)))
    tk = Tokenizer.from_file(str(p), d)
    batch = _check(dict(temperature=(0.0, 0.5, 1.0), initial_prompt=[1000, 1001]), tokenizer=tk, expect_sampled=True)
    assert all(isinstance(r.text, str) for r in batch) and any(r.text for r in batch)
    assert all(isinstance(s["compression_ratio"], float) for r in batch for s in r.segments)
    assert m.transcribe(clips[0], seed=SEED, sample_len=SAMPLE_LEN, tokenizer=str(p), temperature=(0.0, 0.5, 1.0), initial_prompt=[1000, 1001]) == batch[0]


def test_generate_still_raises_and_the_batcher_is_closed_behind_transcribe():
    d, m, clips = _setup()
    with pytest.raises(NotImplementedError, match="text decoder: not built"):
        m.generate(np.zeros((d.n_audio_ctx, d.n_audio_state), np.float32))
    with pytest.raises(NotImplementedError, match="word_timestamps"):
        m.transcribe(clips[0], word_timestamps=True)
    m.transcribe(clips[0], compression_ratio_threshold=None, logprob_threshold=None, sample_len=4)
    with m.serve(max_rows=1) as s:  # transcribe closed its batcher: the model serves again
        with pytest.raises(RuntimeError, match="still open"):
            m.transcribe(clips[0], compression_ratio_threshold=None)
        assert s.submit(T.features(d, 1, 2)[0], language=1, sample_len=3) is not None
