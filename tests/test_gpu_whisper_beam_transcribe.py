"""Long-form transcription with beam search and best_of groups on the device (Model.beam_transcribe, whisper_transcribe.beam_transcribe): a
file's TranscribeResult is == the result of the same call on the file alone, and == the plain restatement of the reference's loop
(tests/_whisper_transcribe_ref.py) driven by `model.beam_search` / `model.sample` per window on `embed_audio` of that window alone, with the same seed
and the stream id (seek * 16 + temperature index) % 2 ** 28.  The tiny model and the noise clips are those of tests/test_gpu_whisper_transcribe.py: with
random weights every window's average log-probability is far below the threshold, so every window is searched with the beam and then sampled as a group."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

from _whisper_transcribe_ref import transcribe_ref  # noqa: E402
from test_gpu_whisper_transcribe import SAMPLE_LEN, SEED, _setup  # noqa: E402

from mlx_audio_amd import whisper  # noqa: E402
from mlx_audio_amd import whisper_decoding as WD  # noqa: E402
from mlx_audio_amd.whisper_transcribe import TranscribeResult  # noqa: E402

TEMPS = (0.0, 0.4)
KW = dict(compression_ratio_threshold=None, temperature=TEMPS)


def _reference(m, audio, beam_size, best_of):
    """the reference's loop for one file on the window-at-a-time entry points"""
    d = m.dims
    W = 2 * d.n_audio_ctx
    tok = whisper.special_tokens(d)
    mel = whisper.log_mel_spectrogram(audio, n_mels=d.n_mels, padding=W * whisper.HOP_LENGTH)
    _, probs = m.detect_language(whisper.pad_or_trim(mel, W, axis=-2))
    language = max(probs, key=probs.get)

    def decode_window(seek, size, prompt, t):
        feats = m.embed_audio(whisper.pad_or_trim(mel[seek:seek + size], W, axis=-2))
        if t > 0:
            return m.sample(feats, WD.DecodingOptions(language=language, prompt=prompt, sample_len=SAMPLE_LEN, temperature=t, best_of=best_of), seed=SEED,
                            streams=[(seek * 16 + TEMPS.index(t)) % 2 ** 28])
        return m.beam_search(feats, WD.DecodingOptions(language=language, prompt=prompt, sample_len=SAMPLE_LEN, beam_size=beam_size))

    out = transcribe_ref(int(mel.shape[0]) - W, decode_window, W=W, n_audio_ctx=d.n_audio_ctx, timestamp_begin=tok.timestamp_begin, eot=tok.eot, **KW)
    return TranscribeResult(text=out["text"], segments=out["segments"], language=language, tokens=out["tokens"])


def test_two_files_on_six_rows_equal_each_file_alone_and_the_reference_loop():
    d, m, clips = _setup()
    files = [clips[1], clips[2]]  # two and three windows
    batch = m.beam_transcribe(files, beam_size=3, best_of=2, seed=SEED, max_rows=6, sample_len=SAMPLE_LEN, **KW)
    assert isinstance(batch, list) and len(batch) == 2
    for i, audio in enumerate(files):
        solo = m.beam_transcribe(audio, beam_size=3, best_of=2, seed=SEED, max_rows=6, sample_len=SAMPLE_LEN, **KW)
        assert isinstance(solo, TranscribeResult) and batch[i] == solo, i
        assert solo == _reference(m, audio, 3, 2), i
    temps = {s["temperature"] for r in batch for s in r.segments}
    assert temps == {0.4} and all(len(r.tokens) > 0 for r in batch)  # every window fell back from the beam to the sampled group


def test_without_beam_and_best_of_it_is_transcribe():
    d, m, clips = _setup()
    got = m.beam_transcribe(clips[1], beam_size=None, best_of=None, seed=SEED, max_rows=2, sample_len=SAMPLE_LEN, **KW)
    assert got == m.transcribe(clips[1], seed=SEED, max_rows=2, sample_len=SAMPLE_LEN, **KW)
    with pytest.raises(NotImplementedError, match="beam search is not built in transcribe"):
        m.transcribe(clips[0], beam_size=3)
    with pytest.raises(NotImplementedError, match="word_timestamps"):
        m.beam_transcribe(clips[0], word_timestamps=True)
