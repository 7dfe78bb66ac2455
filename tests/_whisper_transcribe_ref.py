"""The transcription loop of mlx_audio/stt/models/whisper/whisper.py:437-866 as ONE plain function in this repository's own words (numpy, no device):
the yardstick of whisper_transcribe.FileState (tests/test_whisper_transcribe_cpu.py) and, driven by `model.decode` / `model.sample` per window, of
`Model.transcribe` (tests/test_gpu_whisper_transcribe.py).  `decode_window(seek, size, prompt, temperature)` returns the window's DecodingResult; W
stands where the reference writes N_FRAMES.  Without a tokenizer `text` and `compression_ratio` are None and blank-text clearing is skipped, as
whisper_transcribe documents.  `max_windows` ends a loop that the reference would never leave."""
import zlib
from dataclasses import replace

import numpy as np

HOP_LENGTH, SAMPLE_RATE, FRAMES_PER_SECOND = 160, 16000, 100


def transcribe_ref(content_frames, decode_window, *, W, n_audio_ctx, timestamp_begin, eot, temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                   compression_ratio_threshold=2.4, logprob_threshold=-1.0, no_speech_threshold=0.6, condition_on_previous_text=True, initial_prompt=None,
                   clip_timestamps="0", tokenizer=None, max_windows=1000):
    if isinstance(clip_timestamps, str):
        clip_timestamps = [float(ts) for ts in (clip_timestamps.split(",") if clip_timestamps else [])]
    seek_points = [round(ts * FRAMES_PER_SECOND) for ts in clip_timestamps]
    if len(seek_points) == 0:
        seek_points.append(0)
    if len(seek_points) % 2 == 1:
        seek_points.append(content_frames)
    else:
        seek_points[-1] = min(content_frames, seek_points[-1])
    seek_clips = list(zip(seek_points[::2], seek_points[1::2]))
    calls = []

    def decode_with_fallback(seek, size, prompt):
        temperatures = [temperature] if isinstance(temperature, (int, float)) else temperature
        result = None
        for t in temperatures:
            calls.append((seek, size, tuple(prompt), t))
            if len(calls) > max_windows:
                raise RuntimeError("the reference loop does not end")
            result = decode_window(seek, size, list(prompt), t)
            if tokenizer is not None:
                text = tokenizer.decode(result.tokens).strip()
                tb = text.encode("utf-8")
                result = replace(result, text=text, compression_ratio=len(tb) / len(zlib.compress(tb)))
            needs_fallback = False
            if compression_ratio_threshold is not None and result.compression_ratio > compression_ratio_threshold:
                needs_fallback = True
            if logprob_threshold is not None and result.avg_logprob < logprob_threshold:
                needs_fallback = True
            if no_speech_threshold is not None and result.no_speech_prob > no_speech_threshold:
                needs_fallback = False
            if not needs_fallback:
                break
        return result

    seek = seek_clips[0][0]
    input_stride = W // n_audio_ctx
    time_precision = input_stride * HOP_LENGTH / SAMPLE_RATE
    all_tokens, all_segments, prompt_reset_since = [], [], 0
    initial_prompt_tokens = list(initial_prompt or [])
    all_tokens.extend(initial_prompt_tokens)

    for seek_clip_start, seek_clip_end in seek_clips:
        while seek < seek_clip_end:
            time_offset = float(seek * HOP_LENGTH / SAMPLE_RATE)
            segment_size = min(W, content_frames - seek, seek_clip_end - seek)
            segment_duration = segment_size * HOP_LENGTH / SAMPLE_RATE
            result = decode_with_fallback(seek, segment_size, all_tokens[prompt_reset_since:])
            tokens = np.array(result.tokens, dtype=np.int64)

            def new_segment(*, start, end, tokens):
                tokens = tokens.tolist()
                return {"seek": seek, "start": start, "end": end,
                        "text": None if tokenizer is None else tokenizer.decode([t for t in tokens if t < eot]), "tokens": tokens,
                        "temperature": result.temperature, "avg_logprob": result.avg_logprob,
                        "compression_ratio": None if tokenizer is None else result.compression_ratio, "no_speech_prob": result.no_speech_prob}

            if no_speech_threshold is not None:
                should_skip = result.no_speech_prob > no_speech_threshold
                if logprob_threshold is not None and result.avg_logprob > logprob_threshold:
                    should_skip = False
                if should_skip:
                    seek += segment_size
                    continue
            current_segments = []
            timestamp_tokens = tokens >= timestamp_begin
            single_timestamp_ending = timestamp_tokens[-2:].tolist() == [False, True]
            consecutive = np.where(np.logical_and(timestamp_tokens[:-1], timestamp_tokens[1:]))[0]
            consecutive += 1
            if len(consecutive) > 0:
                slices = consecutive.tolist()
                if single_timestamp_ending:
                    slices.append(len(tokens))
                last_slice = 0
                for current_slice in slices:
                    sliced_tokens = tokens[last_slice:current_slice]
                    start_pos = sliced_tokens[0].item() - timestamp_begin
                    end_pos = sliced_tokens[-1].item() - timestamp_begin
                    current_segments.append(new_segment(start=time_offset + start_pos * time_precision, end=time_offset + end_pos * time_precision,
                                                        tokens=sliced_tokens))
                    last_slice = current_slice
                if single_timestamp_ending:
                    seek += segment_size
                else:
                    seek += (tokens[last_slice - 1].item() - timestamp_begin) * input_stride
            else:
                duration = segment_duration
                timestamps = tokens[timestamp_tokens.nonzero()[0]]
                if len(timestamps) > 0 and timestamps[-1].item() != timestamp_begin:
                    duration = (timestamps[-1].item() - timestamp_begin) * time_precision
                current_segments.append(new_segment(start=time_offset, end=time_offset + duration, tokens=tokens))
                seek += segment_size
            for segment in current_segments:
                if segment["start"] == segment["end"] or (tokenizer is not None and segment["text"].strip() == ""):
                    segment["text"] = None if tokenizer is None else ""
                    segment["tokens"] = []
            all_segments.extend([{"id": i, **segment} for i, segment in enumerate(current_segments, start=len(all_segments))])
            all_tokens.extend([token for segment in current_segments for token in segment["tokens"]])
            if not condition_on_previous_text or result.temperature > 0.5:
                prompt_reset_since = len(all_tokens)

    tokens = all_tokens[len(initial_prompt_tokens):]
    return dict(text=None if tokenizer is None else tokenizer.decode(tokens), segments=all_segments, tokens=tokens, calls=calls)
