"""PCM formats at both audio edges of `CSMBatcher` (`listen(format=)`, `submit(..., format=)`) against a scripted engine (no
device).  The scripted resampler is the sample-and-hold of test_csm_rates_cpu.py with the byte surface of `resample.RowResampler`: it decodes
what a row reads and encodes what it writes with `pcm.py`, and logs the dtype and width of every upload; the scripted converter does the
same for rows at the model's rate.  Checked: a listener's codes and steps equal those of an f32 listener fed the decoded floats, whatever the
slicing; the odd-byte refusal; that limits and counts are in samples; that a request's chunks concatenate to `pcm.encode` of the audio it
yields without a format; and that without a format nothing new is made."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _resample_ref as R  # noqa: E402
from test_csm_interrupt_cpu import N_CB, SPF, Decoder as _Decoder, _batcher  # noqa: E402
from test_csm_rates_cpu import M_FRAMES, MAX_FRAMES, SR, Encoder as _Encoder, Engine as _Engine, Resampler as _Resampler, _marks_of  # noqa: E402

from mlx_audio_amd import pcm  # noqa: E402
from mlx_audio_amd.sesame import Segment  # noqa: E402

SCALE = 1.0 / 64  # the scripted codec's samples are sums of small integers: scaled into (-1, 1), where the formats differ


def _row_bytes(x, row):
    return x[row].contiguous().view(torch.uint8).numpy()


class Resampler(_Resampler):
    """The byte surface: while a row has a format, `step` takes x as bytes and returns bytes."""

    def set_row(self, row, src, dst, in_format=None, out_format=None):
        super().set_row(row, src, dst)
        self.rows[row].update(fi=in_format or "f32", fo=out_format or "f32")
        self.engine.calls.append(("rs_formats", row, in_format, out_format))

    @property
    def byte_mode(self):
        return any(st is not None and (st["fi"], st["fo"]) != ("f32", "f32") for st in self.rows)

    def out_view(self, y, row):
        return y[row] if y.dtype == torch.float32 else y[row].view(pcm.torch_dtype(self.rows[row]["fo"]))

    def step(self, x, n_in, flush):
        self.engine.calls.append(("rs_x", str(x.dtype), tuple(x.shape)))
        if not self.byte_mode:
            return super().step(x, n_in, flush)
        assert x.shape[0] == self.max_rows and (x.dtype != torch.uint8 or x.shape[1] % 16 == 0)  # (another dtype is taken as its bytes and padded)
        xf = torch.zeros((self.max_rows, max(1, max(n_in))), dtype=torch.float32)
        for r in range(self.max_rows):
            if n_in[r]:
                fi = self.rows[r]["fi"]
                xf[r, : n_in[r]] = torch.from_numpy(pcm.decode(_row_bytes(x, r)[: n_in[r] * pcm.bytes_per_sample(fi)].tobytes(), fi))
        y, n_out = super().step(xf, n_in, flush)
        width = max([16] + [n_out[r] * pcm.bytes_per_sample(self.rows[r]["fo"]) for r in range(self.max_rows) if n_out[r]])
        yb = torch.full((self.max_rows, -(-width // 16) * 16), 0xEE, dtype=torch.uint8)
        for r in range(self.max_rows):
            if n_out[r]:
                e = pcm.encode(y[r, : n_out[r]].numpy(), self.rows[r]["fo"])
                yb[r, : e.nbytes] = torch.from_numpy(e.view(np.uint8).copy())
        return yb, n_out


class Converter:
    """The surface of `pcm.RowConverter`."""

    def __init__(self, engine):
        self.engine, self.closed = engine, False

    def convert(self, x, in_formats, out_formats, n):
        assert not self.closed and len(in_formats) == len(out_formats) == len(n) == x.shape[0]
        self.engine.calls.append(("convert", str(x.dtype), tuple(in_formats), tuple(out_formats), tuple(n)))
        width = max([16] + [k * pcm.bytes_per_sample(f) for k, f in zip(n, out_formats)])
        y = torch.full((x.shape[0], -(-width // 16) * 16), 0xEE, dtype=torch.uint8)
        for r, k in enumerate(n):
            if k:
                a = pcm.decode(_row_bytes(x, r)[: k * pcm.bytes_per_sample(in_formats[r])].tobytes(), in_formats[r])
                e = pcm.encode(a, out_formats[r])
                y[r, : e.nbytes] = torch.from_numpy(e.view(np.uint8).copy())
        return y

    def close(self):
        self.closed = True


class Encoder(_Encoder):
    """A frame's codes are [its first sample as a 16-bit linear value, its index + 1]."""

    def step(self, pcm_, active):
        return super().step(pcm_ * 32768.0, active)


class Decoder(_Decoder):
    def step(self, codes, active):
        return super().step(codes, active) * SCALE


class Engine(_Engine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.converters = []

    def row_encoder(self, max_batch, max_frames, max_chunk):
        self.enc = Encoder(self, max_batch, max_frames, max_chunk)
        return self.enc

    def row_resampler(self, max_rows, max_in):
        self.resamplers.append(Resampler(self, max_rows, max_in))
        return self.resamplers[-1]

    def pcm_converter(self):
        self.converters.append(Converter(self))
        return self.converters[-1]

    def decode(self, codes):
        return super().decode(codes) * SCALE

    def row_decoder(self, max_batch, max_frames, max_chunk):
        return Decoder(self, max_batch)


def _listen_batcher(eng, rows=2, **kw):
    return _batcher(eng, listen_rows=rows, listen_chunk_frames=M_FRAMES, listen_max_frames=MAX_FRAMES, **kw)


def _wave(tag, n):
    """n float samples in (-1, 1) that differ from one another"""
    return (0.9 * np.sin(0.37 * (np.arange(n) + 17 * tag))).astype(np.float32)


def _feed(bat, lis, data, how, unit):
    """`data` (bytes) in the slicing `how`; unit: bytes per sample."""
    if how == "at_once":
        lis.feed(data)
        bat.run_until_idle()
        return
    k = (1 if how == "ones" else 7) * unit
    for i in range(0, len(data), k):
        piece = data[i : i + k]
        lis.feed(bytearray(piece) if (i // k) % 2 else memoryview(piece))
        bat.step()


def _heard(rate, fmt, n, how, tag=3):
    """(ListenResult, what the encoder row was fed, the engine) of one listener fed n samples of _wave in `fmt` at `rate`."""
    eng = Engine()
    bat = _listen_batcher(eng, rows=1)
    lis = bat.listen(sample_rate=rate, format=fmt)
    stored = pcm.encode(_wave(tag, n), fmt)
    if fmt is None:
        if how == "at_once":
            lis.feed(stored)
            bat.run_until_idle()
        else:
            k = 1 if how == "ones" else 7
            for i in range(0, n, k):
                lis.feed(stored[i : i + k])
                bat.step()
    else:
        _feed(bat, lis, stored.tobytes(), how, stored.itemsize)
    fut = lis.end()
    bat.run_until_idle()
    res = fut.result(timeout=0)
    fed = np.array(eng.enc.fed[0], np.float32)
    bat.close()
    return res, fed, eng


# ---- in: listeners ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fmt,n", [(8000, "mulaw", 35), (None, "s16le", 7 * SPF + 2), (16000, "alaw", 41), (None, "mulaw", 4 * SPF)])
@pytest.mark.parametrize("how", ["at_once", "ones", "sevens"])
def test_codes_and_steps_are_those_of_an_f32_listener_fed_the_decoded_floats(rate, fmt, n, how):
    res, fed, eng = _heard(rate, fmt, n, how)
    # the f32 twin is fed pcm.decode(the bytes): the same stored samples, decoded on the host
    e2 = Engine()
    b2 = _listen_batcher(e2, rows=1)
    l2 = b2.listen(sample_rate=rate)
    l2.feed(pcm.decode(pcm.encode(_wave(3, n), fmt), fmt))
    f2 = l2.end()
    b2.run_until_idle()
    want = f2.result(timeout=0)
    assert res.steps == want.steps and res.frames == want.frames and res.samples == want.samples == n  # samples, not bytes
    assert res.format == fmt and want.format == "f32" and res.sample_rate == want.sample_rate == (rate or SR)
    np.testing.assert_array_equal(res.codes.numpy(), want.codes.numpy())
    assert np.abs(res.codes.numpy()[0]).max() > 1000  # the codes carry the samples' 16-bit values: the comparison says something
    np.testing.assert_array_equal(fed, np.array(e2.enc.fed[0], np.float32))  # the encoder saw the same floats, padding included
    assert [c[0] for c in eng.enc.calls] == res.steps
    unit = pcm.bytes_per_sample(fmt)
    if rate is not None:  # decoded inside the resampler step: bytes up, 1 per sample for the G.711 formats; no converter
        assert not eng.converters and len(eng.resamplers) == 1
        assert _marks_of(eng, "rs_formats") == [("rs_formats", 0, fmt, None)]
        ups = _marks_of(eng, "rs_x")
        assert all(u[1] == "torch.uint8" and u[2][1] % 16 == 0 for u in ups)
        if how == "at_once":
            assert ups[0][2] == (1, -(-n * unit // 16) * 16)  # the round uploads the bytes it was fed, once
    else:         # at the model's rate: one convert launch per round into the row's device buffer; no resampler
        assert not eng.resamplers and len(eng.converters) == 1 and eng.converters[0].closed
        conv = _marks_of(eng, "convert")
        assert all(c[1] == "torch.uint8" and c[2] == (fmt,) and c[3] == ("f32",) for c in conv) and sum(c[4][0] for c in conv) == n
        if how == "at_once":
            assert len(conv) == 1
    b2.close()


def test_an_odd_number_of_s16le_bytes_is_refused_and_nothing_changes():
    eng = Engine()
    bat = _listen_batcher(eng, rows=2)
    a, b = bat.listen(format="s16le"), bat.listen(sample_rate=16000, format="s16le")
    stored = pcm.encode(_wave(1, 4 * SPF), "s16le")
    for lis in (a, b):
        lis.feed(stored[:5].tobytes())
        with pytest.raises(ValueError, match="whole number"):
            lis.feed(stored[5:9].tobytes()[:-1])
        assert lis.samples == 5
        with pytest.raises(ValueError, match="int16"):
            lis.feed(_wave(1, 4))  # floats into an s16le listener
        lis.feed(stored[5:])       # an array of the format's dtype is taken as it is
        assert lis.samples == 4 * SPF
    with pytest.raises(ValueError, match="unknown PCM format"):
        bat.listen(format="s16be")
    fa = a.end()
    bat.run_until_idle()
    np.testing.assert_array_equal(np.array(eng.enc.fed[0], np.float32) / 32768.0, pcm.decode(stored, "s16le"))
    assert fa.result(timeout=0).frames == 4
    bat.close()


@pytest.mark.parametrize("fmt", ["s16le", "mulaw"])
def test_the_feed_limit_counts_samples_not_bytes(fmt):
    eng = Engine()
    bat = _listen_batcher(eng)
    cap = MAX_FRAMES * SPF
    same, up = bat.listen(format=fmt), bat.listen(sample_rate=8000, format=fmt)
    unit = pcm.bytes_per_sample(fmt)
    same.feed(bytes(unit * (cap - 1)))
    same.feed(bytes(unit))
    with pytest.raises(ValueError, match="listen_max_frames"):
        same.feed(bytes(unit))
    assert same.samples == cap
    up.feed(bytes(unit * (cap // 3)))  # out_len = cap exactly
    with pytest.raises(ValueError, match="listen_max_frames"):
        up.feed(bytes(unit))
    assert up.samples == cap // 3
    fs, fu = same.end(), up.end()
    bat.run_until_idle()
    assert (fs.result(timeout=0).frames, fs.result(timeout=0).samples) == (MAX_FRAMES, cap)
    assert (fu.result(timeout=0).frames, fu.result(timeout=0).samples) == (MAX_FRAMES, cap // 3)
    bat.close()


def test_a_sessions_heard_turn_in_mulaw_enters_as_its_hear_twin():
    eng = Engine()
    bat = _listen_batcher(eng)
    sess = bat.session()
    lis = sess.listen(speaker=1, sample_rate=8000, format="mulaw")
    stored = pcm.encode(_wave(5, 33), "mulaw")
    for i in range(0, 33, 4):
        lis.feed(stored[i : i + 4].tobytes())
        bat.step()
    fut = lis.end([9, 9])
    bat.run_until_idle()
    res = fut.result(timeout=0)
    e2 = Engine()
    b2 = _listen_batcher(e2)
    l2 = b2.listen(speaker=1, sample_rate=8000)
    l2.feed(pcm.decode(stored, "mulaw"))
    f2 = l2.end()
    b2.run_until_idle()
    np.testing.assert_array_equal(res.codes.numpy(), f2.result(timeout=0).codes.numpy())
    heard = eng.heard[-1]  # Segment.audio: the decoded signal at the model's rate, float32, not padded
    assert heard.dtype == np.float32 and heard.shape[0] == R.out_len(33, 3, 1)
    twin = b2.session()
    twin.hear(Segment(1, [9, 9], heard), codes=res.codes.numpy())
    assert twin.turns == sess.turns and twin.length == sess.length
    for x, y in zip(sess.pending + sess.history, twin.pending + twin.history):
        np.testing.assert_array_equal(x, y)
    bat.close(); b2.close()


# ---- out: requests ---------------------------------------------------------------------------------------------------------------------------
def _run(rate, fmt, frames, stream, interrupt=None, steps=None):
    eng = Engine()
    bat = _batcher(eng, stream_chunk_frames=3)
    kw = dict(max_audio_length_ms=80 * frames, voice_match=False, sample_rate=rate, format=fmt)
    h = (bat.submit_stream if stream else bat.submit)(None, [3, 3, 5], **kw)
    other = bat.submit_stream(None, [3, 3, 2], max_audio_length_ms=80 * 5, voice_match=False)  # a row without a format in the same rounds
    if steps is not None:
        for _ in range(steps):
            assert bat.step()
        assert bat.interrupt(h, **interrupt)
    bat.run_until_idle()
    chunks = list(h) if stream else None
    res = h.result(timeout=0)
    ro = other.result(timeout=0)
    assert ro.format == "f32" and ro.audio.dtype == torch.float32 and all(c.format == "f32" and c.audio.dtype == torch.float32 for c in other)
    bat.close()
    return chunks, res, eng


@pytest.mark.parametrize("rate", [None, 8000, 48000])
@pytest.mark.parametrize("fmt", ["s16le", "mulaw", "alaw"])
@pytest.mark.parametrize("frames", [7, 9])  # a remainder chunk; a length that is a multiple of the chunk
def test_chunks_concatenate_to_the_encoded_whole(rate, fmt, frames):
    chunks, res, eng = _run(rate, fmt, frames, True)
    ref_chunks, ref, ref_eng = _run(rate, None, frames, True)
    want = pcm.encode(ref.audio.numpy(), fmt)
    if rate != 8000:  # (the scripted hold reads 30 samples ahead at 1 / 3: these short clips come out as zeros there, as in the f32 tests)
        assert len(np.unique(want)) > 3  # the scripted audio is inside (-1, 1): the encoding is not the clamp
    assert [(c.first_frame, c.frames, c.final) for c in chunks] == [(c.first_frame, c.frames, c.final) for c in ref_chunks]
    assert [c.audio.shape[0] for c in chunks] == [c.audio.shape[0] for c in ref_chunks]
    assert all(c.format == fmt and c.audio.dtype == pcm.torch_dtype(fmt) for c in chunks)
    np.testing.assert_array_equal(torch.cat([c.audio for c in chunks]).numpy(), want)
    assert res.format == fmt and res.audio.dtype == pcm.torch_dtype(fmt) and res.sample_rate == (rate or SR) and res.frames == frames
    np.testing.assert_array_equal(res.audio.numpy(), want)
    if rate is None:  # one convert launch per decode round; no resampler
        assert not eng.resamplers and len(eng.converters) == 1
        assert all(c[2] == ("f32", "f32") and set(c[3]) == {"f32", fmt} for c in _marks_of(eng, "convert"))
        assert len(_marks_of(eng, "convert")) == len(chunks)
    else:             # encoded in the decode round's resampler step: no converter, no step more than the f32 run takes
        assert not eng.converters and len(eng.resamplers) == 1
        assert _marks_of(eng, "rs_formats") == [("rs_formats", 0, None, fmt)]
        assert _marks_of(eng, "rs_step") == _marks_of(ref_eng, "rs_step")


@pytest.mark.parametrize("rate", [None, 48000])
@pytest.mark.parametrize("fmt", ["s16le", "alaw"])
def test_a_plain_request(rate, fmt):
    _, res, eng = _run(rate, fmt, 6, False)
    _, ref, ref_eng = _run(rate, None, 6, False)
    assert res.format == fmt and ref.format == "f32" and res.sample_rate == (rate or SR)
    np.testing.assert_array_equal(res.audio.numpy(), pcm.encode(ref.audio.numpy(), fmt))
    if rate is None:
        assert not eng.resamplers and _marks_of(eng, "convert") == [("convert", "torch.float32", ("f32",), (fmt,), (6 * SPF,))]
    else:  # through the same one-row object as the f32 clip: one whole-clip step with the flush
        assert not eng.converters and [(r.max_rows, r.max_in) for r in eng.resamplers] == [(1, 1 << 30)]
        assert _marks_of(eng, "rs_step") == _marks_of(ref_eng, "rs_step") == [("rs_step", (6 * SPF,), (True,))]
    with pytest.raises(ValueError, match="decode=False"):
        _batcher(Engine(), decode=False).submit(None, [3, 3, 5], voice_match=False, format="mulaw")
    with pytest.raises(ValueError, match="unknown PCM format"):
        _batcher(Engine()).submit(None, [3, 3, 5], voice_match=False, format="s24le")


@pytest.mark.parametrize("rate,played,kept", [(48000, 14, 3), (8000, 3, 3), (None, 14, 5)])
def test_played_samples_go_on_counting_samples(rate, played, kept):
    """14 samples of s16le are 28 bytes; the count the caller gives is in samples at the request's rate, as without a format."""
    _, res, _ = _run(rate, "s16le", 30, False, interrupt=dict(played_samples=played), steps=8)
    _, ref, _ = _run(rate, None, 30, False, interrupt=dict(played_samples=played), steps=8)
    assert res.interrupted and res.frames == ref.frames == kept
    np.testing.assert_array_equal(res.audio.numpy(), pcm.encode(ref.audio.numpy(), "s16le"))


@pytest.mark.parametrize("rate", [None, 48000])
@pytest.mark.parametrize("cut", [dict(played_frames=4), dict(played_frames=2), dict(played_frames=3)])
def test_an_interrupted_streaming_request(rate, cut):
    """Cut behind, inside and exactly at the end of what was sent (3 frames): the §8d-10 rules carry over -- the result is the encoding of the
    f32 run's result in every case; the chunks add up to it unless the cut lies inside a chunk already sent."""
    chunks, res, _ = _run(rate, "mulaw", 40, True, interrupt=cut, steps=6)
    ref_chunks, ref, _ = _run(rate, None, 40, True, interrupt=cut, steps=6)
    assert res.interrupted and res.frames == ref.frames == cut["played_frames"]
    assert [(c.first_frame, c.frames, c.final, c.audio.shape[0]) for c in chunks] == [(c.first_frame, c.frames, c.final, c.audio.shape[0]) for c in ref_chunks]
    assert all(c.format == "mulaw" and c.audio.dtype == torch.uint8 for c in chunks)
    for c, r in zip(chunks, ref_chunks):
        if rate is None:  # element-wise: every chunk is the encoding of its f32 twin
            np.testing.assert_array_equal(c.audio.numpy(), pcm.encode(r.audio.numpy(), "mulaw"))
    np.testing.assert_array_equal(res.audio.numpy(), pcm.encode(ref.audio.numpy(), "mulaw"))
    if cut["played_frames"] != 2:
        np.testing.assert_array_equal(torch.cat([c.audio for c in chunks]).numpy(), res.audio.numpy())


# ---- no format: nothing changes --------------------------------------------------------------------------------------------------------------
def test_without_a_format_no_converter_is_made_and_no_resampler_more():
    eng = Engine()
    bat = _listen_batcher(eng, stream_chunk_frames=3)
    lis, lr = bat.listen(), bat.listen(sample_rate=16000, format="f32")  # "f32" is the default's name
    st = bat.submit_stream(None, [3, 3, 1], max_audio_length_ms=80 * 7, voice_match=False, format="f32")
    plain = bat.submit(None, [3, 3, 2], max_audio_length_ms=80 * 4, voice_match=False, sample_rate=8000)
    lis.feed(_wave(1, 5 * SPF + 1)); lr.feed(_wave(2, 40))
    lis.feed(_wave(1, 2).tobytes())  # bytes are float32 samples for a listener without a format
    fa, fb = lis.end(), lr.end()
    bat.run_until_idle()
    assert fa.result(timeout=0).format == fb.result(timeout=0).format == "f32" and fa.result(timeout=0).samples == 5 * SPF + 3
    assert st.result(timeout=0).format == "f32" and plain.result(timeout=0).format == "f32" and plain.result(timeout=0).audio.dtype == torch.float32
    assert not eng.converters and bat._cvt is None
    assert all(m[2:] == (None, None) for m in _marks_of(eng, "rs_formats"))  # every set_row is the call it was
    assert all(u[1] == "torch.float32" for u in _marks_of(eng, "rs_x"))  # float32 up and down, as before
    # the resamplers today's code makes for this load: the rate listener's and the plain request's one-row object; none for the streams
    assert sorted((r.max_rows, r.max_in) for r in eng.resamplers) == [(1, 1 << 30), (2, bat.LISTEN_IN)]
    assert bat._ors is None
    bat.close()
