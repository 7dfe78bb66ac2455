"""Host logic (no GPU): the mirrors of the reference's Python surface behave like the reference's own tests expect
(mlx_audio/tts/tests/test_base.py:10-62, test_models.py:138-324) and the C-ABI library exports every declared symbol."""
import ctypes
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import mlx_audio_amd.params as P
from mlx_audio_amd import _lib
from mlx_audio_amd.base import BaseModelArgs, check_array_shape
from mlx_audio_amd.pipeline import ALIASES, LANG_CODES, KokoroPipeline, load_voice_tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "kokoro_hip.h")).read()
    declared = set(re.findall(r"\b(kk_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert lib.kk_abi_version() == 2
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in kokoro_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert set(_lib.SIGNATURES) <= declared


def test_library_reads_no_environment_switches():
    # the library is steered through its C ABI only: a switch read from the environment escapes the graph caches' keys and every test
    found = []
    for sub in ("mlx-audio_amd/csrc", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".hip", ".h", ".hpp", ".cpp", ".cc", ".c", ".inc")):
                    p = os.path.join(dirpath, f)
                    found += [f"{os.path.relpath(p, ROOT)}:{i}" for i, line in enumerate(open(p), 1) if "getenv" in line]
    assert not found, found


def test_library_has_no_compile_time_switches():
    # one shipped form per kernel: the only macros the sources test are the ABI header's guard, C++ detection and two instrumentation
    # builds (build.py --trace; tools/gridbar/gemvm_bench.hip), so no alternative form can sit uncompiled next to the product one
    allowed = {"__cplusplus", "KOKORO_HIP_H", "KK_MFMA_TRACE", "KK_TS_PER_WG"}
    tested = set()
    for sub in ("mlx-audio_amd/csrc", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".hip", ".h", ".hpp", ".cpp", ".cc", ".c", ".inc")):
                    for line in open(os.path.join(dirpath, f)):
                        m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif)\b(.*)", line)
                        if m:  # every name in the condition, defined(X) included
                            tested |= set(re.findall(r"[A-Za-z_]\w*", m.group(2).split("//")[0].split("/*")[0])) - {"defined"}
    assert tested <= allowed, sorted(tested - allowed)
    # build.py builds the product library and the --trace side build, nothing else
    src = open(os.path.join(ROOT, "mlx-audio_amd", "build.py")).read()
    assert set(re.findall(r"""["'](--[a-z][\w-]*)["']""", src)) <= {"--trace", "--force"}


def test_kk_create_rejects_bad_configs_without_a_gpu():
    from mlx_audio_amd.engine import make_kk_config

    lib = _lib.load()
    h = ctypes.c_void_p()
    cfg = P.kokoro_config(with_vocab=False)
    kc = make_kk_config(cfg)
    assert lib.kk_create(ctypes.byref(kc), ctypes.byref(h)) == 0
    # loading after create works on the host; an unknown dtype is refused with a message
    arr = np.zeros((4,), np.float32)
    shp = (ctypes.c_int64 * 1)(4)
    assert lib.kk_load_tensor(h, b"x", 99, shp, 1, arr.ctypes.data_as(ctypes.c_void_p)) != 0
    assert b"dtype" in lib.kk_last_error()
    assert lib.kk_workspace_bytes(h, 1, 10, 10) == 0  # not finalized
    lib.kk_destroy(h)
    kc.style_dim = 64
    assert lib.kk_create(ctypes.byref(kc), ctypes.byref(h)) != 0
    assert b"style_dim" in lib.kk_last_error()


def test_base_model_args_from_dict():
    class TestArgs(BaseModelArgs):
        def __init__(self, param1, param2, param3=None):
            self.param1, self.param2, self.param3 = param1, param2, param3

    a = TestArgs.from_dict({"param1": 1, "param2": "test", "param3": True, "extra": "ignored"})
    assert (a.param1, a.param2, a.param3) == (1, "test", True) and not hasattr(a, "extra")
    assert TestArgs.from_dict({"param1": 1, "param2": "t"}).param3 is None


def test_check_array_shape_truth_table():
    assert check_array_shape(np.zeros((64, 3, 3)))
    assert not check_array_shape(np.zeros((64, 3, 4)))
    assert not check_array_shape(np.zeros((2, 3, 3)))
    assert not check_array_shape(np.zeros((64, 3)))
    assert not check_array_shape(np.zeros((64, 3, 3, 3)))


def test_model_config_from_reference_hyperparameters():
    from mlx_audio_amd.kokoro import Model, ModelConfig

    cfg = P.kokoro_config()
    cfg["vocab"] = {"a": 1, "b": 2}
    mc = ModelConfig.from_dict(cfg)  # extra keys (model_type) are dropped
    m = Model(mc)
    assert m.vocab == {"a": 1, "b": 2} and m.sample_rate == 24000 and m.context_length == 512
    out = Model.Output(audio="A", pred_dur="D")
    assert out.audio == "A" and out.pred_dur == "D"
    with pytest.raises(_lib.KokoroHipError):
        m.engine  # no weights -> loud failure, never a fallback


def test_aliases_and_quiet_pipeline():
    for v in ALIASES.values():
        assert v in LANG_CODES
    assert ALIASES["en-us"] == "a" and LANG_CODES["j"] == "Japanese"
    p = KokoroPipeline(lang_code="en-us", model=False, repo_id="mock")
    assert p.lang_code == "a" and p.model is False
    with pytest.raises(ValueError):
        KokoroPipeline(lang_code="a", model=False, repo_id=None)
    r = list(p.generate_from_tokens("hɛlˈoʊ", voice=None))
    assert r[0].phonemes == "hɛlˈoʊ" and r[0].audio is None and len(r[0]) == 3 and list(r[0])[1] == "hɛlˈoʊ"
    with pytest.raises(ValueError):
        list(p.generate_from_tokens("a" * 511, voice=None))
    with pytest.raises(ValueError):
        list(KokoroPipeline(lang_code="a", model=object(), repo_id="m")("text", voice=None))


def _tok(text, ph, ws=" "):
    return SimpleNamespace(text=text, phonemes=ph, whitespace=ws, start_ts=None, end_ts=None)


def test_chunker_and_timestamps():
    toks = [_tok("Hello", "həlˈoʊ"), _tok(",", ",", " "), _tok("world", "wˈɜɹld", ""), _tok(".", ".", "")]
    assert KokoroPipeline.tokens_to_ps(toks) == "həlˈoʊ , wˈɜɹld."
    assert KokoroPipeline.tokens_to_text(toks) == "Hello , world."
    p = KokoroPipeline(lang_code="a", model=False, repo_id="m")
    # > 510 phonemes: split at the last sentence end (waterfall, pipeline.py:170-226)
    long = []
    for i in range(60):
        long += [_tok("word", "wˈɜɹdwˈɜɹd"), _tok(".", ".", " ")]
    chunks = list(p.en_tokenize(long))
    assert len(chunks) >= 2 and all(len(ps) <= 510 for _, ps, _ in chunks)
    assert "".join(ps.replace(" ", "") for _, ps, _ in chunks) == KokoroPipeline.tokens_to_ps(long).replace(" ", "")
    assert chunks[0][1].endswith(".")
    # timestamps: <bos>=5 frames, then tokens
    toks = [_tok("hi", "hˈaɪ"), _tok("you", "jˈu", "")]
    pred = np.array([5, 3, 3, 3, 2, 4, 4, 4, 6, 7], np.int32)  # bos | h ˈ a ɪ | space | j ˈ u | eos
    KokoroPipeline.join_timestamps(toks, pred)
    assert toks[0].start_ts == pytest.approx(2 * (5 - 3) / 80) and toks[0].end_ts > toks[0].start_ts
    assert toks[1].start_ts >= toks[0].end_ts


def test_voice_pack_formats(tmp_path):
    rows = np.load(os.path.join(ROOT, "tests", "golden", "af_heart_rows.npz"))["rows"]
    pack = np.repeat(rows[:1][None], 510, axis=0).reshape(510, 1, 256)
    np.save(tmp_path / "v.npy", pack)
    json.dump(pack[:4].tolist(), open(tmp_path / "v.json", "w"))
    import torch

    torch.save(torch.tensor(pack), tmp_path / "v.pt")
    assert load_voice_tensor(str(tmp_path / "v.npy")).shape == (510, 1, 256)
    assert load_voice_tensor(str(tmp_path / "v.json")).shape == (4, 1, 256)
    np.testing.assert_array_equal(load_voice_tensor(str(tmp_path / "v.pt")), pack)
    p = KokoroPipeline(lang_code="a", model=False, repo_id="m")
    a = p.load_voice(str(tmp_path / "v.npy"))
    both = p.load_voice(f"{tmp_path / 'v.npy'},{tmp_path / 'v.pt'}")
    np.testing.assert_allclose(both, a)


def test_load_model_error_behaviour(tmp_path):
    from mlx_audio_amd.utils import load_model

    d = tmp_path / "kokoro-82m"
    d.mkdir()
    with pytest.raises(FileNotFoundError):
        load_model(str(d))  # no config.json
    json.dump(dict(P.kokoro_config(), model_type="kokoro"), open(d / "config.json", "w"))
    with pytest.raises(FileNotFoundError):
        load_model(str(d))  # no safetensors (utils.py:195-215)
    d2 = tmp_path / "bark-small"
    d2.mkdir()
    json.dump({"model_type": "bark"}, open(d2 / "config.json", "w"))
    open(d2 / "x.safetensors", "wb").write(b"")
    with pytest.raises(ValueError):
        load_model(str(d2))  # unsupported model type (utils.py:116-119)
    with pytest.raises(ValueError):
        load_model(123)


def test_mlx_affine_quantisation_round_trip():
    """quant.py (row Q1, loader level): pack / unpack are inverse, the dequantised matrix is within half a step of the original,
    and dequantize_checkpoint applies the reference's predicate ({p}.scales present, utils.py:243-252)."""
    from mlx_audio_amd.quant import dequantize_affine, dequantize_checkpoint, quantize_affine

    rng = np.random.default_rng(0)
    for bits in (8, 4):
        w = rng.standard_normal((24, 256)).astype(np.float32)
        words, scales, biases = quantize_affine(w, 64, bits)
        assert words.dtype == np.uint32 and words.shape == (24, 256 * bits // 32) and scales.shape == biases.shape == (24, 4)
        back = dequantize_affine(words, scales, biases, 64, bits)
        assert np.all(np.abs(back - w) <= 0.5 * np.repeat(scales, 64, axis=1) + 1e-6)
        w2, s2, b2 = quantize_affine(back, 64, bits)  # a dequantised matrix is a fixed point of the quantiser's grid
        np.testing.assert_allclose(dequantize_affine(w2, s2, b2, 64, bits), back, atol=2e-6)
    # first element of a word sits in the least significant bits
    words, scales, biases = quantize_affine(np.tile(np.arange(64, dtype=np.float32), (1, 1)), 64, 8)
    assert int(words[0, 0] & 0xFF) == 0 and int((words[0, 0] >> 8) & 0xFF) == round(1 / scales[0, 0])
    ck = {"a.weight": words, "a.scales": scales, "a.biases": biases, "b.weight": np.ones((2, 2), np.float32), "c.bias": np.zeros(3, np.float32)}
    out = dequantize_checkpoint(ck, 64, 8)
    assert set(out) == {"a.weight", "b.weight", "c.bias"} and out["a.weight"].shape == (1, 64) and out["a.weight"].dtype == np.float32
    np.testing.assert_allclose(out["a.weight"][0], np.arange(64), atol=0.5 * float(scales[0, 0]) + 1e-5)


def test_batch_scheduler_plans_and_keeps_text_order():
    """plan_batches: every chunk once, batches bounded in size and in padding waste, longest first; the batched __call__ yields the
    chunks in text order with the outputs of the batch they ran in (fake model: no GPU)."""
    rng = np.random.default_rng(0)
    lens = rng.integers(5, 500, 57).tolist()
    plan = KokoroPipeline.plan_batches(lens, 8, 0.25)
    assert sorted(i for b in plan for i in b) == list(range(57))
    assert all(1 <= len(b) <= 8 for b in plan)
    assert all(min(lens[i] for i in b) >= 0.75 * max(lens[i] for i in b) for b in plan)
    assert [max(lens[i] for i in b) for b in plan] == sorted((max(lens[i] for i in b) for b in plan), reverse=True)
    assert KokoroPipeline.plan_batches([], 8) == [] and KokoroPipeline.plan_batches([3], 8) == [[0]]

    calls = []

    class FakeModel:
        def batch_call(self, phonemes, ref_s, speed=1, seed=None):
            calls.append(list(phonemes))
            assert ref_s.shape == (len(phonemes), 256)
            # the style row of a chunk is pack[len(ps) - 1] (pipeline.py:236): the fake pack stores its own row index
            assert [int(r[0]) for r in ref_s] == [len(p) - 1 for p in phonemes]
            return [SimpleNamespace(audio=np.full((1, 600 * len(p)), float(len(p)), np.float32), pred_dur=None) for p in phonemes]

        def __call__(self, ps, ref_s, speed=1, return_output=False):
            return self.batch_call([ps], np.asarray(ref_s).reshape(1, 256), speed)[0]

    words = ["a" * n for n in (30, 7, 31, 8, 29, 300)]
    p = KokoroPipeline(lang_code="e", model=FakeModel(), repo_id="m", g2p=lambda t: (t, None))  # identity G2P, non-English branch
    p.voices["v"] = np.repeat(np.arange(510, dtype=np.float32)[:, None, None], 256, axis=2)
    res = list(p("\n".join(words), voice="v", batch_size=4))
    assert [r.phonemes for r in res] == words and [r.text_index for r in res] == list(range(6))
    assert [float(r.audio[0, 0]) for r in res] == [float(len(w)) for w in words]
    assert sorted(map(sorted, calls)) == sorted(map(sorted, [["a" * 300], ["a" * 31, "a" * 30, "a" * 29], ["a" * 8, "a" * 7]]))
    calls.clear()
    assert [r.phonemes for r in p("\n".join(words), voice="v")] == words and all(len(c) == 1 for c in calls)  # default: chunk by chunk


def test_chunk_planner_and_timestamps_against_reference_generated_vectors():
    """tests/golden/reference_chunker_cases.json was produced by the REFERENCE'S OWN en_tokenize / waterfall_last / tokens_to_ps /
    tokens_to_text (pipeline.py:163-226) and join_timestamps (:292-328), compiled from the reference's source in the build container by
    tests/golden/make_golden_reference_host.py: 36 random token streams -> chunks, 42 (tokens, pred_dur) pairs -> start / end times, incl.
    too-short duration vectors.  (Round 2's self-generated file was byte-for-byte what the reference produces; it is gone.)"""
    from types import SimpleNamespace

    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_chunker_cases.json")))
    assert "compiled from /root/reference" in cases["source"] and len(cases["chunk_cases"]) == 36 and len(cases["timestamp_cases"]) == 42
    p = KokoroPipeline(lang_code="a", model=False, repo_id="m")
    for c in cases["chunk_cases"]:
        objs = [SimpleNamespace(text=t, phonemes=ph, whitespace=ws) for t, ph, ws in c["tokens"]]
        got = [[gs, ps, len(tk)] for gs, ps, tk in p.en_tokenize(objs)]
        assert got == c["chunks"]  # (the reference's planner can overshoot 510 when the blanks it did not count add up; its callers truncate)
    for c in cases["timestamp_cases"]:
        objs = [SimpleNamespace(text=t, phonemes=ph, whitespace=ws, start_ts=None, end_ts=None) for t, ph, ws in c["tokens"]]
        KokoroPipeline.join_timestamps(objs, np.asarray(c["pred_dur"], np.int32))
        assert [[o.start_ts, o.end_ts] for o in objs] == c["ts"]


def test_host_functions_against_reference_generated_vectors(tmp_path):
    """tests/golden/reference_host_cases.json (same script): the reference's check_array_shape (base.py:21-34) on every 3-D shape of the
    Kokoro checkpoint, sanitize_lstm_weights (kokoro.py:24-44), Model.sanitize + Decoder.sanitize (kokoro.py:172-252, istftnet.py:965-979) run on
    the PyTorch-layout checkpoints `params.to_torch_layout` makes, and load_voice_tensor (voice.py:9-81) on a torch.save'd pack."""
    import hashlib

    import torch

    import mlx_audio_amd.params as P
    from mlx_audio_amd.pipeline import load_voice_tensor

    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_host_cases.json")))
    for shape, want in g["check_array_shape"]:
        assert check_array_shape(np.zeros(shape, np.int8)) is want, shape
    # LSTM renames: params.to_torch_layout is the inverse table (the forward table lives in kk_load_tensor, exercised on the GPU by
    # test_python_surface_load_model_pipeline_both_layouts)
    for key, new in g["sanitize_lstm_weights"]:
        if new != key:
            assert list(P.to_torch_layout({new: np.zeros(1)})) == [key]
    # reference.sanitize(to_torch_layout(w)) == w, names, shapes and values, on the tiny and the full Kokoro-82M checkpoint
    for name, cfg in (("tiny", P.tiny_config()), ("full", P.kokoro_config(False))):
        rec = g[f"sanitize_{name}"]
        assert rec["equals_mlx_layout_checkpoint"] is True and rec["differing"] == []
        inv = {n: list(s) for n, s, _ in P.param_inventory(cfg)}
        assert rec["table"] == {k: inv[k] for k in sorted(inv)}
    w = P.synth_checkpoint(P.tiny_config(), g["sanitize_tiny"]["seed"])  # the checkpoint the fixture was made from is today's
    assert {k: sha(np.asarray(v, np.float32)) for k, v in sorted(w.items())} == g["sanitize_tiny"]["sha"]
    # voice pack reader
    vp = g["voice_pack"]
    pack = torch.randn(510, 1, 256, generator=torch.Generator().manual_seed(vp["seed"]))
    torch.save(pack, tmp_path / "v.pt")
    arr = load_voice_tensor(str(tmp_path / "v.pt"))
    assert list(arr.shape) == vp["shape"] and vp["equals_torch_tensor"] and sha(np.asarray(arr, np.float32)) == vp["sha"]


def test_dequantize_checkpoint_honours_per_layer_group_size_and_bits():
    """config["quantization"][p] = {"group_size", "bits"} (tts/utils.py:244-246): that layer's triplet is unpacked with ITS parameters, the
    rest with the global ones; a layer mapped to False passes through untouched."""
    from mlx_audio_amd.quant import dequantize_affine, dequantize_checkpoint, quantize_affine

    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(s).astype(np.float32) for s in ((8, 128), (16, 64), (4, 64)))
    ck = {}
    ck["x.weight"], ck["x.scales"], ck["x.biases"] = quantize_affine(a, 64, 8)
    ck["y.weight"], ck["y.scales"], ck["y.biases"] = quantize_affine(b, 32, 4)
    ck["z.weight"] = c
    ck["norm.weight"] = np.ones(7, np.float32)
    out = dequantize_checkpoint(ck, 64, 8, {"y": {"group_size": 32, "bits": 4}, "z": False})
    assert sorted(out) == ["norm.weight", "x.weight", "y.weight", "z.weight"]
    np.testing.assert_array_equal(out["x.weight"], dequantize_affine(ck["x.weight"], ck["x.scales"], ck["x.biases"], 64, 8))
    np.testing.assert_array_equal(out["y.weight"], dequantize_affine(ck["y.weight"], ck["y.scales"], ck["y.biases"], 32, 4))
    assert out["y.weight"].shape == (16, 64) and np.abs(out["y.weight"] - b).max() < (b.max() - b.min()) / 15
    assert np.abs(out["x.weight"] - a).max() < (a.max() - a.min()) / 255
    assert out["z.weight"] is c


def test_tts_service_request_semantics_and_pool_planner():
    """The `/tts` handler's parameter rules (server.py:126-163, 193-220) and the cross-request batch planner, no GPU."""
    from mlx_audio_amd.service import TTSError, TTSService, parse_request, plan_pool

    assert parse_request("hi", None, "1.0", "a") == ("hi", "af_heart", 1.0, "a")
    assert parse_request("hi", "bf_emma", "0.5", "british_english")[2:] == (0.5, "b")
    assert parse_request("hi", "em_alex", "2", "klingon")[3] == "e"     # unknown language: first letter of the voice
    assert parse_request("hi", "  ", "1", "klingon")[1:] == ("af_heart", 1.0, "a")  # blank voice = no voice
    for bad, status, msg in ((("", None, "1.0", "a"), 400, "Text is empty"), (("   ", None, "1.0", "a"), 400, "Text is empty"),
                             (("x", None, "fast", "a"), 400, "Invalid speed value"), (("x", None, "0.49", "a"), 400, "Speed must be between 0.5 and 2.0"),
                             (("x", None, "2.5", "a"), 400, "Speed must be between 0.5 and 2.0")):
        with pytest.raises(TTSError) as ei:
            parse_request(*bad)
        assert ei.value.status == status and ei.value.message == msg
    # pooled planner: every chunk exactly once, batches bounded, padding waste bounded
    rng = np.random.default_rng(0)
    lengths = rng.integers(3, 510, 200).tolist()
    batches = plan_pool(lengths, 32)
    assert sorted(i for b in batches for i in b) == list(range(200))
    for b in batches:
        assert 1 <= len(b) <= 32 and min(lengths[i] for i in b) >= 0.75 * max(lengths[i] for i in b)
    # a request that fails validation never reaches the queue: its future already holds the error
    svc = TTSService(model=None, start=False)
    f = svc.submit("", speed="1.0")
    assert f.done() and isinstance(f.exception(), TTSError) and f.exception().status == 400
    assert svc._q.empty()


def test_csm_generate_batch_tracks_every_streams_own_eos():
    """sesame.Model.generate_batch on a scripted frame generator (no GPU): an all-zero frame ends a stream (sesame.py:765-766); streams that
    end early are trimmed to their own frames, the loop runs until the LAST stream has ended (checked every `eos_check_interval` frames),
    ragged prompts are left-padded and announced to the model, and sampling draws fresh uniforms when seed is None."""
    import torch

    from mlx_audio_amd.sesame import Model

    class FakeCsm:
        cfg = dict(audio_num_codebooks=2, max_seq_len=64)
        device = torch.device("cpu")
        max_batch = 0

        def __init__(self):
            self.calls, self.pads, self.uniforms = [], None, []
            self.script = {0: 5, 1: 2, 2: 9}  # stream b emits its all-zero frame at frame index script[b]

        def caches_are_enabled(self):
            return self.max_batch > 0

        def setup_caches(self, B):
            self.max_batch = B

        def reset_caches(self):
            self.frame = 0

        def set_padding(self, pads):
            self.pads = list(pads)

        def set_graph_mode(self, on):
            pass

        def generate_frame(self, tok, msk, temperature=0.0, top_k=50, uniforms=None):
            self.calls.append(tuple(tok.shape))
            self.uniforms.append(None if uniforms is None else uniforms.clone())
            out = torch.full((tok.shape[0], 2), 7, dtype=torch.int32)
            for b, at in self.script.items():
                if self.frame == at:
                    out[b] = 0
            self.frame += 1
            return out

    class FakeMimi:
        def decode(self, codes):
            return torch.arange(codes.shape[0] * codes.shape[2] * 1920, dtype=torch.float32).reshape(codes.shape[0], 1, -1)

    real_sync = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: None
    try:
        csm = FakeCsm()
        m = Model(dict(csm.cfg, backbone={}, decoder={}, text_vocab_size=10, audio_vocab_size=10), mimi=FakeMimi(), csm=csm)
        prompts = [(np.ones((L, 3), np.int32), np.ones((L, 3), np.float32)) for L in (4, 6, 5)]
        res = m.generate_batch(prompts, max_audio_length_ms=80 * 40, temperature=0.9, seed=None, eos_check_interval=4)
    finally:
        torch.cuda.synchronize = real_sync
    assert csm.pads == [2, 0, 1] and csm.calls[0] == (3, 6, 3) and set(csm.calls[1:]) == {(3, 1, 3)}
    assert res.frames == [5, 2, 9] and [a.shape[0] for a in res.audio] == [5 * 1920, 2 * 1920, 9 * 1920]
    assert len(csm.calls) == 12  # the last EOS is frame 9; the host looks every 4 frames: 12 frames were generated, 3 dropped
    assert res.codes.shape == (3, 2, 9)
    u = [x for x in csm.uniforms if x is not None]
    assert len(u) == 12 and not torch.equal(u[0], u[1])  # seed=None still SAMPLES (fresh entropy), it does not fall back to argmax


def test_tts_service_close_fails_queued_requests_and_later_submits():
    """close() used to drop the requests queued behind the stop marker (their callers blocked forever in Future.result()) and
    submit() kept enqueueing afterwards.  Both now fail with 503 at once.  No GPU: the service never starts a worker here."""
    from mlx_audio_amd.service import TTSError, TTSService

    svc = TTSService(model=object(), start=False)
    queued = [svc.submit("hello there", "af_heart", "1.0", "a") for _ in range(3)]
    assert not any(f.done() for f in queued)
    svc.close()
    for f in queued:
        with pytest.raises(TTSError) as ei:
            f.result(timeout=1)
        assert ei.value.status == 503
    late = svc.submit("too late", "af_heart", "1.0", "a")
    with pytest.raises(TTSError) as ei:
        late.result(timeout=1)
    assert ei.value.status == 503 and ei.value.message == "service closed"
    bad = TTSService(model=object(), start=False).submit("", None, "1.0", "a")  # validation errors still come first on an open service
    with pytest.raises(TTSError) as ei:
        bad.result(timeout=1)
    assert ei.value.status == 400
