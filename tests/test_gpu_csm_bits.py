"""The CSM generator handle's outputs, bit for bit (csrc/kk_csm.hip over csrc/kk_csm_kernels.hip and csrc/kk_csm_sample.hip): every array
the generator hands back on a set of fixed scripts -- classic frames, the device RNG, the per-row sampler table, the serving path (admit, park, shift,
prefixes), a transfer between two generators, quantised checkpoints -- hashed and compared with tests/golden/csm_bits.json.  The other CSM tests hold
the generator to oracles and to itself; a host-side slip that stays inside them (a copy launch handed the wrong pitch, an admission run with the other
entry's workspace plan or position) shows here as a changed hash.  The kernels are deterministic (fixed reduction orders, no floating-point atomics), so
the hashes are a property of the code and the MI355X, not of a run.

The golden file is RECORDED, never derived from the code under test: `python tests/test_gpu_csm_bits.py --record COMMIT [--out FILE]` in a checkout
of the commit the file names, through the Python surface only (csm.SesameModel), so the same file runs there."""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "csm_bits.json")
KINDS = {"float32": None, "bfloat16": None, "q8g32": (32, 8), "q4g64": (64, 4)}
# (a) classic, (b) device RNG, (c) table mode, (d) serving path, (e) transfer on both float formats; (f) = the classic script on the packed checkpoints
CASES = [(k, c) for k in ("float32", "bfloat16") for c in ("classic", "device_rng", "table", "serving", "transfer")] + [("q8g32", "classic"), ("q4g64", "classic")]
NCB, V, TV = 4, 67, 300
_models = {}


def _model(kind):
    """the tiny generator (max_seq_len 64) from a fixed seed: fp32 weights, their bf16 rounding in bf16 weight mode, or quantised and kept packed"""
    if kind not in _models:
        import torch

        import mlx_audio_amd.params as P
        from mlx_audio_amd import quant
        from mlx_audio_amd.csm import SesameModel

        cfg = P.csm_tiny_config()
        assert cfg["max_seq_len"] <= 64 and cfg["audio_num_codebooks"] == NCB and cfg["audio_vocab_size"] == V and cfg["text_vocab_size"] == TV
        w = P.csm_synth_checkpoint(cfg, 3)
        if KINDS[kind] is not None:
            group, bits = KINDS[kind]
            qw = quant.quantize_checkpoint(w, group, bits, names=quant.csm_quantised_layer_names(w, group))
            m = SesameModel(cfg, weights=qw, quantization={"group_size": group, "bits": bits})
            assert m.weight_format == f"q{bits}" and m.weight_fallback is None
        elif kind == "bfloat16":
            w = {k: torch.tensor(np.asarray(v, np.float32)).to(torch.bfloat16).float().numpy() for k, v in w.items()}
            m = SesameModel(cfg, weights=w, weight_dtype="bfloat16")
        else:
            m = SesameModel(cfg, weights=w)
        _models[kind] = m
    return _models[kind]


def _prompt(rng, S, pad=0):
    """S prompt frames [S][n_cb + 1] (text frames, then audio frames), the first `pad` of them padding (zero mask)"""
    tok, mask = np.zeros((S, NCB + 1), np.int32), np.zeros((S, NCB + 1), np.float32)
    n_text = (S - pad + 1) // 2
    for s in range(pad, S):
        if s < pad + n_text:
            tok[s, NCB], mask[s, NCB] = rng.integers(0, TV), 1.0
        else:
            tok[s, :NCB], mask[s, :NCB] = rng.integers(0, V, NCB), 1.0
    return tok, mask


def _next(codes, live):
    """the single-token frame that feeds every live row its last codes; a parked row gets a zero frame"""
    B = len(live)
    tok, mask = np.zeros((B, 1, NCB + 1), np.int32), np.zeros((B, 1, NCB + 1), np.float32)
    for b in range(B):
        if live[b]:
            tok[b, 0, :NCB], mask[b, 0, :NCB] = codes[b], 1.0
    return tok, mask


def _frames(m, out, name, codes, live, n, rng, first=0, **kw):
    """n single-token frames on injected uniforms (`rng` None: none, the keywords say how to draw); hashes the live rows' codes of every frame"""
    rows = [b for b in range(len(live)) if live[b]]
    for i in range(first, first + n):
        u = rng.random((len(live), NCB), dtype=np.float32) if rng is not None else None
        got = m.generate_frame(*_next(codes, live), uniforms=u, **kw).cpu().numpy()
        for b in rows:
            codes[b] = got[b]
        out[f"{name}.frame{i}"] = got[rows]
    return codes


def _classic_script(m, out, name, graph, rng_seed, draw, **kw):
    """B = 3, ragged left padding, a 9-token prompt block, 4 single-token frames; the codes of every frame and the last frame's logits"""
    rng = np.random.default_rng(rng_seed)
    pads = [0, 2, 4]
    blocks = [_prompt(rng, 9, p) for p in pads]
    m.setup_caches(3)
    m.set_graph_mode(graph)
    m.reset_caches()
    m.set_padding(pads)
    u = rng.random((3, NCB), dtype=np.float32) if draw else None
    codes = m.generate_frame(np.stack([t for t, _ in blocks]), np.stack([k for _, k in blocks]), uniforms=u, **kw).cpu().numpy()
    out[f"{name}.prompt"] = codes
    _frames(m, out, name, codes.copy(), [True] * 3, 4, rng if draw else None, **kw)
    out[f"{name}.logits"] = m.debug_logits().cpu().numpy()
    m.set_graph_mode(False)


def _both_modes(m, out, rng_seed, draw, **kw):
    """the script with graph mode off and on: the two must agree with each other as well as with the recording"""
    eager, graph = {}, {}
    _classic_script(m, eager, "eager", False, rng_seed, draw, **kw)
    _classic_script(m, graph, "graph", True, rng_seed, draw, **kw)
    for k, a in eager.items():
        assert np.array_equal(a, graph["graph" + k[len("eager"):]]), f"graph replay differs from the eager frame: {k}"
    out.update(eager)
    out.update(graph)


def _classic(m, out):
    _both_modes(m, out, 31, True, sampler=SimpleNamespace(temp=0.9, top_k=5))


def _device_rng(m, out):
    _both_modes(m, out, 32, False, sampler=SimpleNamespace(temp=0.9, top_k=0, top_p=0.8, min_p=0.05), seed=1234, stream_ids=[7, 3, 11])


def _table(m, out):
    """three rows, three samplers (one arg-max) read from the table by one replayed graph; row 0's entry changes between frames 2 and 3"""
    rng = np.random.default_rng(33)
    pads = [1, 0, 3]
    blocks = [_prompt(rng, 9, p) for p in pads]
    m.setup_caches(3)
    m.set_graph_mode(True)
    m.reset_caches()
    m.set_padding(pads)
    m.set_row_sampler(0, SimpleNamespace(temp=0.9, top_k=5))
    m.set_row_sampler(1, SimpleNamespace(temp=0.0, top_k=50))
    m.set_row_sampler(2, SimpleNamespace(temp=0.7, top_k=0, top_p=0.8))
    codes = m.generate_frame(np.stack([t for t, _ in blocks]), np.stack([k for _, k in blocks]), uniforms=rng.random((3, NCB), dtype=np.float32),
                             sampler="rows").cpu().numpy()
    out["prompt"] = codes
    codes = _frames(m, out, "frames", codes.copy(), [True] * 3, 2, rng, sampler="rows")
    m.set_row_sampler(0, SimpleNamespace(temp=1.1, top_k=0, min_p=0.02))
    _frames(m, out, "frames", codes, [True] * 3, 2, rng, first=2, sampler="rows")
    out["logits"] = m.debug_logits().cpu().numpy()
    m.set_graph_mode(False)


def _state(m):
    pad, pos = m.row_state()
    return np.array(pad + [pos], np.int32)


def _serving(m, out):
    """admit, park, a created and a captured prefix under suffixes of 1, 4 and 2 tokens (the S < 2 and S >= 2 workspace plans), shifts up and down"""
    rng = np.random.default_rng(34)
    sp = SimpleNamespace(temp=0.9, top_k=5)
    m.setup_caches(3)
    m.set_graph_mode(False)
    m.reset_caches_parked()
    m.shift(12)
    codes, live = np.zeros((3, NCB), np.int32), [False] * 3

    def admit(tag, row, S, prefix=None):
        codes[row] = m.admit(row, *_prompt(rng, S), uniforms=rng.random(NCB, dtype=np.float32), sampler=sp, prefix=prefix).cpu().numpy()
        live[row] = True
        out[tag] = codes[row].copy()

    admit("admit0", 0, 7)
    admit("admit2", 2, 9)
    _frames(m, out, "frames", codes, live, 3, rng, sampler=sp)
    m.park(0)
    live[0] = False
    created = m.make_prefix(*_prompt(rng, 5))
    admit("prefixed0", 0, 1, created)
    admit("prefixed1", 1, 4, created)
    _frames(m, out, "frames", codes, live, 2, rng, first=3, sampler=sp)
    m.shift(-2)
    out["state_shifted"] = _state(m)
    _frames(m, out, "frames", codes, live, 2, rng, first=5, sampler=sp)
    captured = m.capture_prefix(2, 6)
    m.park(2)
    live[2] = False
    admit("prefixed2", 2, 2, captured)
    _frames(m, out, "frames", codes, live, 2, rng, first=7, sampler=sp)
    out["prefix_created"], out["prefix_captured"] = created.save().cpu().numpy(), captured.save().cpu().numpy()
    out["state"] = _state(m)
    created.close()
    captured.close()


def _transfer(m, out):
    """two generators on one weight set, on two streams, caches of 2 and 3 rows (their layer pitches differ): an admission made on the first enters a
    parked row of the second, which then runs three frames"""
    import torch

    rng = np.random.default_rng(35)
    sp = SimpleNamespace(temp=0.9, top_k=5)
    src, dst = m.share(), m.share()
    s1, s2 = torch.cuda.Stream(m.device), torch.cuda.Stream(m.device)
    codes, live = np.zeros((3, NCB), np.int32), [True, False, True]
    with torch.cuda.stream(s1):
        src.setup_caches(2)
        src.reset_caches_parked()
        src.shift(8)
        moved = src.admit(1, *_prompt(rng, 6), uniforms=rng.random(NCB, dtype=np.float32), sampler=sp)
    with torch.cuda.stream(s2):
        dst.setup_caches(3)
        dst.reset_caches_parked()
        dst.shift(10)
        codes[0] = dst.admit(0, *_prompt(rng, 5), uniforms=rng.random(NCB, dtype=np.float32), sampler=sp).cpu().numpy()
        dst.admit_transfer(2, src, 1, s1)
        codes[2] = moved.cpu().numpy()
        out["admitted"] = codes[[0, 2]]
        out["state"] = _state(dst)
        _frames(dst, out, "frames", codes, live, 3, rng, sampler=sp)
        s2.synchronize()
    s1.synchronize()


SCRIPTS = dict(classic=_classic, device_rng=_device_rng, table=_table, serving=_serving, transfer=_transfer)


def run(kind, case):
    """-> {array name: (sha256 of its bytes, dtype, shape)} of one script on one model"""
    import torch

    m = _model(kind)
    out = {}
    with torch.cuda.device(m.device):
        SCRIPTS[case](m, out)
        torch.cuda.synchronize()
    return {f"{kind}/{case}.{k}": [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), str(a.dtype), list(a.shape)] for k, a in out.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        g = json.load(f)
    assert len(g["commit"]) == 40 and set(g["commit"]) <= set("0123456789abcdef")
    return g["arrays"]


@pytest.mark.parametrize("kind,case", CASES)
def test_bits(golden, kind, case):
    got = run(kind, case)
    want = {k: v for k, v in golden.items() if k.startswith(f"{kind}/{case}.")}
    assert sorted(got) == sorted(want)
    assert all(np.prod(v[2]) > 0 for v in got.values()), "an output came back empty"
    changed = [k for k in sorted(got) if got[k] != want[k]]
    assert not changed, f"bits differ from the recorded ones: {changed}"


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_csm_bits.py --record COMMIT [--out FILE]   (in a checkout of COMMIT)")
    arrays = {}
    for kind_, case_ in CASES:
        arrays.update(run(kind_, case_))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"commit": sys.argv[2], "arrays": arrays}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(arrays)} arrays to {path}")
