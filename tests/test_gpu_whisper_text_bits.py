"""The Whisper text handle's outputs, bit for bit (csrc/kk_whisper_text.hip over csrc/kk_whisper_text_kernels.hip): every array the decoder
hands back on a set of fixed scripts -- window, sampled groups, beam search, the capturing forward, row mode -- hashed and compared with
tests/golden/whisper_text_bits.json.  The other Whisper tests hold the decoder to float64 and transformers references within tolerances; a host-side slip
that stays inside them (a slice offset of the shared cross projection, a table handed to the wrong launcher) shows here as a changed hash.  The kernels
are deterministic (fixed reduction orders, no floating-point atomics), so the hashes are a property of the code and the MI355X, not of a run.

The golden file is RECORDED, never derived from the code under test: `python tests/test_gpu_whisper_text_bits.py --record COMMIT [--out FILE]` in a
checkout of the commit the file names, through the Python surface only (whisper.Model, TextRuntime, RowRuntime), so the same file runs there."""
import hashlib
import json
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "whisper_text_bits.json")
KINDS = {"float": None, "q4g64": (64, 4), "q8g32": (32, 8)}  # the float checkpoint; 4-bit packed in groups of 64; 8-bit packed in groups of 32
CASES = ("window", "groups", "beam", "qk", "rows")
_models = {}


def _model(kind):
    """SHAPE_A from fixed seeds, as a float checkpoint or quantised and kept packed"""
    if kind not in _models:
        from mlx_audio_amd import quant, whisper

        d = T.dims(**T.SHAPE_A)
        w = {**R.encoder_weights(d, 5), **T.decoder_weights(d, 21)}
        if KINDS[kind] is None:
            m = whisper.Model(d).load_weights(w)
        else:
            group, bits = KINDS[kind]
            q = quant.quantize_checkpoint(w, group, bits, names=quant.whisper_quantised_layer_names(w, group))
            m = whisper.Model(d).load_weights(q, {"group_size": group, "bits": bits}, "packed")
            assert m.weight_report()["packed"] > 0
        _models[kind] = (d, m)
    return _models[kind]


def _tokens(d, shape, seed):
    return np.random.default_rng(seed).integers(0, d.n_vocab, shape).astype(np.int32)


def _states(rows):
    """pick states -> (the integer fields [n][6], the float fields [n][2])"""
    ints = np.array([[r.last, r.penultimate, r.last_timestamp, r.ended, r.count, r.reserved] for r in rows], np.int32)
    return ints, np.array([[r.sum_logprob, r.last_logprob] for r in rows], np.float32)


def _picked(out, name, toks, rows):
    """what read() returns: the states, and of every row the tokens it has sampled (the store behind them is not written)"""
    out[name + ".state_ints"], out[name + ".state_floats"] = _states(rows)
    out[name + ".tokens"] = np.concatenate([toks[b, : max(int(r.count), 0)] for b, r in enumerate(rows)] + [np.zeros(0, np.int32)])


def _rounds(rt, out, name, n):
    """n rounds of pick + step, the logits of every step"""
    for i in range(n):
        rt.pick()
        rt.step()
        out[f"{name}.step{i}"] = rt._step_logits.cpu().numpy()
    out[name + ".not_ended"] = np.array([rt.not_ended()], np.int32)
    _picked(out, name, *rt.read())


def _window(d, m, out):
    """B = 3 on a 7-token prompt with all positions: 21 flat rows, a full 16-row Linear launch and a 5-row tail; then four greedy rounds"""
    import torch

    from mlx_audio_amd import whisper_decoding as WD

    rt = m._text
    rt.set_audio(torch.from_numpy(T.features(d, 3, 8)).to(m.device))
    out["window.logits"] = rt.forward(torch.from_numpy(_tokens(d, (3, 7), 3)).to(m.device), True).cpu().numpy()
    rt.pick_setup(*WD.pick_params(d, WD.special_tokens(d), WD.DecodingOptions()))
    _rounds(rt, out, "window", 4)


def _groups(d, m, out):
    """2 windows x 3 rows on one cross K/V each, sampled at a fixed temperature, seed and stream ids (no suppress mask: the cleared one)"""
    import torch

    from mlx_audio_amd import whisper_decoding as WD

    rt = m._text
    rt.set_audio_groups(torch.from_numpy(T.features(d, 2, 9)).to(m.device), 3)
    out["groups.logits"] = rt.forward(torch.from_numpy(np.repeat(_tokens(d, (2, 4), 4), 3, axis=0)).to(m.device), False).cpu().numpy()
    params, _ = WD.pick_params(d, WD.special_tokens(d), WD.DecodingOptions(suppress_tokens=None))
    rt.pick_setup(params, None)
    rt.sample_setup(0.7, 1234, np.arange(6) + 10)
    _rounds(rt, out, "groups", 4)


def _beam(d, m, out):
    """2 windows x beam 3 for five steps: from the second on the self-attention reads its keys through the owner table"""
    import torch

    from mlx_audio_amd import whisper_decoding as WD

    rt = m._text
    rt.set_audio_groups(torch.from_numpy(T.features(d, 2, 10)).to(m.device), 3)
    rt.pick_setup(*WD.pick_params(d, WD.special_tokens(d), WD.DecodingOptions()))
    rt.beam_setup(3, 3)
    rt.forward(torch.from_numpy(np.repeat(_tokens(d, (2, 4), 5), 3, axis=0)).to(m.device), True)
    rt.pick()
    for _ in range(5):
        rt.step()
        rt.pick()
    out["beam.logits"] = rt._step_logits.cpu().numpy()
    out["beam.not_complete"] = np.array([rt.beam_not_complete()], np.int32)
    finished, live = rt.beam_read()
    for which, seqs in (("finished", finished), ("live", live)):
        flat = [s for window in seqs for s in window]
        out[f"beam.{which}.count"] = np.array([len(window) for window in seqs], np.int32)
        out[f"beam.{which}.length"] = np.array([len(t) for t, _ in flat], np.int32)
        out[f"beam.{which}.tokens"] = np.array([t for seq, _ in flat for t in seq], np.int32)
        out[f"beam.{which}.sum"] = np.array([s for _, s in flat], np.float32)


def _qk(d, m, out):
    """the capturing forward on three (layer, head) pairs over both layers"""
    import torch

    rt = m._text
    rt.set_audio(torch.from_numpy(T.features(d, 3, 11)).to(m.device))
    logits, qk = rt.forward_qk(torch.from_numpy(_tokens(d, (3, 7), 6)).to(m.device), [(0, 1), (1, 0), (1, 1)], 90)
    out["qk.logits"], out["qk.scores"] = logits.cpu().numpy(), qk.cpu().numpy()


def _rows(d, m, out):
    """row mode, max_rows 4, three admissions with prompts of 3, 4 and 5 tokens.  Round 0 prefills two rows and asks for their last positions only (the
    gather path); round 1 mixes the third row's 5-token prefill with two step rows, out_rows a reordered proper subset with a kept position; round 2
    steps all three (every row wanted: no gather)."""
    import torch

    from mlx_audio_amd import whisper_decoding as WD

    tok = WD.special_tokens(d)
    rr = WD.RowRuntime(m._text, 4)
    feats = torch.from_numpy(T.features(d, 3, 12)).to(m.device)
    with_mask = WD.pick_params(d, tok, WD.DecodingOptions())
    plain = WD.pick_params(d, tok, WD.DecodingOptions(suppress_tokens=None, without_timestamps=True))
    rr.admit(0, feats[0], _tokens(d, 3, 13), *with_mask)
    rr.admit(2, feats[1], _tokens(d, 4, 14), *plain)
    out["rows.round0"] = rr.forward([(0, 0, 3, 0, -1, 0), (2, 0, 4, 0, -1, 0)], [2, 6]).cpu().numpy()
    rr.pick([0, 2])
    rr.admit(3, feats[2], _tokens(d, 5, 15), *with_mask)
    out["rows.round1"] = rr.forward([(0, 3, 1, -1, -1, 0), (3, 0, 5, 0, 1, 1), (2, 4, 1, -1, -1, 0)], [6, 5, 2, 0]).cpu().numpy()
    rr.pick([0, 3, 2])
    out["rows.round2"] = rr.forward([(0, 4, 1, -1, -1, 0), (2, 5, 1, -1, -1, 0), (3, 5, 1, -1, -1, 0)], [0, 1, 2]).cpu().numpy()
    rr.pick([3, 0, 2])
    out["rows.flags"] = np.array(rr.flags(), np.int32)
    for row in (0, 2, 3):
        toks, st, kept = rr.read(row, kept=True)
        _picked(out, f"rows.row{row}", toks[None], [st])
        if row == 3:
            out["rows.row3.kept"] = kept[1].cpu().numpy()  # slot 1, the only one a round wrote


SCRIPTS = dict(window=_window, groups=_groups, beam=_beam, qk=_qk, rows=_rows)


def run(kind, case):
    """-> {array name: (sha256 of its bytes, dtype, shape)} of one script on one model"""
    import torch

    d, m = _model(kind)
    out = {}
    with torch.cuda.device(m.device):
        SCRIPTS[case](d, m, out)
    return {f"{kind}/{k}": [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), str(a.dtype), list(a.shape)] for k, a in out.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        g = json.load(f)
    assert len(g["commit"]) == 40 and set(g["commit"]) <= set("0123456789abcdef")
    return g["arrays"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_bits(golden, kind, case):
    got = run(kind, case)
    want = {k: v for k, v in golden.items() if k.startswith(f"{kind}/{case}.")}
    assert sorted(got) == sorted(want)
    assert all(np.prod(v[2]) > 0 for k, v in got.items() if not k.endswith((".tokens", ".sum", ".length"))), "an output came back empty"
    changed = [k for k in sorted(got) if got[k] != want[k]]
    assert not changed, f"bits differ from the recorded ones: {changed}"


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_whisper_text_bits.py --record COMMIT [--out FILE]   (in a checkout of COMMIT)")
    arrays = {}
    for kind_ in KINDS:
        for case_ in CASES:
            arrays.update(run(kind_, case_))
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"commit": sys.argv[2], "arrays": arrays}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(arrays)} arrays to {path}")
