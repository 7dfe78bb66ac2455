"""Restatements of Parakeet's text side (mlx_audio/stt/models/parakeet/rnnt.py, parakeet.py:307-599) in numpy on the bf16-rounded operands the device
uses: weights rounded once, every Linear's input rounded as it is read, everything else in the dtype asked for (float64 unless a test wants float32)."""
import numpy as np
import torch

ACTS = {"relu": lambda v: np.maximum(v, 0), "sigmoid": lambda v: 1 / (1 + np.exp(-v)), "tanh": np.tanh}


def bf16(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).bfloat16().double().numpy()


def sigmoid(v):
    return 1 / (1 + np.exp(-v))


def lstm_cell(x, h, c, wx, wh, b, dtype=np.float64):
    """MLX's LSTM step, gates i, f, g, o: x [M][in], h, c [M][H] -> (h', c')"""
    z = (bf16(x).astype(dtype) @ bf16(wx).astype(dtype).T + bf16(h).astype(dtype) @ bf16(wh).astype(dtype).T + np.asarray(b, dtype)).astype(dtype)
    i, f, g, o = np.split(z, 4, axis=-1)
    cn = sigmoid(f) * np.asarray(c, dtype) + sigmoid(i) * np.tanh(g)
    return (sigmoid(o) * np.tanh(cn)).astype(dtype), cn.astype(dtype)


def interleave_rows(H):
    """row p of the packed LSTM matrix holds original row perm[p]: tile of 16 = 4 hidden units x their 4 gates"""
    return np.array([(p % 4) * H + 4 * (p // 16) + (p % 16) // 4 for p in range(4 * H)])


def joint_logits(encp_rows, predp, w, b, act):
    """encp_rows, predp [M][Hj] -> [M][C]; the add in float32, as on the device"""
    a = ACTS[act]((np.asarray(encp_rows, np.float32) + np.asarray(predp, np.float32)).astype(np.float64))
    return bf16(a) @ bf16(w).T + np.asarray(b, np.float64)


def linear(x, w, b):
    return bf16(x) @ bf16(w).T + np.asarray(b, np.float64)


def greedy(P, feat, length, kind, max_symbols, cap=None, step_cap=None):
    """The reference loop for one row.  P: embed, lstm [(wx, wh, b)], pred (w, b), enc (w, b), out (w, b), act, V, durations.
    -> (triples (token, frame, duration index), margins [both arg-maxima of every step], events)"""
    V, L = P["V"], len(P["lstm"])
    H = P["lstm"][0][1].shape[1]
    encp = linear(feat, *P["enc"])
    hid, last, t, ns, out, margins, ev = None, V, 0, 0, [], [], set()

    def margin(v):
        s = np.sort(v)
        return s[-1] - s[-2] if len(s) > 1 else np.inf

    steps = 0
    while t < length:
        if cap is not None and (len(out) >= cap or steps >= step_cap):
            ev.add("truncated")
            break
        steps += 1
        x = np.zeros((1, H)) if last == V else bf16(P["embed"])[last][None]
        prop = []
        for l in range(L):
            h0, c0 = (np.zeros((1, H)), np.zeros((1, H))) if hid is None else hid[l]
            hn, cn = lstm_cell(x, h0, c0, *P["lstm"][l])
            prop.append((hn, cn))
            x = hn
        z = joint_logits(encp[t][None], linear(x, *P["pred"]), *P["out"], P["act"])[0]
        tok = int(np.argmax(z[:V + 1]))
        margins.append(margin(z[:V + 1]))
        di = 0
        if kind == "tdt":
            di = int(np.argmax(z[V + 1:]))
            margins.append(margin(z[V + 1:]))
        if tok != V:
            out.append((tok, t, di))
            last, hid = tok, prop
            ev.add("emission")
        else:
            ev.add("blank")
        if kind == "tdt":
            d = P["durations"][di]
            t += d
            ns += 1
            if d > 1:
                ev.add("skip")
            if d != 0:
                ns = 0
            else:
                if tok != V:
                    ev.add("duration0")
                if max_symbols is not None and max_symbols <= ns:
                    t += 1
                    ns = 0
                    ev.add("forced")
        elif tok != V:
            ns += 1
            if max_symbols is not None and max_symbols <= ns:
                t += 1
                ns = 0
                ev.add("forced")
        else:
            t += 1
            ns = 0
    return out, margins, ev


def ctc_tokens(ids, blank):
    """parakeet.py:526-594: (token, first frame, end frame) with end = the next token's first frame, or the last non-blank frame + 1"""
    out, prev, bounds = [], -1, []
    for t, k in enumerate(ids):
        k = int(k)
        if k == blank or k == prev:
            continue
        if prev != -1:
            out.append((prev, bounds[-1], t))
        bounds.append(t)
        prev = k
    if prev != -1:
        last = len(ids) - 1
        for t in range(len(ids) - 1, bounds[-1], -1):
            if int(ids[t]) != blank:
                last = t
                break
        out.append((prev, bounds[-1], last + 1))
    return out
