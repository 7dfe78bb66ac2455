"""CPU references of Whisper's token timestamps (mlx-audio_amd/whisper_timing.py, csrc/kk_whisper_align.hip): numpy restatements of
mlx_audio/stt/models/whisper/timing.py in this repository's own words -- `dtw_cpu` + `backtrace` with fp32 costs (:47-95), the reflect-padded median
filter on scipy.signal.medfilt as the reference has it (:19-44), and the alignment matrix of :147-155 in float64.  tests/test_whisper_align_cpu.py pins
the first two against transformers' `_dynamic_time_warping` and `_median_filter` (independent implementations of OpenAI's original); the GPU tests
compare the kernels against them."""
import numpy as np


def dtw(x):
    """x (N, M) -> (text_indices, time_indices), int64 arrays in forward order.  fp32 costs, cost[i][j] = x[i-1][j-1] + min3; the diagonal wins if it is
    strictly below both others, else "up" if it is strictly below both, else "left" (with NaN every comparison is false: "left")."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    inf = np.float32(np.inf)
    cost = np.full((N + 1, M + 1), inf, np.float32)
    trace = np.full((N + 1, M + 1), -1, np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, N + 1):
            prev, row, tr, xi = cost[i - 1], cost[i], trace[i], x[i - 1]
            left = inf  # cost[i][0]
            for j in range(1, M + 1):
                c0, c1, c2 = prev[j - 1], prev[j], left
                if c0 < c1 and c0 < c2:
                    c, t = c0, 0
                elif c1 < c0 and c1 < c2:
                    c, t = c1, 1
                else:
                    c, t = c2, 2
                left = xi[j - 1] + c  # float32 + float32
                row[j] = left
                tr[j] = t
    return backtrace(trace)


def backtrace(trace):
    trace = trace.copy()
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    trace[0, :] = 2
    trace[:, 0] = 1
    ti, tj = [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        tj.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        elif t == 2:
            j -= 1
        else:
            raise ValueError("Unexpected trace[i, j]")
    return np.asarray(ti[::-1], np.int64), np.asarray(tj[::-1], np.int64)


def first_cols(text_indices, time_indices, n_rows):
    """per row the column of the path's first entry there; equals time_indices[jumps] of timing.py:169-170 (the path enters every row once, in order)"""
    out = np.full(n_rows, -2, np.int64)
    for k in range(len(text_indices) - 1, -1, -1):
        if text_indices[k] >= 0:
            out[text_indices[k]] = time_indices[k]
    return out


def jumps(text_indices, time_indices):
    """timing.py:169-170 word for word"""
    j = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    return np.asarray(time_indices)[j]


def median_filter(x, filter_width):
    """timing.py:19-44 along the last dimension of a 2-D or 3-D array, in the array's own precision"""
    from scipy import signal

    x = np.asarray(x)
    pad = filter_width // 2
    if x.shape[-1] <= pad:
        return x
    assert filter_width > 0 and filter_width % 2 == 1
    lead = x.shape[:-1]
    y = np.pad(x.reshape(-1, x.shape[-1]), ((0, 0), (pad, pad)), mode="reflect")
    y = signal.medfilt(y, kernel_size=(1, filter_width))
    if pad:
        y = y[:, pad:-pad]
    return y.reshape(*lead, -1)


def align_matrix(qk, qk_scale=1.0, medfilt_width=7):
    """timing.py:147-155 in float64: qk (heads, rows, frames), already cropped -> (rows, frames)"""
    w = np.asarray(qk, np.float64) * np.float64(np.float32(qk_scale))
    w = np.exp(w - w.max(axis=-1, keepdims=True))
    w = w / w.sum(axis=-1, keepdims=True)
    return standardise_filter_mean(w, medfilt_width)


def standardise_filter_mean(w, medfilt_width=7):
    """the part behind the softmax: w (heads, rows, frames) attention weights, float64"""
    w = np.asarray(w, np.float64)
    mean = w.mean(axis=-2, keepdims=True)
    std = np.sqrt(w.var(axis=-2, keepdims=True, ddof=0))
    w = (w - mean) / std
    return median_filter(w, medfilt_width).mean(axis=0)


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a)))
