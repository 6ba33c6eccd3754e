"""Numpy restatement of the frame smoothing (DESIGN.md 6c "Frame smoothing"; helper module of the frame-smoothing tests; not collected).

The specification, literally, frame by frame in int64:
  quantise(x, thr)          the evidence q_t of float32 logits on the 1/64-logit grid, its sign forced to agree with the activity;
  viterbi_path(q, a, b)     forward d_t = q_t + clamp(d_t-1, -a, b) from d_-1 = 0, then backward s_L-1 = d_L-1 > 0 and, below it,
                            s_t = 1 if d_t > b, 0 if d_t <= -a, s_t+1 otherwise;
  smooth_ref(x, thr, on, off, lengths)   the (B, P, T) tensor mt_frame_smooth writes: +64 / -64 on valid frames, x elsewhere.
best_paths(q, a, b) is the brute force the scan is checked against: the maximum of sum s_t q_t - a #(0->1) - b #(1->0) over all 2^T paths.
"""
import itertools

import numpy as np

GRID, CAP = 64, 64.0                                   # evidence steps per logit; the cap of |x - logit(thr)| in logits
Y_ON, Y_OFF = np.float32(64.0), np.float32(-64.0)


def centre(thr):
    """logit(thr) as the library forms it: the float32 threshold, the logarithm in double, rounded to float32."""
    t = np.float64(np.float32(thr))
    return np.float32(np.log(t / (1.0 - t)))


def active(x, thr):
    """sigmoid(x) > thr in float32, the expression of mt_predict_threshold (a NaN is inactive).  On the device expf may differ from
    numpy's in the last bit, so the GPU tests pass the library's own activity to quantise / smooth_ref instead."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32)) > np.float32(thr)


def penalty(p):
    """A penalty in logits -> grid steps, rint(p * 64) of the float32 value."""
    return int(np.rint(np.float32(p) * np.float32(GRID)))


def quantise(x, thr, act=None):
    """float32 logits -> int64 evidence: rint(clamp(x - logit(thr), -64, 64) * 64) with fmax / fmin (a NaN ends up at the lower cap),
    then q >= 1 where the frame is active and q <= 0 where it is not.  act: the activity to use (None: active(x, thr))."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        e = np.fmin(np.fmax(x - centre(thr), np.float32(-CAP)), np.float32(CAP)) * np.float32(GRID)
    q = np.rint(e).astype(np.int64)
    act = active(x, thr) if act is None else np.asarray(act, bool)
    return np.where(act, np.maximum(q, 1), np.minimum(q, 0))


def forward_d(q, a, b):
    """d_t = V_t(on) - V_t(off) for rows q of shape (..., T): d_-1 = 0, d_t = q_t + clamp(d_t-1, -a, b)."""
    q = np.asarray(q, np.int64)
    d = np.zeros(q.shape, np.int64)
    prev = np.zeros(q.shape[:-1], np.int64)
    for t in range(q.shape[-1]):
        prev = q[..., t] + np.minimum(np.maximum(prev, -a), b)
        d[..., t] = prev
    return d


def viterbi_path(q, a, b):
    """The path of one row, a boolean array of len(q) -- or of many rows at once, q of shape (..., T): the same two loops over the
    frames, each step taken on all rows together."""
    d = forward_d(q, a, b)
    L = d.shape[-1]
    s = np.zeros(d.shape, bool)
    for t in range(L - 1, -1, -1):
        if t == L - 1:
            s[..., t] = d[..., t] > 0
        else:
            s[..., t] = np.where(d[..., t] > b, True, np.where(d[..., t] <= -a, False, s[..., t + 1]))
    return s


def score(q, s, a, b):
    """sum s_t q_t - a #(0->1) - b #(1->0), switches inside the row only; q and s of shape (..., T)."""
    q, s = np.asarray(q, np.int64), np.asarray(s, bool)
    up = (~s[..., :-1] & s[..., 1:]).sum(-1)
    down = (s[..., :-1] & ~s[..., 1:]).sum(-1)
    return (q * s).sum(-1) - a * up - b * down


def all_paths(T):
    """(2^T, T) boolean: every path of T frames."""
    return np.asarray(list(itertools.product((False, True), repeat=T)), bool).reshape(-1, T)


def best_paths(q, a, b):
    """Brute force over all 2^T paths for rows q (N, T) -> (the maximum score (N,), how many paths reach it (N,), the first of them (N, T))."""
    q = np.asarray(q, np.int64)
    S = all_paths(q.shape[-1])
    assert np.abs(q).sum(-1).max(initial=0) < 2 ** 24                        # the sums below are exact in float32, which has a fast matmul
    sc = (q.astype(np.float32) @ S.T.astype(np.float32)).astype(np.int32)
    sc -= (a * (~S[:, :-1] & S[:, 1:]).sum(-1) + b * (S[:, :-1] & ~S[:, 1:]).sum(-1)).astype(np.int32)[None, :]
    best = sc.max(-1)
    return best, (sc == best[:, None]).sum(-1), S[sc.argmax(-1)]


def smooth_ref(x, thr, on, off, lengths=None, act=None):
    """(B, P, T) float32 logits -> what mt_frame_smooth leaves in an output that started as a copy of x."""
    x = np.asarray(x, np.float32)
    B, P, T = x.shape
    a, b = penalty(on), penalty(off)
    out = x.copy()
    for i in range(B):
        L = T if lengths is None else int(min(T, max(0, lengths[i])))
        q = quantise(x[i, :, :L], thr, None if act is None else np.asarray(act, bool)[i, :, :L])
        out[i, :, :L] = np.where(viterbi_path(q, a, b), Y_ON, Y_OFF)
    return out
