"""Numpy restatement of the sub-frame onset rules (helper module of the onset-regression tests; not collected).

`regress_target` = mt_onset_regress_windows in integers (units of 12.5 us: a 16 kHz sample is 5, a tick of 100 us 8, a frame 2560) with one
float32 division; `refine_onsets` = mt_refine_onsets in float64.  DESIGN.md 6c "Sub-frame onsets".
"""
import numpy as np

UNITS_PER_SAMPLE, UNITS_PER_TICK, UNITS_PER_FRAME, TICKS_PER_FRAME = 5, 8, 2560, 320
ONE_Q32 = 1 << 32


def frame_centres(start, T_out, rate_q32=None):
    """tau of frames 0 .. T_out - 1 of a window whose first sample is `start`, int64 units of 12.5 us."""
    t = np.arange(T_out, dtype=np.int64)
    rate = ONE_Q32 if rate_q32 is None else int(rate_q32)
    assert T_out <= 1 << 19 and rate < 1 << 33                     # 2560 t rate + 2^31 stays below 2^63
    return UNITS_PER_SAMPLE * int(start) + ((UNITS_PER_FRAME * t * rate + (1 << 31)) >> 32)


def regress_target(on_tick, tick_off, win_rec, start, t_keep, T_out, J, rate_q32=None):
    """(B, 88, T_out) float32: on_tick int32 of all recordings, tick_off int64 (R * 89,), per window its recording, first sample, kept
    frames and (optionally) speed."""
    on_tick, tick_off = np.asarray(on_tick, np.int64), np.asarray(tick_off, np.int64)
    B, W = len(win_rec), UNITS_PER_FRAME * int(J)
    out = np.zeros((B, 88, T_out), np.float32)
    for b in range(B):
        keep = min(int(t_keep[b]), T_out)
        tau = frame_centres(start[b], T_out, None if rate_q32 is None else rate_q32[b])[:keep]
        for p in range(88):
            lo, hi = (int(v) for v in tick_off[int(win_rec[b]) * 89 + p:int(win_rec[b]) * 89 + p + 2])
            if hi == lo or not keep:
                continue
            d = np.abs(tau[:, None] - UNITS_PER_TICK * on_tick[None, lo:hi]).min(axis=1)
            y = (W - d).astype(np.float32) / np.float32(W)         # one correctly rounded float32 division of exact integers
            out[b, p, :keep] = np.where(d < W, y, np.float32(0.0))
    return out


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def refine_one(q, s, e, reach):
    """One note [s, e) of a row whose valid frames hold the float64 probabilities q (length L) -> (on_tick, k, B - m)."""
    L = len(q)
    at = lambda g: float(q[g]) if 0 <= g < L else 0.0
    k = s
    while k + 1 <= min(s + reach, e - 1, L - 1) and at(k + 1) > at(k):
        k += 1
    A, B, C = at(k - 1), at(k), at(k + 1)
    m = min(A, C)
    if B - m < 2.0 ** -10:
        shift = 0.0
    elif C > A:
        shift = (C - A) / (2.0 * (B - A))
    else:
        shift = (C - A) / (2.0 * (B - C))
    shift = min(max(shift, -0.5), 0.5)
    tick = TICKS_PER_FRAME * k + int(np.rint(TICKS_PER_FRAME * shift))
    return min(max(tick, 0), TICKS_PER_FRAME * e - 1), k, B - m


def refine_onsets(rows_q, starts, ends, row_off, reach):
    """rows_q[r] = the float64 probabilities of row r's valid frames; the notes of row r are starts / ends[row_off[r]:row_off[r + 1]].
    -> (on_tick int64 (n,), margin float64 (n,) = B - m of every note)."""
    ticks, margin = np.zeros(len(starts), np.int64), np.zeros(len(starts), np.float64)
    for r, q in enumerate(rows_q):
        for i in range(int(row_off[r]), int(row_off[r + 1])):
            ticks[i], _, margin[i] = refine_one(q, int(starts[i]), int(ends[i]), reach)
    return ticks, margin


def onset_notes_of(active):
    """The runs of a boolean row as [s, e) pairs (the onset-gated decoder on frame = onset: a note opens at each rising edge)."""
    a = np.concatenate([[False], np.asarray(active, bool), [False]])
    d = np.diff(a.astype(np.int8))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))
