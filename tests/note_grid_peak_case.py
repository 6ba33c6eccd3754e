"""The case of the peak-grid tests and its numpy restatement (helper module of test_gpu_note_grid_peak.py / test_note_grid_peak_cpu.py;
not collected; numpy only).

The case is note_grid_case.Case (12 x 5 x 1100 with LENGTHS) with the onset head replaced by a copy with planted plateaus -- equal logits
on frames 63|64, 511|512, 1023|1024, 0|1 and L-2|L-1 of every row that has them -- and planted maxima within 8 frames of either side of
512 and 1024, so that a peak's neighbours cross the window, slab and row boundaries and ties break on both sides of each.

`ridge(x, R)` is the threshold-free half of peak_decode_ref.peak_mask (DESIGN.md 6c "Peak picking in the decoder grid"): bit t = x[t] is
> every existing x[u], u in [t-R, t-1], and >= every existing x[u], u in [t+1, t+R].  `starts(x, o, R)` = the frames where a note opens at
reach R: o & ridge(x, R), or for R = 0 the rising edges of o.  `fast_notes` is peak_decode_ref.peak_notes in array operations (the CPU
test holds the two against each other); `cpu_counts` restates the grid with them and the matchers of note_metrics_ref / note_list_ref.
"""
import numpy as np

import note_grid_case as GC
import note_list_ref as LR
import note_metrics_ref as NR
from note_clean_ref import bridge
from note_grid_case import B, GRID_64, LENGTHS, P, POOL, T
from offset_decode_ref import _length

SEED = 0                                  # test_note_grid_peak_cpu.py asserts the coverage condition on this seed
REACHES = [0, 1, 2, 8]
CLEANUPS_2 = [(1, 0), (3, 2)]
GRID_PEAK = dict(tf=GRID_64["tf"], to=GRID_64["to"], tk=GRID_64["tk"], cleanups=CLEANUPS_2, reaches=REACHES)      # 2 x 2 x (1 | 2) x 2 x 4


def planted_onset(case):
    x = np.array(case.onset, np.float32)
    for b in range(B):
        L = LENGTHS[b]
        for p in range(P):
            v = np.float32(2.5 + 0.25 * p + 0.125 * (b % 3))               # sigmoid 0.92 .. 0.98: passes every threshold of POOL
            for edge in (512, 1024):                                        # maxima near the slab boundary, some on both sides at once
                for d in ((-2 - (p + b) % 7, 1 + (2 * p + b) % 7) if (p + b) % 2 else (2 + (p + 3 * b) % 6,)):
                    if 0 <= edge + d < L:
                        x[b, p, edge + d] = np.float32(4.5 + 0.01 * abs(d))
            for t in (63, 511, 1023, 0, L - 2):                             # (after the maxima: a plateau near a row's end wins)
                if 0 <= t and t + 1 < L:
                    x[b, p, t] = x[b, p, t + 1] = v
    x.setflags(write=False)
    return x


def ridge(x, R):
    x = np.asarray(x, np.float32)
    L = len(x)
    out = np.ones(L, bool)
    for d in range(1, R + 1):
        out[d:] &= x[d:] > x[:L - d] if L > d else True
        out[:L - d] &= x[:L - d] >= x[d:] if L > d else True
    return out


def starts(x, o, R):
    o = np.asarray(o, bool)
    if R == 0:
        return o & ~np.concatenate([[False], o[:-1]])
    return o & ridge(x, R)


def fast_notes(f, o, st, k=None, M=1, G=0):
    """peak_decode_ref.peak_notes without a loop over frames: open[t] <=> the last start at or before t is not older than the last frame
    at or before t on which the note cannot stay open."""
    f, o, st = np.asarray(f, bool), np.asarray(o, bool), np.asarray(st, bool)
    L = len(f)
    if L == 0:
        return []
    a = np.asarray(bridge(f | o, G), bool)
    if k is not None:
        k = np.asarray(k, bool)
        e = k & ~np.concatenate([[False], k[:-1]])
        a = a & ~np.concatenate([[False], e[:-1]])
    idx = np.arange(L)
    last_start = np.maximum.accumulate(np.where(st, idx, -1))
    last_stop = np.maximum.accumulate(np.where(~a, idx, -1))
    is_open = (last_start >= 0) & (last_start >= last_stop)
    s = np.flatnonzero(st)
    closed = np.flatnonzero(~is_open)
    nxt = np.append(s[1:], L)
    at = np.searchsorted(closed, s, side="right")
    first_closed = np.where(at < len(closed), np.append(closed, L)[at], L)
    ends = np.minimum(nxt, first_closed)
    return [(int(a0), int(b0)) for a0, b0 in zip(s, ends) if b0 - a0 >= M]


class Case(GC.Case):
    def __init__(self, seed=SEED):
        super().__init__(seed)
        self.onset = planted_onset(self)                    # (host_act("onset", ...) reads it from here)


def cpu_counts(case, kind, decoder, tf, to, tk, cleanups, reaches, lengths, act=None):
    """(B, Kf, Ko, Kk, Kc, Kr, 4): the peak grid's contract restated; decoder "onset" / "onset_offset"."""
    act = act or case.host_act
    tk = tk if decoder == "onset_offset" else [None]
    out = np.zeros((B, len(tf), len(to), len(tk), len(cleanups), len(reaches), 4), np.int64)
    refs = {}
    for j, o in enumerate(to):
        o_act = act("onset", o)
        for b in range(B):
            L = _length(lengths, b, T)
            for p in range(P):
                if (b, p) not in refs:
                    if kind == "roll":
                        refs[b, p] = NR.frame_notes(case.ref[b, p, :L] > 0)
                    else:
                        lo, hi = int(case.notes[2][b * P + p]), int(case.notes[2][b * P + p + 1])
                        refs[b, p] = LR.clip_notes(case.notes[0][lo:hi], case.notes[1][lo:hi], L)
                ob = o_act[b, p, :L]
                sts = [starts(case.onset[b, p, :L], ob, R) for R in reaches]
                for i, a in enumerate(tf):
                    f = act("frame", a)[b, p, :L]
                    for k, kt in enumerate(tk):
                        kb = None if kt is None else act("offset", kt)[b, p, :L]
                        for c, (M, G) in enumerate(cleanups):
                            for r, st in enumerate(sts):
                                est = fast_notes(f, ob, st, kb, M, G)
                                if kind == "roll":
                                    out[b, i, j, k, c, r] += NR.row_counts(refs[b, p], est)
                                else:
                                    out[b, i, j, k, c, r] += LR.list_row_counts(*refs[b, p], est)
    return out
