"""Numpy restatement of peak-picked onsets in the note decoders (DESIGN.md 6c "Peak-picked onsets"; helper module of the peak-decoding
tests; not collected).

`peak_mask(x, o, R)` is the rule in plain loops on one pitch row of L valid frames, x its onset logits and o its onset activity
(sigmoid(x) > thr_onset, the kernels' float32 expression): frame t is an onset iff o[t], x[t] > x[u] for every existing u in
[t - R, t - 1] and x[t] >= x[u] for every existing u in [t + 1, t + R].  Frames outside [0, L) do not exist.

`peak_notes(f, o, st, k, M, G)` is note_clean_ref.clean_notes with the starts given: the activity a = f | o is bridged by
note_clean_ref.bridge, `decode_starts` is note_clean_ref.decode with st[t] in place of the rising edge of o, and notes shorter than M
are dropped.  The wrappers plug it into the matchers of note_metrics_ref / note_list_ref, as note_clean_ref's do.
"""
import numpy as np

import note_list_ref as LR
import note_metrics_ref as NR
from note_clean_ref import bridge
from offset_decode_ref import _length

R_MAX = 8


def peak_mask(x, o, R):
    assert 1 <= R <= R_MAX
    x, o = np.asarray(x, np.float32), np.asarray(o, bool)
    L = len(x)
    out = np.zeros(L, bool)
    for t in range(L):
        if not o[t]:
            continue
        ok = True
        for u in range(max(0, t - R), t):
            ok = ok and bool(x[t] > x[u])
        for u in range(t + 1, min(L, t + R + 1)):
            ok = ok and bool(x[t] >= x[u])
        out[t] = ok
    return out


def decode_starts(a, st, k):
    """note_clean_ref.decode with the start mask given: open[t] = st[t] | (open[t-1] & a[t] & !e[t-1]), e the rising edges of k."""
    notes, start = [], None
    open_prev = k_prev = e_prev = False
    for t in range(len(a)):
        s = bool(st[t])
        e = bool(k[t]) and not k_prev
        open_t = s or (open_prev and bool(a[t]) and not e_prev)
        if open_prev and (not open_t or s):
            notes.append((start, t))
        if s:
            start = t
        open_prev, k_prev, e_prev = open_t, bool(k[t]), e
    if open_prev:
        notes.append((start, len(a)))
    return notes


def peak_notes(f, o, st, k=None, M=1, G=0):
    f, o, st = np.asarray(f, bool), np.asarray(o, bool), np.asarray(st, bool)
    assert not (st & ~o).any()                              # every onset frame is onset-active
    a = bridge(f | o, G)
    k = np.zeros(len(f), bool) if k is None else np.asarray(k, bool)
    return [(s, e) for s, e in decode_starts(a, st, k) if e - s >= M]


def row_notes(xf, xo, xk, L, R, M=1, G=0, thr=(0.5, 0.5, 0.5)):
    """One row's notes from its logits (xk None: no offset head); frames at or past L are not looked at."""
    f, o = NR.sigmoid_active(xf[:L], thr[0]), NR.sigmoid_active(xo[:L], thr[1])
    k = None if xk is None else NR.sigmoid_active(xk[:L], thr[2])
    return peak_notes(f, o, peak_mask(xo[:L], o, R), k, M, G)


def match_counts(xf, xo, xk, ref, lengths, R, M=1, G=0):
    """(B, P, T) logits and the reference roll -> (B, 4): what mt_note_match_counts_peak returns at thresholds 0.5."""
    B, P, T = xf.shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = _length(lengths, b, T)
        for p in range(P):
            est = row_notes(xf[b, p], xo[b, p], None if xk is None else xk[b, p], L, R, M, G)
            out[b] += NR.row_counts(NR.frame_notes(np.asarray(ref)[b, p, :L] > 0), est)
    return out


def match_list_counts(xf, xo, xk, ref_on, ref_off, ref_ptr, lengths, R, M=1, G=0):
    """The same against a note list in ticks: what mt_note_match_list_peak returns."""
    B, P, T = xf.shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = _length(lengths, b, T)
        for p in range(P):
            est = row_notes(xf[b, p], xo[b, p], None if xk is None else xk[b, p], L, R, M, G)
            lo, hi = int(ref_ptr[b * P + p]), int(ref_ptr[b * P + p + 1])
            on, off = LR.clip_notes(ref_on[lo:hi], ref_off[lo:hi], L)
            out[b] += LR.list_row_counts(on, off, est)
    return out


def heads_notes(xf, xo, xk, R, M=1, G=0):
    """(NB, P, T) logits -> [(pitch index, start, end)] over the chunks concatenated in time, pitch-major (mt_heads_to_notes_peak)."""
    NB, P, T = xf.shape
    cat = lambda x, p: None if x is None else np.ascontiguousarray(x[:, p]).reshape(-1)
    out = []
    for p in range(P):
        out += [(p, s, e) for s, e in row_notes(cat(xf, p), cat(xo, p), cat(xk, p), NB * T, R, M, G)]
    return out


def batch_notes(xf, xo, lengths, R, M=1, G=0):
    """(B, P, T) logits with lengths -> per recording [(pitch index, start, end)], pitch-major (mt_notes_batch_peak)."""
    B, P, T = xf.shape
    out = []
    for b in range(B):
        L = _length(lengths, b, T)
        out.append([(p, s, e) for p in range(P) for s, e in row_notes(xf[b, p], xo[b, p], None, L, R, M, G)])
    return out


# ------------------------------------------------------------------------------------------------ the merge demonstration
def triangle_pairs():
    """Two note-ons of one pitch `gap` ticks apart under triangular targets of width J, as (J, first on_tick, gap in ticks), the gaps
    between 2 frames and J frames.  Frame t is centred on tick 320 t, so a frame's distance to a note-on at phase ph is ph or 320 - ph
    (mod 320).  The first phase is 23 and no gap is 0 or -46 mod 320 except the whole-frame gap 640, so neighbouring frames never see
    equal distances: at gap 640 the two vertices tie with each other, two frames apart, which reach 1 does not compare."""
    out = []
    for J in (2, 4, 8):
        for gap in sorted({640, 640 + 37, (J + 2) * 160 + 11, J * 320 - 53, J * 320 - 7}):
            if 640 <= gap <= J * 320:
                out.append((J, 320 * 10 + 23, gap))
    return out


def triangle_row(J, on, gap, T=48):
    """The target row (float64 of the float32 target, T frames) of the two note-ons and its logits; targets 0 / 1 map to logits -30 / 30."""
    import onset_regress_ref as OG
    ticks = np.array([on, on + gap], np.int32)
    off = np.zeros(89, np.int64)
    off[1:] = 2                                                       # both notes on pitch row 0
    y = OG.regress_target(ticks, off, [0], [0], [T], T, J)[0, 0].astype(np.float64)
    with np.errstate(divide="ignore"):
        x = np.clip(np.log(y) - np.log1p(-y), -30.0, 30.0).astype(np.float32)
    return y, x
