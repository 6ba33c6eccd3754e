"""Numpy restatement of the decoders' note cleanup (DESIGN.md 6c "Note cleanup"; helper module of the note-cleanup tests; not collected).

`clean_notes(f, o, k, M, G)` is the rule scanned literally, frame by frame, on the boolean activity rows of one pitch (o None: the
frame decoder, k None: no offset head):
  1. bridge: a = f | o; every inactive run of a of at most G frames that has an active frame directly before it and directly after
     it is filled (leading runs and runs that reach the end of the row are not).  The frame decoder takes f' for f and for o; the
     other two keep their onset (and offset) rows.
  2. decode: open[t] = st[t] | (open[t-1] & a'[t] & !e[t-1]), st / e the rising edges of o / k; a note starts at every st[t], the
     open note ends at t when open[t-1] & (!open[t] | st[t]), and a note still open at the end of the row ends there.
  3. drop: every note [s, e) with e - s < M goes.
The wrappers plug it into the matchers of note_metrics_ref / note_list_ref, so expected counts come from scipy's maximum matching.
"""
import numpy as np

import note_list_ref as LR
import note_metrics_ref as NR
from offset_decode_ref import _length

M_MAX, G_MAX = 64, 63


def bridge(a, G):
    """a with its interior inactive runs of at most G frames filled, scanned frame by frame."""
    a = [bool(v) for v in a]
    out = list(a)
    seen, run = False, 0                                  # an active frame so far; length of the inactive run that ends before t
    for t, v in enumerate(a):
        if not v:
            run += 1
            continue
        if seen and 0 < run <= G:
            for u in range(t - run, t):
                out[u] = True
        seen, run = True, 0
    return np.asarray(out, bool)


def decode(a, o, k):
    """The decoders' rule on activity a, onset o and offset k rows."""
    notes, start = [], None
    open_prev = o_prev = k_prev = e_prev = False
    for t in range(len(a)):
        st = bool(o[t]) and not o_prev
        e = bool(k[t]) and not k_prev
        open_t = st or (open_prev and bool(a[t]) and not e_prev)
        if open_prev and (not open_t or st):
            notes.append((start, t))
        if st:
            start = t
        open_prev, o_prev, k_prev, e_prev = open_t, bool(o[t]), bool(k[t]), e
    if open_prev:
        notes.append((start, len(a)))
    return notes


def clean_notes(f, o=None, k=None, M=1, G=0):
    assert 1 <= M <= M_MAX and 0 <= G <= G_MAX
    f = np.asarray(f, bool)
    if o is None:
        assert k is None
        a = bridge(f, G)
        o = a
    else:
        o = np.asarray(o, bool)
        a = bridge(f | o, G)
    k = np.zeros(len(f), bool) if k is None else np.asarray(k, bool)
    return [(s, e) for s, e in decode(a, o, k) if e - s >= M]


def frame_notes_list_rule(f, M, G):
    """The frame decoder's cleanup restated on note lists: merge neighbours whose gap is <= G, then drop those shorter than M."""
    merged = []
    for s, e in NR.frame_notes(np.asarray(f, bool)):
        if merged and s - merged[-1][1] <= G:
            merged[-1] = (merged[-1][0], e)
        else:
            merged.append((s, e))
    return [(s, e) for s, e in merged if e - s >= M]


def _row(x, b, p, L):
    return None if x is None else np.asarray(x, bool)[b, p, :L]


def match_counts_active(f_act, ref, o_act=None, k_act=None, lengths=None, M=1, G=0):
    """(B, P, T) boolean activities and the reference roll -> (B, 4): what mt_note_match_counts_clean returns."""
    ref = np.asarray(ref, np.float32)
    B, P, T = np.asarray(f_act).shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = _length(lengths, b, T)
        for p in range(P):
            est = clean_notes(_row(f_act, b, p, L), _row(o_act, b, p, L), _row(k_act, b, p, L), M, G)
            out[b] += NR.row_counts(NR.frame_notes(ref[b, p, :L] > 0), est)
    return out


def match_list_counts_active(f_act, ref_on, ref_off, ref_ptr, o_act=None, k_act=None, lengths=None, M=1, G=0):
    """The same against a note list in ticks: what mt_note_match_list_clean returns."""
    B, P, T = np.asarray(f_act).shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = _length(lengths, b, T)
        for p in range(P):
            est = clean_notes(_row(f_act, b, p, L), _row(o_act, b, p, L), _row(k_act, b, p, L), M, G)
            lo, hi = int(ref_ptr[b * P + p]), int(ref_ptr[b * P + p + 1])
            on, off = LR.clip_notes(ref_on[lo:hi], ref_off[lo:hi], L)
            out[b] += LR.list_row_counts(on, off, est)
    return out


def heads_notes_active(f_act, o_act=None, k_act=None, M=1, G=0):
    """(NB, P, T) activities -> [(pitch index, start, end)] over the chunks concatenated in time, pitch-major (mt_heads_to_notes_clean)."""
    cat = lambda x, p: None if x is None else np.asarray(x, bool)[:, p].reshape(-1)
    out = []
    for p in range(np.asarray(f_act).shape[1]):
        out += [(p, s, e) for s, e in clean_notes(cat(f_act, p), cat(o_act, p), cat(k_act, p), M, G)]
    return out


def batch_notes_active(f_act, o_act=None, lengths=None, M=1, G=0):
    """(B, P, T) activities with lengths -> per recording [(pitch index, start, end)], pitch-major (mt_notes_batch_clean)."""
    B, P, T = np.asarray(f_act).shape
    out = []
    for b in range(B):
        L = _length(lengths, b, T)
        out.append([(p, s, e) for p in range(P) for s, e in clean_notes(_row(f_act, b, p, L), _row(o_act, b, p, L), None, M, G)])
    return out
