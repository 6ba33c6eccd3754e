"""Numpy restatement of the offset-gated note decoder (helper module of the offset-decoder tests; not collected).

`onset_offset_notes` is the rule scanned literally, frame by frame, on boolean activity rows of one pitch:
    a[t] = f[t] | o[t]     st[t] = o[t] & !o[t-1]     e[t] = k[t] & !k[t-1]          (everything before frame 0 is inactive)
    open[t] = st[t] | (open[t-1] & a[t] & !e[t-1])
A note starts at every t with st[t]; the note open after t-1 ends at t when open[t-1] & (!open[t] | st[t]); a note still open at the
end of the row ends there.  The wrappers plug it into the matchers of note_metrics_ref / note_list_ref, so expected counts come from
scipy's maximum matching as in the other note tests.
"""
import numpy as np

import note_list_ref as LR
import note_metrics_ref as NR


def logit(p):
    return float(np.log(p / (1.0 - p)))


def markov(rng, shape, p_on, p_off):
    """Boolean rows of runs: a two-state chain along the last axis."""
    u = rng.random(shape)
    out = np.zeros(shape, bool)
    state = rng.random(shape[:-1]) < p_on / (p_on + p_off)
    for t in range(shape[-1]):
        state = np.where(state, u[..., t] >= p_off, u[..., t] < p_on)
        out[..., t] = state
    return out


def onset_offset_notes(f, o, k):
    f, o, k = np.asarray(f, bool), np.asarray(o, bool), np.asarray(k, bool)
    notes, start = [], None
    open_prev = o_prev = k_prev = e_prev = False
    for t in range(len(f)):
        a = bool(f[t] or o[t])
        st = bool(o[t]) and not o_prev
        e = bool(k[t]) and not k_prev
        open_t = st or (open_prev and a and not e_prev)
        if open_prev and (not open_t or st):
            notes.append((start, t))
            start = None
        if st:
            start = t
        open_prev, o_prev, k_prev, e_prev = open_t, bool(o[t]), bool(k[t]), e
    if open_prev:
        notes.append((start, len(f)))
    return notes


def _length(lengths, b, T):
    return T if lengths is None else int(min(T, max(0, int(lengths[b]))))


def match_counts_active(f_act, o_act, k_act, ref, lengths=None):
    """(B, P, T) boolean activities of the three heads and the reference roll -> (B, 4): what mt_note_match_counts_off returns."""
    f_act, o_act, k_act, ref = np.asarray(f_act, bool), np.asarray(o_act, bool), np.asarray(k_act, bool), np.asarray(ref, np.float32)
    B, P, T = f_act.shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = _length(lengths, b, T)
        for p in range(P):
            est = onset_offset_notes(f_act[b, p, :L], o_act[b, p, :L], k_act[b, p, :L])
            out[b] += NR.row_counts(NR.frame_notes(ref[b, p, :L] > 0), est)
    return out


def match_list_counts_active(f_act, o_act, k_act, ref_on, ref_off, ref_ptr, lengths=None):
    """The same against a note list in ticks: what mt_note_match_list_off returns."""
    f_act, o_act, k_act = np.asarray(f_act, bool), np.asarray(o_act, bool), np.asarray(k_act, bool)
    B, P, T = f_act.shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = _length(lengths, b, T)
        for p in range(P):
            est = onset_offset_notes(f_act[b, p, :L], o_act[b, p, :L], k_act[b, p, :L])
            lo, hi = int(ref_ptr[b * P + p]), int(ref_ptr[b * P + p + 1])
            on, off = LR.clip_notes(ref_on[lo:hi], ref_off[lo:hi], L)
            out[b] += LR.list_row_counts(on, off, est)
    return out


def heads_notes_active(f_act, o_act, k_act):
    """(NB, P, T) activities -> [(pitch index, start, end)] over the chunks concatenated in time, pitch-major (mt_heads_to_notes_off)."""
    f_act, o_act, k_act = np.asarray(f_act, bool), np.asarray(o_act, bool), np.asarray(k_act, bool)
    out = []
    for p in range(f_act.shape[1]):
        out += [(p, s, e) for s, e in onset_offset_notes(f_act[:, p].reshape(-1), o_act[:, p].reshape(-1), k_act[:, p].reshape(-1))]
    return out
