"""Numpy restatement of note matching against a note list in ticks (helper module of the note-list tests; not collected).

Times are integers: ticks of 100 us, one model frame (512 / 16000 s) = 320 ticks.  An estimated note [s, e) in frames has times
320 s, 320 e.  mir_eval's criteria (distances to 4 decimals) in these integers:
    onset:          |on_r - on_e| <= 500
    onset + offset: also 5 |off_r - off_e| <= max(2500, off_r - on_r)
`max_matching_ticks` is scipy's maximum bipartite matching of the explicit graph; `stream_matching` is the one-pass rule of
mt_note_match_list, restated literally: reference notes are edges on the estimates (a loop at j, or a link j -- j+1),
a component of V estimates with E edges contributes min(E, V).
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

from note_metrics_ref import frame_notes, onset_notes, sigmoid_active

TICKS_PER_FRAME = 320
ONSET_TOL = 500
NO_NOTE = -4096


def compatible_ticks(ref_on, ref_off, est, with_offset):
    ref_on, ref_off = np.asarray(ref_on, np.int64), np.asarray(ref_off, np.int64)
    e = np.asarray(est, np.int64).reshape(-1, 2) * TICKS_PER_FRAME
    ok = np.abs(ref_on[:, None] - e[None, :, 0]) <= ONSET_TOL
    if with_offset:
        ok &= 5 * np.abs(ref_off[:, None] - e[None, :, 1]) <= np.maximum(2500, ref_off - ref_on)[:, None]
    return ok


def max_matching_ticks(ref_on, ref_off, est, with_offset):
    if not len(ref_on) or not len(est):
        return 0
    g = csr_matrix(compatible_ticks(ref_on, ref_off, est, with_offset).astype(np.int8))
    return int((maximum_bipartite_matching(g, perm_type="column") >= 0).sum())


class _Crit:
    def __init__(self):
        self.v_a = self.e_a = self.e_cur = self.links = self.tp = 0

    def edge(self, with_prev, with_cur):
        if with_prev and with_cur:
            self.links += 1
        elif with_prev:
            self.e_a += 1
        elif with_cur:
            self.e_cur += 1

    def shift(self):
        if self.links:
            self.v_a += 1
            self.e_a += self.e_cur + self.links
        else:
            self.tp += min(self.e_a, self.v_a)
            self.v_a, self.e_a = 1, self.e_cur
        self.e_cur = self.links = 0


def stream_matching(ref_on, ref_off, est):
    """(tp_onset, tp_onset_offset) by the streaming rule: estimates in order; when estimate k+1 starts, every unread reference note
    with on < on_{k+1} - 500 is read against estimates k-1 and k."""
    ref_on, ref_off = [int(x) for x in ref_on], [int(x) for x in ref_off]
    c_on, c_onoff = _Crit(), _Crit()
    prev, cur, at = (NO_NOTE, NO_NOTE), (NO_NOTE, NO_NOTE), 0

    def drain(limit):
        nonlocal at
        while at < len(ref_on) and ref_on[at] < limit:
            on_r, off_r = ref_on[at], ref_off[at]
            tol = max(ONSET_TOL, (off_r - on_r) // 5)
            p_on, k_on = abs(on_r - prev[0]) <= ONSET_TOL, abs(on_r - cur[0]) <= ONSET_TOL
            c_on.edge(p_on, k_on)
            c_onoff.edge(p_on and abs(off_r - prev[1]) <= tol, k_on and abs(off_r - cur[1]) <= tol)
            at += 1
    for s, e in est:
        drain(TICKS_PER_FRAME * int(s) - ONSET_TOL)
        c_on.shift()
        c_onoff.shift()
        prev, cur = cur, (TICKS_PER_FRAME * int(s), TICKS_PER_FRAME * int(e))
    drain(1 << 62)
    c_on.shift()
    c_onoff.shift()
    return c_on.tp + min(c_on.e_a, c_on.v_a), c_onoff.tp + min(c_onoff.e_a, c_onoff.v_a)


def clip_notes(ref_on, ref_off, L):
    """The notes mt_note_match_list reads with L valid frames: on < 320 L, offsets clipped to 320 L."""
    ref_on, ref_off = np.asarray(ref_on, np.int64), np.asarray(ref_off, np.int64)
    keep = ref_on < TICKS_PER_FRAME * L
    return ref_on[keep], np.minimum(ref_off[keep], TICKS_PER_FRAME * L)


def list_row_counts(ref_on, ref_off, est, matcher="scipy"):
    if matcher == "scipy":
        tp = max_matching_ticks(ref_on, ref_off, est, False), max_matching_ticks(ref_on, ref_off, est, True)
    else:
        tp = stream_matching(ref_on, ref_off, est)
    return np.array([len(ref_on), len(est), tp[0], tp[1]], np.int64)


def match_list_counts_active(f_act, ref_on, ref_off, ref_ptr, o_act=None, lengths=None, matcher="scipy"):
    """(B, P, T) boolean frame activity (and onset activity for the onset-gated decoder) and the note list -> (B, 4)
    {n_ref, n_est, tp_onset, tp_onset_offset}: what mt_note_match_list returns."""
    f_act = np.asarray(f_act, bool)
    B, P, T = f_act.shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = T if lengths is None else int(min(T, max(0, int(lengths[b]))))
        for p in range(P):
            est = frame_notes(f_act[b, p, :L]) if o_act is None else onset_notes(f_act[b, p, :L], np.asarray(o_act, bool)[b, p, :L])
            lo, hi = int(ref_ptr[b * P + p]), int(ref_ptr[b * P + p + 1])
            on, off = clip_notes(ref_on[lo:hi], ref_off[lo:hi], L)
            out[b] += list_row_counts(on, off, est, matcher)
    return out


def match_list_counts(frame, ref_on, ref_off, ref_ptr, thr, onset=None, onset_thr=0.5, lengths=None, matcher="scipy"):
    """As match_list_counts_active, from logits (activity = sigmoid_active)."""
    o_act = None if onset is None else sigmoid_active(onset, onset_thr)
    return match_list_counts_active(sigmoid_active(frame, thr), ref_on, ref_off, ref_ptr, o_act, lengths, matcher)


def notes_from_roll(ref):
    """The runs of a (B, P, T) roll as a note list on the frame grid: (on, off int32, ptr int64 (B*P + 1,))."""
    ref = np.asarray(ref)
    B, P, T = ref.shape
    on, off, ptr = [], [], [0]
    for b in range(B):
        for p in range(P):
            for s, e in frame_notes(ref[b, p] > 0):
                on.append(TICKS_PER_FRAME * s)
                off.append(TICKS_PER_FRAME * e)
            ptr.append(len(on))
    return np.array(on, np.int32), np.array(off, np.int32), np.array(ptr, np.int64)
