"""Numpy restatement of the note decoders and of mir_eval's note matching (helper module of the note tests; not collected).

Decoders work on boolean activity rows of one pitch.  The matching follows mir_eval.transcription.match_notes: times in
seconds, distances rounded to 4 decimals, maximum bipartite matching of the explicit compatibility graph
(scipy.sparse.csgraph.maximum_bipartite_matching).  The offset tolerance max(50 ms, 0.2 * reference length) is rounded to 4
decimals as well: on the 32 ms grid it is then exact (0.0064 * length), where the unrounded product can land one float ulp
below an exactly equal distance.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

FS = 16000 / 512
N_DECIMALS = 4


def sigmoid_active(x, thr):
    """The kernels' expression 1 / (1 + exp(-x)) > thr in float32 (tests keep logits off the threshold's ulp band)."""
    x = np.asarray(x, np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))) > np.float32(thr)


def frame_notes(f):
    """Maximal runs of active frames: [(start, end)]."""
    f = np.asarray(f, bool).astype(np.int8)
    d = np.diff(np.concatenate([[0], f, [0]]))
    return list(zip(np.where(d == 1)[0].tolist(), np.where(d == -1)[0].tolist()))


def onset_notes(f, o):
    """The onset-gated decoder, scanned literally: a = f | o; close on !a, re-open on a rising onset edge, open on onset."""
    f, o = np.asarray(f, bool), np.asarray(o, bool)
    notes, start, prev_o = [], None, False
    for g in range(len(f)):
        a = f[g] or o[g]
        if start is not None and not a:
            notes.append((start, g))
            start = None
        elif start is not None and o[g] and not prev_o:
            notes.append((start, g))
            start = g
        elif start is None and o[g]:
            start = g
        prev_o = bool(o[g])
    if start is not None:
        notes.append((start, len(f)))
    return notes


def _compatible(ref, est, with_offset):
    ref_s = np.asarray(ref, np.float64).reshape(-1, 2) / FS
    est_s = np.asarray(est, np.float64).reshape(-1, 2) / FS
    on = np.around(np.abs(np.subtract.outer(ref_s[:, 0], est_s[:, 0])), N_DECIMALS) <= 0.05
    if not with_offset:
        return on
    off = np.around(np.abs(np.subtract.outer(ref_s[:, 1], est_s[:, 1])), N_DECIMALS)
    tol = np.around(np.maximum(0.05, 0.2 * (ref_s[:, 1] - ref_s[:, 0])), N_DECIMALS)
    return on & (off <= tol[:, None])


def max_matching(ref, est, with_offset):
    """Size of a maximum matching between reference and estimated notes [(start, end)] of one pitch (mir_eval's rule)."""
    if not len(ref) or not len(est):
        return 0
    g = csr_matrix(_compatible(ref, est, with_offset).astype(np.int8))
    return int((maximum_bipartite_matching(g, perm_type="column") >= 0).sum())


def greedy_matching(ref, est, with_offset):
    """Each reference note, in time order, takes the earliest unmatched compatible estimate."""
    if not len(ref) or not len(est):
        return 0
    c = _compatible(ref, est, with_offset)
    used = np.zeros(len(est), bool)
    tp = 0
    for i in range(len(ref)):
        for j in range(len(est)):
            if c[i, j] and not used[j]:
                used[j] = True
                tp += 1
                break
    return tp


def row_counts(ref_notes, est_notes):
    return np.array([len(ref_notes), len(est_notes), max_matching(ref_notes, est_notes, False), max_matching(ref_notes, est_notes, True)],
                    np.int64)


def match_counts_active(f_act, ref, o_act=None, lengths=None):
    """(B, P, T) boolean frame activity (and onset activity for the onset-gated decoder) and reference roll -> (B, 4)
    {n_ref, n_est, tp_onset, tp_onset_offset}: what mt_note_match_counts returns."""
    f_act, ref = np.asarray(f_act, bool), np.asarray(ref, np.float32)
    B, P, T = f_act.shape
    out = np.zeros((B, 4), np.int64)
    for b in range(B):
        L = T if lengths is None else int(min(T, max(0, int(lengths[b]))))
        for p in range(P):
            est = frame_notes(f_act[b, p, :L]) if o_act is None else onset_notes(f_act[b, p, :L], np.asarray(o_act, bool)[b, p, :L])
            out[b] += row_counts(frame_notes(ref[b, p, :L] > 0), est)
    return out


def match_counts(frame, ref, thr, onset=None, onset_thr=0.5, lengths=None):
    """As match_counts_active, from logits (activity = sigmoid_active)."""
    o_act = None if onset is None else sigmoid_active(onset, onset_thr)
    return match_counts_active(sigmoid_active(frame, thr), ref, o_act, lengths)


def heads_notes(frame, onset, thr, onset_thr):
    """(NB, P, T) logits -> [(pitch index, start, end)] of the onset-gated decoder over the chunks concatenated in time, pitch-major."""
    frame, onset = np.asarray(frame, np.float32), np.asarray(onset, np.float32)
    NB, P, T = frame.shape
    out = []
    for p in range(P):
        f = sigmoid_active(frame[:, p, :].reshape(-1), thr)
        o = sigmoid_active(onset[:, p, :].reshape(-1), onset_thr)
        out += [(p, s, e) for s, e in onset_notes(f, o)]
    return out


def prf(tp, n_ref, n_est):
    p = tp / n_est if n_est else 0.0
    r = tp / n_ref if n_ref else 0.0
    f = 2.0 * tp / (n_ref + n_est) if (n_ref + n_est) else 0.0
    return p, r, f
