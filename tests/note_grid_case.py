"""The case of the decoder-grid tests and its numpy restatement (helper module of test_gpu_note_grid.py / test_note_grid_cpu.py; not
collected; numpy only).

Twelve samples of 5 pitch rows and 1100 frames whose lengths sit on the slab boundary (512, 1024), on window boundaries, in the flush and
at nothing at all.  The three heads are run-structured processes turned into logits as in test_gpu_note_sweep.py: inside a run the
sigmoid is uniform over the upper half of (0.02, 0.98), outside over the lower, so every threshold moves cells, short dropouts and short
notes abound (what the cleanup works on), and no sigmoid comes within 1e-3 of a threshold of POOL or of 0.5 -- except the planted ties:
cells at logit 0, whose sigmoid is exactly 0.5 everywhere, and cells at the float32 logit of a POOL threshold, which the device's
expression decides one way or the other, the same way in every kernel.  `cpu_counts` restates the grid with note_clean_ref's literal scan
and scipy's matchings; given `act` it takes the activities from there (the GPU tests pass mt_predict_threshold's, the same expression as
the decoders', so that the planted near-ties cannot make the two sides disagree)."""
import numpy as np

import note_clean_ref as CR
import note_list_ref as LR
import note_metrics_ref as NR
from offset_decode_ref import _length, markov

B, P, T = 12, 5, 1100
LENGTHS = [1100, 1025, 1024, 1023, 513, 512, 511, 65, 64, 63, 1, 0]
POOL = [round(float(v), 3) for v in np.linspace(0.06, 0.94, 16)]
TIES = 60                                 # per head and kind of tie
SEED = 0                                  # 55 of the 64 count rows of GRID_64 are distinct (numpy restatement, roll reference): test_gpu_note_grid.py

CLEANUPS_8 = [(1, 0), (64, 63), (1, 63), (64, 0), (3, 2), (2, 0), (1, 1), (8, 4)]
GRID_64 = dict(tf=[POOL[5], 0.5], to=[0.5, POOL[4]], tk=[0.5, POOL[10]], cleanups=CLEANUPS_8)      # 2 x 2 x 2 x 8


def _head(rng, p_on, p_off, long_row):
    run = markov(rng, (B, P, T), p_on, p_off)
    run[:, 0] = markov(rng, (B, T), *long_row)                               # pitch row 0: long notes, which a long minimum keeps
    u = np.where(run, rng.uniform(0.5, 0.98, size=(B, P, T)), rng.uniform(0.02, 0.5, size=(B, P, T)))
    for t in POOL + [0.5]:
        u = np.where(np.abs(u - t) < 1e-3, t + 2e-3, u)
    x = np.log(u / (1.0 - u)).astype(np.float32)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, size=TIES)] = 0.0
    near = np.float32(np.log(np.asarray(POOL) / (1.0 - np.asarray(POOL))))
    flat[rng.integers(0, flat.size, size=TIES)] = near[rng.integers(0, len(near), size=TIES)]
    return x


def _restruck_list(rng, ref):
    """The runs of the roll as a note list, with re-struck notes 300-900 ticks after some onsets (the list matcher's multi-edge components)."""
    on, off, ptr = LR.notes_from_roll(ref)
    ons, offs, new_ptr = [], [], [0]
    for r in range(len(ptr) - 1):
        a, b = on[ptr[r]:ptr[r + 1]].astype(np.int64), off[ptr[r]:ptr[r + 1]].astype(np.int64)
        again = rng.random(len(a)) < 0.4
        a2 = a[again] + rng.integers(300, 901, size=int(again.sum()))
        b2 = a2 + rng.integers(1, 4000, size=len(a2))
        aa, bb = np.concatenate([a, a2]), np.concatenate([b, b2])
        order = np.argsort(aa, kind="stable")
        ons.append(aa[order])
        offs.append(bb[order])
        new_ptr.append(new_ptr[-1] + len(aa))
    return np.concatenate(ons).astype(np.int32), np.concatenate(offs).astype(np.int32), np.array(new_ptr, np.int64)


class Case:
    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        self.frame = _head(rng, 0.05, 0.12, (0.02, 0.004))
        self.onset = _head(rng, 0.05, 0.5, (0.006, 0.6))
        self.offset = _head(rng, 0.04, 0.5, (0.004, 0.6))
        self.ref = markov(rng, (B, P, T), 0.05, 0.15).astype(np.float32)
        self.notes = _restruck_list(rng, self.ref)
        for a in (self.frame, self.onset, self.offset, self.ref) + self.notes:
            a.setflags(write=False)

    def host_act(self, head, thr):
        """sigmoid(x) > thr in float32, as the decoders write it (the planted near-ties may fall the other way on the device)."""
        x = {"frame": self.frame, "onset": self.onset, "offset": self.offset}[head]
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))) > np.float32(thr)


def cpu_counts(case, kind, decoder, tf, to, tk, cleanups, lengths, act=None):
    """(B, Kf, Ko, Kk, Kc, 4): the grid's contract restated; decoder "frame" / "onset" / "onset_offset" (absent heads: one cell)."""
    act = act or case.host_act
    to = to if decoder != "frame" else [None]
    tk = tk if decoder == "onset_offset" else [None]
    out = np.zeros((B, len(tf), len(to), len(tk), len(cleanups), 4), np.int64)
    none = np.zeros(T, bool)
    for i, a in enumerate(tf):
        f_act = act("frame", a)
        for j, o in enumerate(to):
            o_act = None if o is None else act("onset", o)
            for k, kt in enumerate(tk):
                k_act = None if kt is None else act("offset", kt)
                for b in range(B):
                    L = _length(lengths, b, T)
                    for p in range(P):
                        f = f_act[b, p, :L]
                        decoded = {}
                        for c, (M, G) in enumerate(cleanups):
                            if G not in decoded:                             # bridge and decode once per G, drop per M
                                if o_act is None:
                                    ab = CR.bridge(f, G)
                                    decoded[G] = CR.decode(ab, ab, none[:L])
                                else:
                                    decoded[G] = CR.decode(CR.bridge(f | o_act[b, p, :L], G), o_act[b, p, :L],
                                                           none[:L] if k_act is None else k_act[b, p, :L])
                            est = [(s, e) for s, e in decoded[G] if e - s >= M]
                            if kind == "roll":
                                out[b, i, j, k, c] += NR.row_counts(NR.frame_notes(case.ref[b, p, :L] > 0), est)
                            else:
                                lo, hi = int(case.notes[2][b * P + p]), int(case.notes[2][b * P + p + 1])
                                on, off = LR.clip_notes(case.notes[0][lo:hi], case.notes[1][lo:hi], L)
                                out[b, i, j, k, c] += LR.list_row_counts(on, off, est)
    return out
