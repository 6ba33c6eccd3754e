"""The case of the tick-grid tests and the host composition it is held against (helper module of test_note_grid_ticks_cpu.py /
test_gpu_note_grid_ticks.py; not collected; numpy only).

B = 3 recordings x 88 pitches x T = 1100 frames (three 512-frame slabs, the last partial) with lengths [1100, 600, 0]; the padding past a
length holds NaN, which nothing may read.  Every second pitch row carries planted notes: strikes in clusters 2 to 3 frames apart whose
onset head is the triangular target of onset_regress_ref.regress_target (width 3 frames) scaled by a per-row amplitude and per-frame
noise, a frame head that hovers around the thresholds while a note sounds and an offset head that fires, sometimes, where it ends.
Two rows are built by hand:
  * TRIPLE (b, p): three peaks two frames apart whose neighbours push the first half a frame late and the last half a frame early, so the
    three refined onsets lie within 960 ticks -- more estimates inside one reference window than the streaming matcher allows;
  * CHAIN (b, p): 80 strikes two frames apart with symmetric peaks (refined onsets on the grid, 640 ticks apart) and reference onsets
    150 to 400 ticks late, so each reference note shares an estimate with the next: one connected component of 80 reference notes.
The reference note list is the planted notes with onsets and offsets jittered by up to +-400 ticks (40 ms), a tenth of them dropped
and as many strays added.

`host_tables(case, cell, refine_reach)` composes the host references: the decoder of note_grid_peak_case (starts / fast_notes), then
onset_regress_ref.refine_one, in the layout of MaestroDataset.ref_notes, for notes.note_match_ticks to score."""
import itertools

import numpy as np

import note_metrics_ref as NR
import onset_regress_ref as OG
from note_grid_peak_case import fast_notes, starts

B, P, T = 3, 88, 1100
LENGTHS = [1100, 600, 0]
SEED = 11
TRIPLE, CHAIN = (0, 5), (0, 7)
TRIPLE_AT, CHAIN_AT, CHAIN_N = 300, 100, 80

# the main grid: 2 x 2 x 2 x 2 x 2 = 32 cells (offset-gated), 16 without the offset axis
GRID = dict(tf=[0.4, 0.6], to=[0.35, 0.65], tk=[0.4, 0.6], cleanups=[(1, 0), (3, 1)], reaches=[0, 1])
# past 64 cells: 3 x 3 x 2 x 2 x 3 = 108, with a repeated and an unsorted axis
GRID_108 = dict(tf=[0.6, 0.4, 0.5], to=[0.5, 0.35, 0.5], tk=[0.6, 0.4], cleanups=[(2, 0), (1, 2)], reaches=[2, 0, 8])


def _logit(q):
    q = np.clip(np.asarray(q, np.float64), 1e-9, 1 - 1e-9)
    return (np.log(q) - np.log1p(-q)).astype(np.float32)


class Case:
    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        frame = rng.normal(-2.5, 1.0, (B, P, T)).astype(np.float32)
        onset = rng.normal(-3.0, 0.7, (B, P, T)).astype(np.float32)
        offset = rng.normal(-3.0, 0.8, (B, P, T)).astype(np.float32)
        truth = {}                                                   # (b, p) -> [(on_tick, off_tick)]
        for b, p in itertools.product(range(B), range(P)):
            L = LENGTHS[b]
            if (b, p) in (TRIPLE, CHAIN) or p % 2 or L < 64:
                continue
            notes, t = [], int(rng.integers(2, 40))
            while t < L - 30:
                on = 320 * t + int(rng.integers(-150, 151))
                for _ in range(int(rng.integers(1, 4))):             # a cluster of strikes 2 to 3 frames apart (640 .. 960 ticks)
                    notes.append(on)
                    on += int(rng.integers(640, 961))
                t = on // 320 + int(rng.integers(4, 70))
            ons = np.array(sorted(set(n for n in notes if 0 <= n < 320 * (L - 4))), np.int32)
            if not len(ons):
                continue
            tick_off = np.zeros(89, np.int64)
            tick_off[1:] = len(ons)
            y = OG.regress_target(ons, tick_off, [0], [0], [L], L, 3)[0, 0].astype(np.float64)
            amp = rng.uniform(0.45, 0.97) * (1.0 - 0.2 * rng.random(L))
            hit = y > 0
            onset[b, p, :L][hit] = _logit(y * amp)[hit]
            offs = []
            for i, on in enumerate(ons):
                s = (int(on) + 160) // 320
                nxt = (int(ons[i + 1]) + 160) // 320 if i + 1 < len(ons) else L
                e = min(L, s + int(rng.integers(2, 45)))
                frame[b, p, s:min(e, nxt + 2)] = rng.normal(0.5, 1.0, min(e, nxt + 2) - s)
                if rng.random() < 0.7 and e < L:
                    offset[b, p, e - 1:e + int(rng.integers(0, 2))] = rng.normal(0.3, 1.2)
                offs.append(320 * e)
            truth[b, p] = list(zip(ons.tolist(), offs))
        # TRIPLE: peaks at t, t + 2, t + 4; q[t] = q[t + 1] (shift +0.5), q[t + 3] one float below q[t + 4] (shift -0.5), the middle one highest
        b, p = TRIPLE
        t = TRIPLE_AT
        frame[b, p, t - 1:t + 12] = 3.0
        hi, top = np.float32(2.0), np.float32(3.0)
        onset[b, p, t - 3:t + 9] = -6.0
        onset[b, p, [t, t + 1, t + 4]] = hi
        onset[b, p, t + 2] = top
        onset[b, p, t + 3] = np.nextafter(hi, np.float32(0.0))
        truth[b, p] = [(320 * t + 160, 320 * (t + 2)), (320 * (t + 2), 320 * (t + 4)), (320 * (t + 4) - 160, 320 * (t + 12))]
        # CHAIN: symmetric peaks on even frames
        b, p = CHAIN
        t = CHAIN_AT
        frame[b, p, t:t + 2 * CHAIN_N] = 3.0
        onset[b, p, t - 2:t + 2 * CHAIN_N + 2] = -1.5
        onset[b, p, t:t + 2 * CHAIN_N:2] = 2.5
        truth[b, p] = [(320 * (t + 2 * i), 320 * (t + 2 * i + 2)) for i in range(CHAIN_N)]
        for b in range(B):                                           # the padding: never read
            for x in (frame, onset, offset):
                x[b, :, LENGTHS[b]:] = np.nan
        # the reference: jittered truth, a tenth dropped, as many strays
        r_on, r_off, r_ptr = [], [], [0]
        for b, p in itertools.product(range(B), range(P)):
            row = []
            for on, off in truth.get((b, p), []):
                if (b, p) in (CHAIN, TRIPLE):                        # CHAIN: late enough to link; TRIPLE: the middle note sees all three
                    a = on + (int(rng.integers(150, 401)) if (b, p) == CHAIN else int(rng.integers(-20, 21)))
                    row.append((a, max(a + 1, off + int(rng.integers(-400, 401)))))
                    continue
                if rng.random() < 0.1:
                    s = int(rng.integers(0, 320 * max(LENGTHS[b], 1)))
                    row.append((s, s + int(rng.integers(300, 6000))))
                    continue
                a = max(0, on + int(rng.integers(-400, 401)))
                row.append((a, max(a + 1, off + int(rng.integers(-400, 401)))))
            if b == 2 and p % 11 == 0:                               # a recording without frames still has reference notes
                row.append((1000 + p, 5000))
            row.sort()
            r_on += [a for a, _ in row]
            r_off += [z for _, z in row]
            r_ptr.append(len(r_on))
        self.frame, self.onset, self.offset, self.truth = frame, onset, offset, truth
        self.ref = {"on": np.array(r_on, np.int32), "off": np.array(r_off, np.int32), "ptr": np.array(r_ptr, np.int64)}
        for x in (frame, onset, offset, *self.ref.values()):
            x.setflags(write=False)
        self._q, self._ticks = {}, {}

    def row_notes(self, b, p, cell, offset_gated=True):
        """[(s, e)] of row (b, p) at cell = (thr_f, thr_o, thr_k, (M, G), reach)."""
        tf, to, tk, (M, G), R = cell
        L = LENGTHS[b]
        if L == 0:
            return []
        f, o = NR.sigmoid_active(self.frame[b, p, :L], tf), NR.sigmoid_active(self.onset[b, p, :L], to)
        k = NR.sigmoid_active(self.offset[b, p, :L], tk) if offset_gated else None
        return fast_notes(f, o, starts(self.onset[b, p, :L], o, R), k, M, G)

    def tick(self, b, p, s, e, reach):
        key = (b, p, s, e, reach)
        if key not in self._ticks:
            if (b, p) not in self._q:
                self._q[b, p] = OG.sigmoid64(self.onset[b, p, :LENGTHS[b]])
            self._ticks[key] = OG.refine_one(self._q[b, p], s, e, reach)[0]
        return self._ticks[key]

    def host_tables(self, cell, refine_reach=2, offset_gated=True, refined=True):
        """The cell's note list {"on", "off", "ptr"}; refined=False: the 320 s stamps."""
        on, off, ptr = [], [], [0]
        for b, p in itertools.product(range(B), range(P)):
            for s, e in self.row_notes(b, p, cell, offset_gated):
                on.append(self.tick(b, p, s, e, refine_reach) if refined else 320 * s)
                off.append(320 * e)
            ptr.append(len(on))
        return {"on": np.array(on, np.int32), "off": np.array(off, np.int32), "ptr": np.array(ptr, np.int64)}


def cells(grid, offset_gated=True):
    """The cells of a grid in the kernel's order (frame-major, the reach innermost) -> [(index tuple, cell)]."""
    tk = grid["tk"] if offset_gated else [0.5]
    axes = (grid["tf"], grid["to"], tk, grid["cleanups"], grid["reaches"])
    return [(idx, tuple(a[i] for a, i in zip(axes, idx))) for idx in itertools.product(*(range(len(a)) for a in axes))]
