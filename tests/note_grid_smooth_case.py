"""A batch on which frame smoothing pays (helper module of test_gpu_note_grid_smooth.py / test_note_grid_smooth_cpu.py; not collected; numpy
only).  In the shape of note_grid_case.py, so that its cpu_counts applies: the reference runs carry strong evidence (+4 logits inside a
run, -4 outside) and the distractors are isolated one-frame blips of +0.5 logit outside the runs.  At threshold 0.5 every blip is a
false note of the frame decoder; at penalties (2, 2) a blip's evidence (32 grid steps) does not pay for switching on and off (256), while a
run of two frames or more does (512 and up) and its edges stay where they are, the frames around it being strong evidence against."""
import numpy as np

import note_grid_case as GC
from offset_decode_ref import markov

BLIP_SMOOTHINGS = [(0.0, 0.0), (2.0, 2.0)]


def blip_case(seed=5):
    rng = np.random.default_rng(seed)
    run = markov(rng, (GC.B, GC.P, GC.T), 0.02, 0.1)
    run[..., 0] = run[..., -1] = False
    run &= np.roll(run, 1, -1) | np.roll(run, -1, -1)                        # no run of a single frame
    near = run | np.roll(run, 1, -1) | np.roll(run, -1, -1) | np.roll(run, 2, -1) | np.roll(run, -2, -1)
    blip = (rng.random(run.shape) < 0.03) & ~near
    blip &= ~np.roll(blip, 1, -1)                                            # isolated: never two in a row
    blip[..., 0] = False
    x = np.where(run, 4.0, np.where(blip, 0.5, -4.0)).astype(np.float32)
    case = GC.Case.__new__(GC.Case)
    case.frame, case.onset, case.offset = x, np.full_like(x, -4.0), np.full_like(x, -4.0)
    case.ref = run.astype(np.float32)
    case.notes = None
    case.blips = int(blip.sum())
    return case


def f1_of(counts):
    """(B, S, 4) counts {n_ref, n_est, tp_onset, tp_onset_offset} -> (S,) mean over samples of the onset F1 (0 for an empty denominator)."""
    c = np.asarray(counts, np.float64)
    den = c[..., 0] + c[..., 1]
    return np.where(den > 0, 2.0 * c[..., 2] / np.maximum(den, 1.0), 0.0).mean(0)
