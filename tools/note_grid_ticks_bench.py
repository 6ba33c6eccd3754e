"""Time of one 64-cell decoder grid in ticks (notes.note_grid_ticks_counts: one mt_notes_grid_ticks launch pair and one
mt_note_match_ticks_cells launch; 2 x 2 x 2 thresholds x 2 cleanups x reaches [0, 1, 2, 8] offset-gated, and 2 x 2 thresholds x 4 cleanups
x the same reaches onset-gated) beside the 64 pairs of calls it replaces (notes.notes_ticks_tables_device + notes.note_match_ticks_device
per cell), in one process on the same tensors, on the two shapes of tools/note_grid_bench.py:

  * chunks:     a batch of 128 chunks x 88 pitches x 938 frames;
  * recordings: a padded batch of 8 whole recordings of 10-25 minutes (T up to ~47 000 frames), masked by `lengths`.

Both paths read results back (the capacity checks, and per recording in the offset-gated loop), so two times are recorded per window:
the device-event time and the wall time that ends in a synchronise.  --repeats windows of --iters calls each, the two paths
alternating; median and range are reported, and `speedup` is the ratio of the wall medians (below 1: the grid is slower than the calls
it replaces).  Nothing is timed before the grid's counts equal the loop's cell by cell; the tool stops if they differ.

    python tools/note_grid_ticks_bench.py [--iters 1] [--repeats 5] [--out profiles/note_grid_ticks_bench.json]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from note_metrics_bench import FS, make_case, roll_notes  # noqa: E402
from note_sweep_bench import spread_logits  # noqa: E402

GRID_F, GRID_O, GRID_K = [0.35, 0.5], [0.3, 0.5], [0.5, 0.65]
CLEANUPS, REACHES = [(1, 0), (3, 2)], [0, 1, 2, 8]
CLEANUPS_ONSET = [(1, 0), (3, 2), (2, 0), (2, 1)]           # the onset-gated grid has no offset axis: 4 cleanups keep it at 64 cells
REFINE_REACH = 2


def timed(fn, iters):
    """-> (device-event ms, wall ms ending in a synchronise) per call."""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters


def time_case(name, frame, onset, offset, ref, lengths, iters, repeats):
    import torch
    from music_transcription_amd.notes import note_grid_ticks_counts, note_match_ticks_device, notes_ticks_tables_device
    B, P, T = frame.shape
    out = {"case": name, "B": B, "P": P, "T": T, "valid_frames": B * T if lengths is None else int(sum(lengths)), "cells": 64,
           "refine_reach": REFINE_REACH}
    notes = roll_notes(ref)
    for kind, off, tk, cleanups in (("offset_gated", offset, GRID_K, CLEANUPS), ("onset_gated", None, [0.5], CLEANUPS_ONSET)):
        cells = list(itertools.product(GRID_F, GRID_O, tk, cleanups, REACHES))
        assert len(cells) == 64

        def grid():
            return note_grid_ticks_counts(frame, onset, notes, GRID_F, GRID_O, off, tk if off is not None else None, cleanups, REACHES, lengths,
                                          REFINE_REACH)

        def loop():
            res = []
            for a, b, k, (m, g), r in cells:
                est = notes_ticks_tables_device(frame, onset, a, b, lengths, offset_logits=off, offset_threshold=k, min_note_frames=m,
                                                bridge_frames=g, refine_reach=REFINE_REACH, onset_detect="peak" if r else "edge",
                                                peak_reach=r or 1)
                res.append(note_match_ticks_device(est, notes))
            return torch.stack(res, 1)
        got, want = grid().reshape(B, 64, 4), loop()
        if not torch.equal(got, want):
            raise SystemExit(f"{name} ({kind}): the grid's counts differ from the single-configuration calls'")
        grid()
        t_grid, t_loop = [], []
        for _ in range(repeats):
            t_grid.append(timed(grid, iters))
            t_loop.append(timed(loop, iters))
        res = {"distinct_cells": len({tuple(v) for v in got.sum(0).tolist()}), "estimated_notes_all_cells": int(got[..., 1].sum())}
        for i, what in enumerate(("device", "wall")):
            g, l = [t[i] for t in t_grid], [t[i] for t in t_loop]
            res[what] = {"grid_ms": round(float(np.median(g)), 3), "grid_min_max": [round(min(g), 3), round(max(g), 3)],
                         "loop_x64_ms": round(float(np.median(l)), 3), "loop_x64_min_max": [round(min(l), 3), round(max(l), 3)],
                         "speedup": round(float(np.median(l) / np.median(g)), 2)}
        res["grid_faster_by_wall"] = bool(res["wall"]["grid_ms"] < res["wall"]["loop_x64_ms"])
        out[kind] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import music_transcription_amd  # noqa: F401  (loads libmt_hip.so)
    if not torch.cuda.is_available():
        raise SystemExit("note_grid_ticks_bench measures on the GPU only")
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(5)
    res = []
    frame, onset, ref = make_case(128, 88, 938, None, 1, dev)
    _, offset, _ = make_case(128, 88, 938, None, 11, dev)
    res.append(time_case("chunks 128 x 88 x 938", spread_logits(frame, gen), spread_logits(onset, gen), spread_logits(offset, gen), ref, None,
                         args.iters, args.repeats))
    print(json.dumps(res[-1]), flush=True)
    minutes = np.random.default_rng(2).uniform(10.0, 25.0, size=8)
    minutes[0] = 25.0
    lengths = [int(m * 60 * FS) for m in minutes]
    frame, onset, ref = make_case(8, 88, max(lengths), lengths, 3, dev)
    _, offset, _ = make_case(8, 88, max(lengths), lengths, 13, dev)
    res.append(time_case("recordings 8 x 10-25 min, padded", spread_logits(frame, gen), spread_logits(onset, gen), spread_logits(offset, gen), ref,
                         lengths, args.iters, args.repeats))
    print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
