"""Device time of one 64-configuration decoder grid (mt_note_grid_counts / mt_note_grid_list: 2 x 2 x 2 thresholds x 8 cleanups, the
offset-gated decoder) beside the 64 single-configuration calls it replaces (mt_note_match_counts_clean / mt_note_match_list_clean), in
one process on the same tensors, on the two shapes and by the protocol of tools/note_sweep_bench.py:

  * chunks:     a batch of 128 chunks x 88 pitches x 938 frames;
  * recordings: a padded batch of 8 whole recordings of 10-25 minutes (T up to ~47 000 frames), masked by `lengths`.

Each variant is warmed up, then timed with device events: --repeats windows of --iters calls each, the two variants alternating;
the median window and the spread (min .. max) are reported, and `speedup` is the ratio of the medians (below 1: the grid is slower
than the calls it replaces).  Before timing, the grid's counts are compared with the 64 calls' cell by cell; the tool stops if they differ.

--peak times the peak grid instead (DESIGN.md 6c "Peak picking in the decoder grid"): one 64-cell mt_note_grid_counts_peak /
mt_note_grid_list_peak launch, 2 x 2 x 2 thresholds x 2 cleanups x reaches [0, 1, 2, 8], beside the 64 calls it replaces
(mt_note_match_*_peak, at reach 0 mt_note_match_*_clean), compared first in the same way.

    python tools/note_grid_bench.py [--peak] [--iters 3] [--repeats 7] [--out note_grid.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from note_metrics_bench import FS, make_case, roll_notes  # noqa: E402
from note_sweep_bench import spread_logits, timed  # noqa: E402

GRID_F, GRID_O, GRID_K = [0.35, 0.5], [0.3, 0.5], [0.5, 0.65]
CLEANUPS = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (3, 2), (4, 2), (6, 3)]        # (min_frames, bridge_frames): up to 192 ms / 96 ms
PEAK_CLEANUPS, PEAK_REACHES = [(1, 0), (3, 2)], [0, 1, 2, 8]                        # --peak: 2 cleanups x 4 reaches in place of 8 cleanups


def time_case(name, frame, onset, offset, ref, lengths, iters, repeats, peak=False):
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd._lib import check, lib, ptr
    B, P, T = frame.shape
    out = {"case": name, "B": B, "P": P, "T": T, "valid_frames": B * T if lengths is None else int(sum(lengths)), "configurations": 64}
    notes = roll_notes(ref)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=frame.device)
    gf, go, gk = (np.array(g, np.float32) for g in (GRID_F, GRID_O, GRID_K))
    cleanups = PEAK_CLEANUPS if peak else CLEANUPS
    cl = np.array(cleanups, np.int32)
    reaches = np.array(PEAK_REACHES if peak else [0], np.int32)
    c_grid = torch.empty(B, 2, 2, 2, len(cl) * len(reaches), 4, dtype=torch.int64, device=frame.device)
    c_one = torch.empty(64, B, 4, dtype=torch.int64, device=frame.device)
    st = _lib.stream_ptr()
    axes = (ptr(frame), ptr(onset), ptr(offset), gf.ctypes.data, 2, go.ctypes.data, 2, gk.ctypes.data, 2, cl.ctypes.data, len(cl))
    if peak:
        axes += (reaches.ctypes.data, len(reaches))
    grid_counts, grid_list = (lib.mt_note_grid_counts_peak, lib.mt_note_grid_list_peak) if peak else (lib.mt_note_grid_counts, lib.mt_note_grid_list)

    def one_counts(n, a, b, k, m, g, r):                    # a reach of 0: the edge rule, the _clean entry point
        head = (ptr(frame), ptr(onset), ptr(offset), a, b, k, ptr(ref), ptr(ln), ptr(c_one[n]), B, P, T, m, g)
        check(lib.mt_note_match_counts_peak(*head, r, st) if r else lib.mt_note_match_counts_clean(*head, st))

    def one_list(n, a, b, k, m, g, r):
        head = (ptr(frame), ptr(onset), ptr(offset), a, b, k, ptr(notes["on"]), ptr(notes["off"]), ptr(notes["ptr"]), ptr(ln), ptr(c_one[n]),
                B, P, T, m, g)
        check(lib.mt_note_match_list_peak(*head, r, st) if r else lib.mt_note_match_list_clean(*head, st))
    calls = {
        "roll": (lambda: check(grid_counts(*axes, ptr(ref), ptr(ln), ptr(c_grid), B, P, T, st)), one_counts),
        "list": (lambda: check(grid_list(*axes, ptr(notes["on"]), ptr(notes["off"]), ptr(notes["ptr"]), ptr(ln), ptr(c_grid), B, P, T, st)),
                 one_list),
    }
    cells = [(float(a), float(b), float(k), int(m), int(g), int(r)) for a in gf for b in go for k in gk for m, g in cleanups for r in reaches]
    if peak:
        out["grid"] = "peak: 2 x 2 x 2 thresholds x 2 cleanups x reaches " + str(PEAK_REACHES)
    for kind, (grid_call, one_call) in calls.items():
        def grid():
            grid_call()
            return c_grid

        def loop():
            for n, cell in enumerate(cells):
                one_call(n, *cell)
            return c_one
        got = grid().reshape(B, 64, 4)
        want = loop().permute(1, 0, 2)
        if not torch.equal(got, want):
            raise SystemExit(f"{name} ({kind}): the grid's counts differ from the single-configuration calls'")
        for _ in range(2):
            grid()
            loop()
        torch.cuda.synchronize()
        t_grid, t_loop = [], []
        for _ in range(repeats):
            t_grid.append(timed(grid, iters))
            t_loop.append(timed(loop, iters))
        mg, ml = float(np.median(t_grid)), float(np.median(t_loop))
        out[kind] = {"grid_ms": round(mg, 4), "grid_min_max": [round(min(t_grid), 4), round(max(t_grid), 4)],
                     "single_x64_ms": round(ml, 4), "single_x64_min_max": [round(min(t_loop), 4), round(max(t_loop), 4)],
                     "grid_over_single": round(mg / ml, 3), "speedup": round(ml / mg, 2),
                     "distinct_cells": len({tuple(v) for v in got.sum(0).tolist()})}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--peak", action="store_true", help="time the peak grid (mt_note_grid_*_peak) and the 64 _peak / _clean calls it replaces")
    args = ap.parse_args()
    import torch
    import music_transcription_amd  # noqa: F401  (loads libmt_hip.so)
    if not torch.cuda.is_available():
        raise SystemExit("note_grid_bench measures on the GPU only")
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(5)
    res = []
    frame, onset, ref = make_case(128, 88, 938, None, 1, dev)
    _, offset, _ = make_case(128, 88, 938, None, 11, dev)
    res.append(time_case("chunks 128 x 88 x 938", spread_logits(frame, gen), spread_logits(onset, gen), spread_logits(offset, gen), ref, None,
                         args.iters, args.repeats, args.peak))
    print(json.dumps(res[-1]), flush=True)
    minutes = np.random.default_rng(2).uniform(10.0, 25.0, size=8)
    minutes[0] = 25.0
    lengths = [int(m * 60 * FS) for m in minutes]
    frame, onset, ref = make_case(8, 88, max(lengths), lengths, 3, dev)
    _, offset, _ = make_case(8, 88, max(lengths), lengths, 13, dev)
    res.append(time_case("recordings 8 x 10-25 min, padded", spread_logits(frame, gen), spread_logits(onset, gen), spread_logits(offset, gen), ref,
                         lengths, args.iters, args.repeats, args.peak))
    print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
