"""Device time of one 64-cell decoder grid with a frame-smoothing axis -- 2 frame thresholds x 8 smoothing pairs x 2 onset thresholds x 2
cleanups, the onset-gated decoder: one notes.note_grid_counts(smoothings=...) call, i.e. one mt_frame_smooth_paths launch and the
mt_note_grid_counts_paths launches that read its packed paths (DESIGN.md 6c "Smoothing in the decoder grid") -- beside the 64 x
(mt_frame_smooth + mt_note_match_counts_clean) calls it replaces, in one process on the same tensors, on the project's two shapes:

  * chunks:     a batch of 128 chunks x 88 pitches x 938 frames;
  * recordings: a padded batch of 8 recordings x 88 x 56 000 frames, masked by `lengths`.

And the path kernel alone (mt_frame_smooth_paths at K = 1 and K = 16 candidates) beside one mt_frame_smooth launch on the same logits.
Method as tools/frame_smooth_bench.py: every variant is warmed up, then timed with device events, --repeats windows of --iters calls
each, the variants alternating; the median window and the spread (min .. max) are reported.  `grid_over_single` is the ratio of the
medians (above 1: the grid call is slower than the 64 pairs of calls it replaces).  Before timing, the grid's counts are compared with
the 64 pairs of calls cell by cell; the tool stops if they differ.

    python tools/smooth_grid_bench.py [--iters 3] [--repeats 7] [--out smooth_grid_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from note_metrics_bench import make_case  # noqa: E402
from note_sweep_bench import spread_logits, timed  # noqa: E402

GRID_F, GRID_O = [0.35, 0.5], [0.3, 0.5]
SMOOTHINGS = [(0.0, 0.0), (0.5, 0.5), (1.0, 1.0), (2.0, 2.0), (1.0, 0.0), (0.0, 1.0), (2.0, 1.0), (4.0, 4.0)]
CLEANUPS = [(1, 0), (3, 2)]


def _stats(t):
    return round(float(np.median(t)), 4), [round(min(t), 4), round(max(t), 4)]


def time_case(name, frame, onset, ref, lengths, iters, repeats):
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd._lib import check, lib, ptr
    from music_transcription_amd.notes import note_grid_counts
    B, P, T = frame.shape
    W = (T + 63) // 64
    out = {"case": name, "B": B, "P": P, "T": T, "valid_frames": P * (B * T if lengths is None else int(sum(lengths))), "cells": 64}
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=frame.device)
    st = _lib.stream_ptr()
    smoothed = torch.empty_like(frame)
    c_one = torch.empty(64, B, 4, dtype=torch.int64, device=frame.device)
    cells = [(a, s, o, c) for a in GRID_F for s in SMOOTHINGS for o in GRID_O for c in CLEANUPS]

    def grid():
        return note_grid_counts(frame, ref, GRID_F, onset, GRID_O, cleanups=CLEANUPS, lengths=ln, smoothings=SMOOTHINGS)

    def loop():
        for n, (a, (son, soff), o, (m, g)) in enumerate(cells):
            check(lib.mt_frame_smooth(ptr(frame), ptr(smoothed), a, son, soff, ptr(ln), B, P, T, st))
            check(lib.mt_note_match_counts_clean(ptr(smoothed), ptr(onset), None, a, o, 0.5, ptr(ref), ptr(ln), ptr(c_one[n]), B, P, T, m, g, st))
        return c_one
    if not torch.equal(grid().reshape(B, 64, 4), loop().permute(1, 0, 2)):
        raise SystemExit(f"{name}: the grid's counts differ from the single calls'")
    # the path kernel alone, beside the float kernel
    thr16, on16, off16 = (np.ascontiguousarray(v, dtype=np.float32) for v in ([a for a in GRID_F for _ in SMOOTHINGS],
                                                                              [s[0] for s in SMOOTHINGS] * 2, [s[1] for s in SMOOTHINGS] * 2))
    words = torch.empty(2, 16, B, P, W, dtype=torch.int64, device=frame.device)

    def paths(K):
        return lambda: check(lib.mt_frame_smooth_paths(ptr(frame), thr16.ctypes.data, on16.ctypes.data, off16.ctypes.data, K, ptr(ln), B, P, T,
                                                       ptr(words[0]), ptr(words[1]), st))
    variants = {"grid": grid, "single_x64": loop, "paths_K1": paths(1), "paths_K16": paths(16),
                "frame_smooth": lambda: check(lib.mt_frame_smooth(ptr(frame), ptr(smoothed), 0.5, 1.0, 1.0, ptr(ln), B, P, T, st))}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    for k, t in times.items():
        out[k + "_ms"], out[k + "_min_max"] = _stats(t)
    out["grid_over_single"] = round(out["grid_ms"] / out["single_x64_ms"], 3)
    out["speedup"] = round(out["single_x64_ms"] / out["grid_ms"], 2)
    out["paths_K16_over_16_frame_smooth"] = round(out["paths_K16_ms"] / (16 * out["frame_smooth_ms"]), 3)
    out["paths_K1_over_frame_smooth"] = round(out["paths_K1_ms"] / out["frame_smooth_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import music_transcription_amd  # noqa: F401  (loads libmt_hip.so)
    if not torch.cuda.is_available():
        raise SystemExit("smooth_grid_bench measures on the GPU only")
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(5)
    res = []
    frame, onset, ref = make_case(128, 88, 938, None, 1, dev)
    res.append(time_case("chunks 128 x 88 x 938", spread_logits(frame, gen), spread_logits(onset, gen), ref, None, args.iters, args.repeats))
    print(json.dumps(res[-1]), flush=True)
    T = 56000
    lengths = [int(v) for v in np.random.default_rng(2).integers(T // 3, T + 1, size=8)]
    lengths[0] = T
    frame, onset, ref = make_case(8, 88, T, lengths, 3, dev)
    res.append(time_case("recordings 8 x 88 x 56000, padded", spread_logits(frame, gen), spread_logits(onset, gen), ref, lengths, args.iters,
                         args.repeats))
    print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"grid": {"thresholds": GRID_F, "smoothings": SMOOTHINGS, "onset_thresholds": GRID_O, "cleanups": CLEANUPS},
                       "lengths": lengths, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
