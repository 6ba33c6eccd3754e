"""Device time of one 64-pair threshold sweep (mt_note_sweep_counts / mt_note_sweep_list, an 8 x 8 grid, onset-gated decoder) beside the
64 single-pair calls it replaces (mt_note_match_counts / mt_note_match_list), in one process on the same tensors, on the two shapes of
tools/note_metrics_bench.py:

  * chunks:     a batch of 128 chunks x 88 pitches x 938 frames;
  * recordings: a padded batch of 8 whole recordings of 10-25 minutes (T up to ~47 000 frames), masked by `lengths`.

Each variant is warmed up, then timed with device events: --repeats windows of --iters calls each, the two variants alternating;
the median window and the spread (min .. max) are reported, and `speedup` is the ratio of the medians.  Before timing, the sweep's
counts are compared with the 64 calls' pair by pair; the tool stops if they differ.

    python tools/note_sweep_bench.py [--iters 5] [--repeats 7] [--out note_sweep.json]
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

GRID_F = [0.15, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75, 0.85]
GRID_O = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]


def spread_logits(x, gen):
    """note_metrics_bench's logits are +-(0.01 .. 4): rescale every cell's magnitude so that the sigmoids cover (0.02, 0.98) evenly and
    every threshold of the grid moves cells (the sign, i.e. the activity at 0.5, is kept)."""
    import torch
    u = torch.rand(x.shape, device=x.device, generator=gen) * 0.48 + 0.5           # 0.5 .. 0.98
    mag = torch.log(u / (1.0 - u))
    return torch.where(x > 0, mag, -mag).contiguous()


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_case(name, frame, onset, ref, lengths, iters, repeats):
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd._lib import check, lib, ptr
    B, P, T = frame.shape
    out = {"case": name, "B": B, "P": P, "T": T, "valid_frames": B * T if lengths is None else int(sum(lengths)), "pairs": 64}
    notes = roll_notes(ref)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=frame.device)
    gf, go = np.array(GRID_F, np.float32), np.array(GRID_O, np.float32)
    c_sweep = torch.empty(B, 8, 8, 4, dtype=torch.int64, device=frame.device)
    c_one = torch.empty(64, B, 4, dtype=torch.int64, device=frame.device)
    st = _lib.stream_ptr()
    # the entry points themselves (the Python wrappers of the list variant read the ptr table back, a host synchronisation per call)
    calls = {
        "roll": (lambda: check(lib.mt_note_sweep_counts(ptr(frame), ptr(onset), gf.ctypes.data, 8, go.ctypes.data, 8, ptr(ref), ptr(ln), ptr(c_sweep),
                                                        B, P, T, st)),
                 lambda k, a, b: check(lib.mt_note_match_counts(ptr(frame), ptr(onset), a, b, ptr(ref), ptr(ln), ptr(c_one[k]), B, P, T, st))),
        "list": (lambda: check(lib.mt_note_sweep_list(ptr(frame), ptr(onset), gf.ctypes.data, 8, go.ctypes.data, 8, ptr(notes["on"]),
                                                      ptr(notes["off"]), ptr(notes["ptr"]), ptr(ln), ptr(c_sweep), B, P, T, st)),
                 lambda k, a, b: check(lib.mt_note_match_list(ptr(frame), ptr(onset), a, b, ptr(notes["on"]), ptr(notes["off"]), ptr(notes["ptr"]),
                                                              ptr(ln), ptr(c_one[k]), B, P, T, st))),
    }
    pairs = [(8 * i + j, float(gf[i]), float(go[j])) for i in range(8) for j in range(8)]
    for kind, (sweep_call, one_call) in calls.items():
        def sweep():
            sweep_call()
            return c_sweep

        def loop():
            for k, a, b in pairs:
                one_call(k, a, b)
            return c_one
        got = sweep()
        want = loop().permute(1, 0, 2).reshape(B, 8, 8, 4)
        if not torch.equal(got, want):
            raise SystemExit(f"{name} ({kind}): the sweep's counts differ from the single-pair calls'")
        for _ in range(2):
            sweep()
            loop()
        torch.cuda.synchronize()
        t_sweep, t_loop = [], []
        for _ in range(repeats):
            t_sweep.append(timed(sweep, iters))
            t_loop.append(timed(loop, iters))
        ms, ml = float(np.median(t_sweep)), float(np.median(t_loop))
        out[kind] = {"sweep_ms": round(ms, 4), "sweep_min_max": [round(min(t_sweep), 4), round(max(t_sweep), 4)],
                     "single_x64_ms": round(ml, 4), "single_x64_min_max": [round(min(t_loop), 4), round(max(t_loop), 4)],
                     "speedup": round(ml / ms, 2), "distinct_pairs": len({tuple(v) for v in got.sum(0).reshape(64, 4).tolist()})}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import music_transcription_amd  # noqa: F401  (loads libmt_hip.so)
    if not torch.cuda.is_available():
        raise SystemExit("note_sweep_bench measures on the GPU only")
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(5)
    res = []
    frame, onset, ref = make_case(128, 88, 938, None, 1, dev)
    res.append(time_case("chunks 128 x 88 x 938", spread_logits(frame, gen), spread_logits(onset, gen), ref, None, args.iters, args.repeats))
    print(json.dumps(res[-1]), flush=True)
    minutes = np.random.default_rng(2).uniform(10.0, 25.0, size=8)
    minutes[0] = 25.0
    lengths = [int(m * 60 * FS) for m in minutes]
    frame, onset, ref = make_case(8, 88, max(lengths), lengths, 3, dev)
    res.append(time_case("recordings 8 x 10-25 min, padded", spread_logits(frame, gen), spread_logits(onset, gen), ref, lengths, args.iters,
                         args.repeats))
    print(json.dumps(res[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
