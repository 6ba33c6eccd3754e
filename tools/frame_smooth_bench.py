"""Device time of the frame smoothing (mt_frame_smooth / mt_frame_smooth_chunks, DESIGN.md 6c "Frame smoothing") beside a plain copy of the
same bytes (torch.clone of the logits, same process, same tensors), by the protocol of tools/note_sweep_bench.py, on

  * chunks:     128 chunks x 88 pitches x 938 frames, as one recording per pitch (mt_frame_smooth_chunks: 88 rows of 120 064 frames)
                and as 128 x 88 independent rows (mt_frame_smooth: 11 264 rows of 938 frames);
  * recordings: a padded batch of 8 recordings x 88 x 56 000 frames, masked by `lengths` (mt_frame_smooth: 704 rows), and the same
                buffer read as 39 424 rows of 1 000 frames: the same kernel with rows to spare, which tells the serial walk along a row
                from the work per frame.

Each variant is warmed up, then timed with device events: --repeats windows of --iters calls each, the variants alternating; the
median window and the spread (min .. max) are reported.  Effective GB/s counts 4 B read + 4 B written per valid frame (the kernel
reads its own provisional output once more on top of that); `of_copy` is the copy's time over the kernel's on the same bytes.

--split OUT.json times, in the same process and alternating in the same way, the one-wave kernel (the plain entry points with
MT_SMOOTH_SPLIT=0) against mt_frame_smooth_split / mt_frame_smooth_chunks_split at 2, 4, 8 and 16 waves per row (DESIGN.md 6c "Long
rows: segments per wave") on the first three shapes above and on a short recording of 14 chunks x 88 x 938; the outputs are compared
for equality before anything is timed.  OUT.json is what the dispatch rule of csrc/smooth.hip is read from.

    python tools/frame_smooth_bench.py [--on 1.0] [--off 1.0] [--iters 5] [--repeats 7] [--out frame_smooth.json] [--split split.json]
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


def time_variants(name, x, variants, frames, iters, repeats):
    """variants: {label: call}; every call writes the smoothed logits of `frames` valid frames.  -> one result row per label."""
    import torch
    out = torch.empty_like(x)
    calls = dict(variants)
    calls["copy"] = lambda o: torch.clone(x)
    for fn in calls.values():
        for _ in range(2):
            fn(out)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            times[k].append(timed(lambda: fn(out), iters))
    med = {k: float(np.median(v)) for k, v in times.items()}
    rows = []
    for k in variants:
        rows.append({"case": name, "variant": k, "valid_frames": frames, "ms": round(med[k], 4),
                     "min_max": [round(min(times[k]), 4), round(max(times[k]), 4)], "effective_GBps": round(8.0 * frames / med[k] / 1e6, 1),
                     "copy_ms": round(med["copy"], 4), "copy_GBps": round(8.0 * x.numel() / med["copy"] / 1e6, 1),
                     "of_copy": round(med["copy"] / med[k] * frames / x.numel(), 3)})
    return rows


SPLIT_WAVES = (2, 4, 8, 16)


def split_cases(args, dev, gen):
    """One wave per row against SPLIT_WAVES on four shapes -> result rows (case, rows, windows per row, waves, ms, min_max)."""
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd._lib import check, lib, ptr
    st = _lib.stream_ptr()
    pen = (args.threshold, args.on, args.off)
    T = 56000
    lengths = [int(v) for v in np.random.default_rng(2).integers(T // 3, T + 1, size=8)]
    lengths[0] = T
    ln = torch.tensor(lengths, dtype=torch.int64, device=dev)

    def chunks(x, NB, waves):
        if waves == 1:
            return lambda o: check(lib.mt_frame_smooth_chunks(ptr(x), ptr(o), *pen, NB, 88, 938, st))
        return lambda o: check(lib.mt_frame_smooth_chunks_split(ptr(x), ptr(o), *pen, NB, 88, 938, waves, st))

    def batch(x, ln, B, T, waves):
        if waves == 1:
            return lambda o: check(lib.mt_frame_smooth(ptr(x), ptr(o), *pen, ptr(ln), B, 88, T, st))
        return lambda o: check(lib.mt_frame_smooth_split(ptr(x), ptr(o), *pen, ptr(ln), B, 88, T, waves, st))
    x = spread_logits(make_case(128, 88, 938, None, 1, dev)[0], gen)
    y = spread_logits(make_case(8, 88, T, lengths, 3, dev)[0], gen)
    z = x[:14].contiguous()
    shapes = [("chunks 128 x 88 x 938", x, 88, -(-128 * 938 // 64), x.numel(), lambda w: chunks(x, 128, w)),
              ("rows 11264 x 938", x, 128 * 88, -(-938 // 64), x.numel(), lambda w: batch(x, None, 128, 938, w)),
              ("recordings 8 x 88 x 56000, padded", y, 8 * 88, -(-T // 64), 88 * sum(lengths), lambda w: batch(y, ln, 8, T, w)),
              ("chunks 14 x 88 x 938", z, 88, -(-14 * 938 // 64), z.numel(), lambda w: chunks(z, 14, w))]
    res = []
    for name, t, rows, windows, frames, make in shapes:
        want = torch.zeros_like(t)
        make(1)(want)
        for w in SPLIT_WAVES:                    # the same bits, before anything is timed
            got = torch.zeros_like(t)
            make(w)(got)
            torch.cuda.synchronize()
            if not torch.equal(got, want):
                raise SystemExit(f"{name}: {w} waves per row differ from one")
        variants = {"1": make(1)}
        variants.update({str(w): make(w) for w in SPLIT_WAVES})
        for r in time_variants(name, t, variants, frames, args.iters, args.repeats):
            res.append({"case": name, "rows": rows, "windows_per_row": windows, "waves": int(r["variant"]), "ms": r["ms"], "min_max": r["min_max"],
                        "effective_GBps": r["effective_GBps"], "copy_ms": r["copy_ms"]})
    for name in dict.fromkeys(r["case"] for r in res):      # a wave count qualifies where its whole range lies below the one-wave range
        one = next(r for r in res if r["case"] == name and r["waves"] == 1)
        for r in res:
            if r["case"] == name:
                r["below_one_wave"] = r["waves"] > 1 and r["min_max"][1] < one["min_max"][0]
    return {"on_penalty": args.on, "off_penalty": args.off, "threshold": args.threshold, "lengths": lengths, "iters": args.iters,
            "repeats": args.repeats, "results": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--on", type=float, default=1.0)
    ap.add_argument("--off", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--split", default=None, metavar="OUT.json", help="time one wave per row against 2, 4, 8 and 16 instead, and write OUT.json")
    args = ap.parse_args()
    if args.split:
        os.environ["MT_SMOOTH_SPLIT"] = "0"      # the plain entry points are the one-wave kernel here
    import torch
    import music_transcription_amd  # noqa: F401  (loads libmt_hip.so)
    from music_transcription_amd import _lib
    from music_transcription_amd._lib import check, lib, ptr
    if not torch.cuda.is_available():
        raise SystemExit("frame_smooth_bench measures on the GPU only")
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(5)
    if args.split:
        out = split_cases(args, dev, gen)
        for r in out["results"]:
            print(json.dumps(r), flush=True)
        with open(args.split, "w") as f:
            json.dump(out, f, indent=1)
        return
    st = _lib.stream_ptr()
    pen = (args.threshold, args.on, args.off)

    def batch(x, ln, B, P, T):
        return lambda o: check(lib.mt_frame_smooth(ptr(x), ptr(o), *pen, ptr(ln), B, P, T, st))
    res = []
    x = spread_logits(make_case(128, 88, 938, None, 1, dev)[0], gen)
    res += time_variants("chunks 128 x 88 x 938", x, {
        "chunks (88 rows x 120064)": lambda o: check(lib.mt_frame_smooth_chunks(ptr(x), ptr(o), *pen, 128, 88, 938, st)),
        "rows (11264 rows x 938)": batch(x, None, 128, 88, 938)}, x.numel(), args.iters, args.repeats)
    T = 56000
    lengths = [int(v) for v in np.random.default_rng(2).integers(T // 3, T + 1, size=8)]
    lengths[0] = T
    y = spread_logits(make_case(8, 88, T, lengths, 3, dev)[0], gen)
    ln = torch.tensor(lengths, dtype=torch.int64, device=dev)
    res += time_variants("recordings 8 x 88 x 56000, padded", y, {"recordings (704 rows, lengths)": batch(y, ln, 8, 88, T)}, 88 * sum(lengths),
                         args.iters, args.repeats)
    res += time_variants("recordings 8 x 88 x 56000, all frames", y, {
        "recordings (704 rows x 56000)": batch(y, None, 8, 88, T),
        "same bytes as 39424 rows x 1000": batch(y, None, 8 * 56, 88, 1000)}, y.numel(), args.iters, args.repeats)
    for r in res:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"on_penalty": args.on, "off_penalty": args.off, "threshold": args.threshold, "lengths": lengths, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
