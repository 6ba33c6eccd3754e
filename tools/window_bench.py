"""Cost of overlapping windows (DESIGN.md "Whole recordings in overlapping windows") on 20 minutes of synthetic audio with
cnn_rnn_large (320 mels, hidden 512, 3 layers, seeded random weights):

  * the window count at --overlap against the chunk count of the reference's concatenation;
  * end-to-end device-resident time, waveform -> notes, of transcribe_windows_to_notes against transcribe_chunks_to_notes
    (best of --iters after a warm-up, wall clock around a synchronised call);
  * mt_stitch_windows alone on the windows' logits (device events over --iters launches).

    python tools/window_bench.py [--overlap 2] [--iters 5] [--out window_bench.json]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/window_bench.py --profile     (one windowed pass, for the kernel stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, HOP = 16000, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--overlap", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="one warm-up and one windowed pass only (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import music_transcription_amd as mta
    from music_transcription_amd import _lib, transcribe as TR
    from music_transcription_amd.windows import plan_windows
    if not torch.cuda.is_available():
        raise SystemExit("window_bench measures on the GPU only")
    torch.manual_seed(0)
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=320, hidden_size=512, num_layers=3, dropout=0.2, device="cuda").eval()
    n = int(args.minutes * 60 * SR)
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / SR
    y = (0.05 * torch.randn(n, device="cuda", generator=g) + 0.2 * torch.sin(2 * np.pi * 440.0 * t) * torch.exp(-0.7 * (t % 1.3))).contiguous()
    plan = plan_windows(n, args.overlap)
    chunks, _ = TR.split_into_chunks_device(y)
    res = {"minutes": args.minutes, "overlap_s": args.overlap, "overlap_frames": plan.O, "windows": len(plan.start), "chunks": len(chunks),
           "window_overhead": round(len(plan.start) / len(chunks) - 1.0, 4)}
    windowed = lambda: TR.transcribe_windows_to_notes(model, y, args.overlap, 0.5, n_mels=320)
    chunked = lambda: TR.transcribe_chunks_to_notes(model, chunks, 0.5, n_mels=320)
    windowed()
    chunked()
    torch.cuda.synchronize()
    if args.profile:
        windowed()
        torch.cuda.synchronize()
        print(json.dumps(res))
        return
    for name, fn in (("chunks_ms", chunked), ("windows_ms", windowed)):
        best = float("inf")
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            notes = fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        res[name] = round(best, 2)
        res[name.replace("_ms", "_notes")] = len(notes)
    res["windows_over_chunks"] = round(res["windows_ms"] / res["chunks_ms"], 3)
    # the stitch alone: the windows' logits into one (1, 88, Tg) roll
    Bw = len(plan.start)
    src = torch.randn(Bw, 88, plan.Tw, device="cuda")
    dst = torch.zeros(1, 88, plan.Tg, device="cuda")
    d32 = torch.tensor(np.stack([np.zeros(Bw), plan.lo, plan.hi]).astype(np.int32), device="cuda")
    d64 = torch.from_numpy(plan.start.copy()).cuda()
    stitch = lambda: _lib.check(_lib.lib.mt_stitch_windows(_lib.ptr(src), Bw, 88, plan.Tw, _lib.ptr(d32[0]), _lib.ptr(d64), _lib.ptr(d32[1]),
                                                           _lib.ptr(d32[2]), _lib.ptr(dst), 1, plan.Tg, _lib.stream_ptr()), "mt_stitch_windows")
    for _ in range(3):
        stitch()
    iters = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        stitch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    nbytes = 2 * 88 * 4 * plan.Tg                              # kept frames read once and written once
    res["stitch_ms_events"] = round(ms, 4)
    res["stitch_GB_per_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
