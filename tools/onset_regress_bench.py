"""Device time of the sub-frame onset kernels (DESIGN.md 6c "Sub-frame onsets") on synthetic tables:

  * mt_onset_regress_windows beside mt_roll_windows on a batch of 16 windows of 30 s (938 columns) over 16 recordings of 10 minutes
    with --notes_per_pitch note-ons per pitch each;
  * mt_refine_onsets on the note list mt_notes_batch decodes from 8 padded recordings of --minutes minutes.

Every figure is the median of --iters launches, each between its own pair of device events.

    python tools/onset_regress_bench.py [--iters 200] [--out onset_regress_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--notes_per_pitch", type=int, default=120)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import _notes_batch_raw
    if not torch.cuda.is_available():
        raise SystemExit("onset_regress_bench measures on the GPU only")
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()

    def median_us(fn):
        for _ in range(5):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return round(float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3, 2)

    rng = np.random.default_rng(0)
    R, B, T_out, frames = 16, 16, 938, 18750                 # 10 minutes per recording
    on = np.sort(rng.choice(frames * 320, size=(R * 88, args.notes_per_pitch), replace=False), axis=1)
    tick_off = np.arange(R * 88 + 1, dtype=np.int64) * args.notes_per_pitch
    tick_off = np.concatenate([np.append(tick_off[r * 88:r * 88 + 88], tick_off[r * 88 + 88]) for r in range(R)])     # 89 entries per recording
    spans = np.stack([on // 320, on // 320 + 1 + rng.integers(0, 30, on.shape)], -1)
    spans[:, :-1, 1] = np.minimum(spans[:, :-1, 1], spans[:, 1:, 0])
    keep = spans[..., 1] > spans[..., 0]
    span_off = np.concatenate([[0], np.cumsum(keep.sum(1))])
    span_off = np.concatenate([np.append(span_off[r * 88:r * 88 + 88], span_off[r * 88 + 88]) for r in range(R)])
    d_on, d_off = dev(on.reshape(-1), np.int32), dev(tick_off, np.int64)
    d_sp, d_spo = dev(spans[keep], np.int32), dev(span_off, np.int64)
    start = rng.integers(0, (frames - T_out) * 512, B)
    d_rec, d_start, d_keep = dev(np.arange(B) % R, np.int32), dev(start, np.int32), dev(np.full(B, T_out), np.int32)
    d_rate = dev(rng.integers((1 << 32) - (1 << 26), (1 << 32) + (1 << 26), B), np.int64)
    d_cols, d_ncols = dev(np.full(B, -1), np.int64), dev(np.zeros(B), np.int32)
    out = torch.empty(B, 88, T_out, device="cuda")
    res = {"windows": B, "T_out": T_out, "notes_per_pitch": args.notes_per_pitch, "iters": args.iters}
    res["roll_windows_us"] = median_us(lambda: _lib.check(lib.mt_roll_windows(ptr(d_sp), ptr(d_spo), None, ptr(d_rec), ptr(d_cols), ptr(d_ncols),
                                                                               ptr(d_keep), B, T_out, ptr(out), st()), "mt_roll_windows"))
    for name, rate in (("onset_regress_us", None), ("onset_regress_rates_us", d_rate)):
        for J in (2, 8):
            res[f"{name}_J{J}"] = median_us(lambda: _lib.check(lib.mt_onset_regress_windows(ptr(d_on), ptr(d_off), ptr(d_rec), ptr(d_start), ptr(rate),
                                                                                           ptr(d_keep), B, T_out, J, ptr(out), st()),
                                                               "mt_onset_regress_windows"))
    # refinement: 8 padded recordings, onset logits with a triangle every ~0.6 s per pitch
    Bn, T = 8, int(args.minutes * 60 * 16000 / 512)
    lengths = torch.tensor([T - 37 * b for b in range(Bn)], device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    centre = (torch.rand(Bn, 88, T // 19 + 1, device="cuda", generator=g) * 19).cumsum(-1) * 2.0
    t = torch.arange(T, device="cuda", dtype=torch.float32)
    idx = torch.searchsorted(centre, t.expand(Bn, 88, T).contiguous()).clamp(1, centre.shape[-1] - 1)
    d = torch.minimum((centre.gather(-1, idx) - t).abs(), (centre.gather(-1, idx - 1) - t).abs())
    x = torch.logit((1.0 - d / 2.0).clamp(0.0, 1.0), eps=1e-6).contiguous()
    ln = lengths.to(torch.int64)
    row_off_h, _, s, e, _ = _notes_batch_raw(x, x, ln, 0.5, 0.5, (1, 0), None)
    n = int(row_off_h[-1])
    d_s, d_e, d_ro, ticks = dev(s, np.int32), dev(e, np.int32), dev(row_off_h, np.int64), torch.empty(n, dtype=torch.int32, device="cuda")
    res.update(refine_recordings=Bn, refine_frames=T, refine_notes=n)
    for reach in (2, 8):
        res[f"refine_onsets_us_reach{reach}"] = median_us(lambda: _lib.check(lib.mt_refine_onsets(ptr(d_s), ptr(d_e), ptr(d_ro), Bn * 88, n, ptr(x), Bn, 88,
                                                                                                 T, ptr(ln), 0, reach, ptr(ticks), st()), "mt_refine_onsets"))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
