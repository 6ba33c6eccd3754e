"""Device time of the fused optimizer pass with and without the weight average: mt_adam_clip_step_ex against mt_adam_clip_step_ema at
the parameter counts of the two models (n_mels 320, hidden 512, 3 layers), and mt_swap_f32 over the same buffers.

    python tools/optim_bench.py --out optim_bench.json

The two entry points alternate inside one process on the same buffers, each call between two device events; the figure is the median
over --iters rounds after --warmup rounds, with the spread (10th / 90th percentile) beside it.  Bytes come from the algorithm: the norm
pass reads the gradient (4 B per element), the update pass moves p, m, v in and out and reads g (28 B), the average adds 8 B (36 B).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def param_count(mta, model_type):
    import torch
    with torch.no_grad():
        m = mta.TranscriptionModel(model_type=model_type, n_mels=320, hidden_size=512, num_layers=3, device="cuda")
    n = sum(p.numel() for p in m.parameters() if p.requires_grad)
    del m
    torch.cuda.empty_cache()
    return n


def bench(n, iters, warmup):
    import numpy as np
    import torch
    from music_transcription_amd._lib import lib, check, stream_ptr
    g0 = torch.Generator(device="cuda").manual_seed(0)
    p, g, e = (torch.randn(n, device="cuda", generator=g0) for _ in range(3))
    g.mul_(1e-3)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    stats = torch.zeros(2, device="cuda")
    nws = lib.mt_adam_workspace_bytes()
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    st = stream_ptr()
    hy = (1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0)

    def plain(t):
        check(lib.mt_adam_clip_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hy, t, 1.0, None, 0, stats.data_ptr(),
                                       ws.data_ptr(), nws, st), "mt_adam_clip_step_ex")

    def ema(t):
        check(lib.mt_adam_clip_step_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, *hy, t, 1.0, None, 0, 1e-3,
                                        stats.data_ptr(), ws.data_ptr(), nws, st), "mt_adam_clip_step_ema")

    def swap(t):
        check(lib.mt_swap_f32(p.data_ptr(), e.data_ptr(), n, st), "mt_swap_f32")
    calls = {"step_ex": plain, "step_ema": ema, "swap": swap}
    times = {k: [] for k in calls}
    for r in range(warmup + iters):
        for name, fn in calls.items():                 # alternating: whatever else shares the machine weighs on all three alike
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(r + 1)
            b.record()
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    assert float(stats[1]) == 1.0, "the timed steps were skipped"
    bytes_per = {"step_ex": 4 + 28, "step_ema": 4 + 36, "swap": 16}
    out = {"n": n}
    for k, ts in times.items():
        q10, med, q90 = (float(x) for x in np.percentile(ts, [10, 50, 90]))
        out[k] = {"ms_median": round(med, 4), "ms_p10": round(q10, 4), "ms_p90": round(q90, 4),
                  "GB_per_s": round(bytes_per[k] * n / (med * 1e-3) / 1e9, 1)}
    out["ema_over_ex"] = round(out["step_ema"]["ms_median"] / out["step_ex"]["ms_median"], 4)
    out["bytes_ema_over_ex"] = {"both_passes": round(40 / 32, 4), "update_pass": round(36 / 28, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench measures device time: it needs a GPU")
    import music_transcription_amd as mta
    res = {}
    for mt in ("cnn_rnn", "cnn_rnn_large"):
        res[mt] = bench(param_count(mta, mt), args.iters, args.warmup)
        print(json.dumps({mt: res[mt]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
