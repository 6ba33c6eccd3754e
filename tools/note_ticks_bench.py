"""Device time of the tick matcher mt_note_match_ticks (DESIGN.md 6c "Sub-frame onsets", Scoring) beside the host path it replaces.

The shape of tools/onset_regress_bench.py: 8 padded recordings of --minutes minutes (9 375 frames at 5), onset logits with a triangle
every ~0.6 s per pitch; the estimated note list is what mt_notes_batch and mt_refine_onsets make of them, the reference list the same
notes with +-40 ms of jitter on onsets and offsets, 10 % of them dropped and as many strays added.

  * the counts of the device matcher are compared with notes.note_match_ticks before anything is timed;
  * mt_note_match_ticks: device events around windows of --launches launches, the median and range of --iters windows, per launch;
  * the device path as evaluation runs it, wall time: notes.note_match_ticks_device (table checks, workspace, launch) and the copy of
    the counts to the host;
  * the host path, wall time, in the same process: the device-to-host copy of both lists and notes.note_match_ticks;
  * the yardstick: mt_note_match_list (decoding and streaming match in one kernel) on the same logits and reference list.

    python tools/note_ticks_bench.py [--iters 20] [--out note_ticks_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host_iters", type=int, default=3)
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd import notes as N
    if not torch.cuda.is_available():
        raise SystemExit("note_ticks_bench measures on the GPU only")
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr

    Bn, T = 8, int(args.minutes * 60 * 16000 / 512)
    lengths = [T - 37 * b for b in range(Bn)]
    g = torch.Generator(device="cuda").manual_seed(1)
    centre = (torch.rand(Bn, 88, T // 19 + 1, device="cuda", generator=g) * 19).cumsum(-1) * 2.0
    t = torch.arange(T, device="cuda", dtype=torch.float32)
    idx = torch.searchsorted(centre, t.expand(Bn, 88, T).contiguous()).clamp(1, centre.shape[-1] - 1)
    d = torch.minimum((centre.gather(-1, idx) - t).abs(), (centre.gather(-1, idx - 1) - t).abs())
    x = torch.logit((1.0 - d / 2.0).clamp(0.0, 1.0), eps=1e-6).contiguous()
    est = N.notes_ticks_tables_device(x, x, 0.5, 0.5, lengths)
    h_est = {k: v.cpu().numpy() for k, v in est.items()}

    rng = np.random.default_rng(0)                                           # the reference: the same notes, jittered, thinned, with strays
    r_on, r_off, r_ptr = [], [], [0]
    for r in range(Bn * 88):
        on, off = (h_est[k][h_est["ptr"][r]:h_est["ptr"][r + 1]].astype(np.int64) for k in ("on", "off"))
        keep = rng.random(on.size) >= 0.1
        on, off = on[keep], off[keep]
        k = int((~keep).sum())
        s = rng.integers(0, 320 * T, size=k)
        on = np.concatenate([np.clip(on + rng.integers(-400, 401, size=on.size), 0, None), s])
        off = np.concatenate([off + rng.integers(-400, 401, size=off.size), s + rng.integers(320, 6400, size=k)])
        order = np.argsort(on, kind="stable")
        r_on += on[order].tolist()
        r_off += np.maximum(off[order], on[order] + 1).tolist()
        r_ptr.append(len(r_on))
    h_ref = {"on": np.array(r_on, np.int32), "off": np.array(r_off, np.int32), "ptr": np.array(r_ptr, np.int64)}
    ref = {k: torch.from_numpy(v).cuda() for k, v in h_ref.items()}

    want = N.note_match_ticks(h_est, h_ref).astype(np.int64)
    got = N.note_match_ticks_device(est, ref).cpu().numpy()
    if not np.array_equal(got, want):
        raise SystemExit(f"the device counts differ from the host matcher's: {got.tolist()} != {want.tolist()}")
    n_est, n_ref = int(est["on"].numel()), int(ref["on"].numel())
    res = {"recordings": Bn, "frames": T, "n_est": n_est, "n_ref": n_ref, "counts_sum": want.sum(0).tolist(), "iters": args.iters,
           "launches_per_window": args.launches}

    def device_us(fn):
        """Per launch: (median, min, max) over windows of `launches` launches between one pair of device events."""
        for _ in range(5):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
        torch.cuda.synchronize()
        us = [a.elapsed_time(b) * 1e3 / args.launches for a, b in ev]
        return [round(float(v), 2) for v in (np.median(us), min(us), max(us))]

    def wall_ms(fn, iters):
        fn()
        out = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return [round(float(v), 3) for v in (np.median(out), min(out), max(out))]

    counts = torch.empty(Bn, 4, dtype=torch.int64, device="cuda")
    size = int(lib.mt_note_match_ticks_workspace(n_est, n_ref))
    ws = torch.empty(size, dtype=torch.uint8, device="cuda")
    res["workspace_bytes"] = size
    res["note_match_ticks_us"] = device_us(lambda: _lib.check(lib.mt_note_match_ticks(
        ptr(est["on"]), ptr(est["off"]), ptr(est["ptr"]), ptr(ref["on"]), ptr(ref["off"]), ptr(ref["ptr"]), None, ptr(counts), Bn, 88, ptr(ws), size,
        st()), "mt_note_match_ticks"))
    ln = torch.tensor(lengths, dtype=torch.int64, device="cuda")
    res["note_match_list_us"] = device_us(lambda: _lib.check(lib.mt_note_match_list(
        ptr(x), ptr(x), 0.5, 0.5, ptr(ref["on"]), ptr(ref["off"]), ptr(ref["ptr"]), ptr(ln), ptr(counts), Bn, 88, T, st()), "mt_note_match_list"))
    res["device_path_wall_ms"] = wall_ms(lambda: N.note_match_ticks_device(est, ref).cpu(), max(args.iters, 10))
    res["host_path_wall_ms"] = wall_ms(lambda: N.note_match_ticks({k: v.cpu().numpy() for k, v in est.items()},
                                                                  {k: v.cpu().numpy() for k, v in ref.items()}), args.host_iters)
    res["device_path_faster"] = bool(res["device_path_wall_ms"][0] < res["host_path_wall_ms"][0])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
