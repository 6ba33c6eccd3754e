"""Device time of mt_note_match_counts and mt_note_match_list (DESIGN.md "Note-level F1"), frame, onset-gated and offset-gated decoders,
of mt_heads_to_notes beside mt_heads_to_notes_off (chunks) and of mt_notes_batch (recordings), and of the four cleaning kernels, on two shapes:

  * chunks:     a batch of 128 chunks x 88 pitches x 938 frames (one forward's worth of 30 s chunks);
  * recordings: a padded batch of 8 whole recordings of 10-25 minutes (T up to ~47 000 frames), masked by `lengths`.

Inputs are seeded synthetic logits and rolls with note-like runs (~6 % of the cells active).  Each case is warmed up, then
timed with device events over --iters launches; GB/s counts the bytes the pass must read: the valid frames of the frame
logits, the reference roll and (onset decoder) the onset logits.  The list matcher runs in the same process on the same logits,
its note list being the runs of the same roll (so its counts must equal the roll matcher's); it reads the note list instead of
the roll, and `list_over_roll` is its time over mt_note_match_counts'.  The offset-gated decoder ("onset_offset", the mt_*_off entry
points) reads one array more, offset logits that mark the last active frame of every run; `over_onset` is its time over the
onset-gated entry point's in the same run (expected about 4/3 for the roll matcher, 3/2 for the list matcher and the note lists).
The four cleaning kernels (mt_*_clean, DESIGN.md 6c "Note cleanup") run last, onset-gated at (min_note_frames, bridge_frames) = CLEAN: "*_clean" beside
its counterpart of the same run, `over_plain` = its time over the counterpart's; they read the same bytes.
`--onset-detect peak` adds the peak-picking kernels (mt_*_peak, DESIGN.md 6c "Peak-picked onsets") at reach 1 and 8, onset-gated without
cleanup: "*_peak_r<R>" beside "*_clean_1_0", the _clean entry point at (1, 0) in the same process on the same logits, `peak_over_edge` =
its time over that one's.  The same kernels but for where a note opens, the same bytes.

    python tools/note_metrics_bench.py [--iters 50] [--onset-detect peak] [--out note_metrics.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 16000 / 512


def runs(gen, shape, p_on, p_off, device):
    """Boolean rows of runs (a two-state chain along the last axis), built on the device."""
    import torch
    state = torch.rand(shape[:-1], device=device, generator=gen) < p_on / (p_on + p_off)
    u = torch.rand(shape, device=device, generator=gen)
    out = torch.empty(shape, dtype=torch.bool, device=device)
    for t in range(shape[-1]):
        state = torch.where(state, u[..., t] >= p_off, u[..., t] < p_on)
        out[..., t] = state
    return out


def make_case(B, P, T, lengths, seed, device):
    import torch
    gen = torch.Generator(device=device).manual_seed(seed)
    ref = runs(gen, (B, P, T), 0.02, 0.3, device)
    flip = torch.rand((B, P, T), device=device, generator=gen) < 0.01
    est = ref ^ flip
    mag = torch.rand((B, P, T), device=device, generator=gen) * 4.0 + 0.01
    frame = torch.where(est, mag, -mag)
    onset = torch.where(est & ~torch.nn.functional.pad(est, (1, 0))[..., :-1], mag, -mag)
    if lengths is not None:
        for b, n in enumerate(lengths):
            ref[b, :, n:] = False
    return frame.contiguous(), onset.contiguous(), ref.float().contiguous()


def offset_logits(frame):
    """Offset logits for `frame`: active on the last active frame of every run, with the frame logit's magnitude."""
    import torch
    est = frame > 0
    last = est & ~torch.nn.functional.pad(est, (0, 1))[..., 1:]
    return torch.where(last, frame.abs(), -frame.abs()).contiguous()


def device_ms(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_offset_decoder(out, frame, onset, ref, notes, lengths, iters):
    """The offset-gated entry points beside the onset-gated ones of `out` (same process, same logits), and the two note extractors."""
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import note_match_counts, note_match_list
    B, P, T = frame.shape
    valid = out["valid_frames"]
    off = offset_logits(frame)
    for key, fn, nbytes in (("onset_offset", lambda: note_match_counts(frame, ref, 0.5, onset, 0.5, lengths, offset_logits=off), valid * P * 16),
                            ("onset_offset_list", lambda: note_match_list(frame, notes, 0.5, onset, 0.5, lengths, offset_logits=off),
                             valid * P * 12 + 8 * out["list_notes"])):
        ms = device_ms(fn, iters)
        cs = fn().sum(0).tolist()
        base = out["onset_list" if key.endswith("_list") else "onset"]
        out[key] = {"ms": round(ms, 4), "read_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                    "over_onset": round(ms / base["ms"], 3), "n_ref": cs[0], "n_est": cs[1], "tp_onset": cs[2], "tp_onset_offset": cs[3]}
        if [out[key][k] for k in ("n_ref", "n_est", "tp_onset")] != [base[k] for k in ("n_ref", "n_est", "tp_onset")]:
            raise SystemExit(f"{out['case']} ({key}): the offset head changed more than tp_onset_offset: {out[key]} vs {base}")
    if lengths is not None:                                    # mt_heads_to_notes takes whole chunks: the note lists are timed on the chunks case
        return
    counts = torch.empty(P, dtype=torch.int32, device=frame.device)
    cap = B * P * T // 2 + 1                                   # every note has a frame and a gap of its own
    starts, ends = torch.empty(cap, dtype=torch.int32, device=frame.device), torch.empty(cap, dtype=torch.int32, device=frame.device)
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr()
    gated = lambda: _lib.check(lib.mt_heads_to_notes(ptr(frame), ptr(onset), 0.5, 0.5, B, P, T, ptr(counts), ptr(starts), ptr(ends), cap, st))
    cut = lambda: _lib.check(lib.mt_heads_to_notes_off(ptr(frame), ptr(onset), ptr(off), 0.5, 0.5, 0.5, B, P, T, ptr(counts), ptr(starts),
                                                       ptr(ends), cap, st))
    for key, fn, arrays in (("heads_to_notes", gated, 2), ("heads_to_notes_off", cut, 3)):
        ms = device_ms(fn, iters)
        nbytes = 2 * arrays * valid * P * 4                    # a counting and a writing pass
        out[key] = {"ms": round(ms, 4), "read_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                    "notes": int(counts.sum())}
    out["heads_to_notes_off"]["over_onset"] = round(out["heads_to_notes_off"]["ms"] / out["heads_to_notes"]["ms"], 3)
    if out["heads_to_notes_off"]["notes"] != out["heads_to_notes"]["notes"]:
        raise SystemExit(f"{out['case']}: the offset-gated note list has another number of notes: {out}")


def time_notes_batch(out, frame, onset, lengths, iters):
    """mt_notes_batch (count, prefix, fill) on the padded recordings, frame and onset-gated decoder, at a capacity that holds every note."""
    import torch
    from music_transcription_amd import _lib
    B, P, T = frame.shape
    dev = frame.device
    ln = torch.tensor(lengths, dtype=torch.int64, device=dev)
    counts, row_off = torch.empty(B * P, dtype=torch.int32, device=dev), torch.empty(B * P + 1, dtype=torch.int64, device=dev)
    cap = B * P * T // 2 + 1
    starts, ends = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr()
    for key, on in (("notes_batch_frame", None), ("notes_batch_onset", onset)):
        fn = lambda: _lib.check(lib.mt_notes_batch(ptr(frame), ptr(on), 0.5, 0.5, ptr(ln), B, P, T, ptr(counts), ptr(row_off), ptr(starts),
                                                   ptr(ends), cap, st))
        ms = device_ms(fn, iters)
        nbytes = 2 * (2 if on is not None else 1) * out["valid_frames"] * P * 4        # a counting and a writing pass
        out[key] = {"ms": round(ms, 4), "read_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                    "notes": int(row_off[-1])}
        if out[key]["notes"] != out["onset" if on is not None else "frame"]["n_est"]:
            raise SystemExit(f"{out['case']} ({key}): mt_notes_batch finds another number of notes than the matcher: {out}")


CLEAN = (2, 1)                     # drop one-frame notes, bridge one-frame gaps


def time_clean(out, frame, onset, ref, notes, lengths, iters):
    """The cleaning kernels beside their counterparts in `out`: the two matchers on both shapes, mt_heads_to_notes_clean on the chunks,
    mt_notes_batch_clean on the recordings."""
    import torch
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import note_match_counts, note_match_list
    B, P, T = frame.shape
    dev = frame.device
    kw = dict(min_note_frames=CLEAN[0], bridge_frames=CLEAN[1])
    cases = [("onset", "onset_clean", lambda: note_match_counts(frame, ref, 0.5, onset, 0.5, lengths, **kw)),
             ("onset_list", "onset_list_clean", lambda: note_match_list(frame, notes, 0.5, onset, 0.5, lengths, **kw))]
    for base, key, fn in cases:
        ms = device_ms(fn, iters)
        cs = fn().sum(0).tolist()
        out[key] = {"ms": round(ms, 4), "over_plain": round(ms / out[base]["ms"], 3), "n_ref": cs[0], "n_est": cs[1], "tp_onset": cs[2],
                    "tp_onset_offset": cs[3]}
    if out["onset_clean"]["n_est"] != out["onset_list_clean"]["n_est"] or out["onset_clean"]["n_est"] >= out["onset"]["n_est"]:
        raise SystemExit(f"{out['case']}: the cleaning matchers disagree, or dropped nothing: {out['onset_clean']} vs {out['onset_list_clean']}")
    cap = B * P * T // 2 + 1
    starts, ends = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr()
    if lengths is None:
        counts = torch.empty(P, dtype=torch.int32, device=dev)
        base, key = "heads_to_notes", "heads_to_notes_clean"
        fn = lambda: _lib.check(lib.mt_heads_to_notes_clean(ptr(frame), ptr(onset), None, 0.5, 0.5, 0.5, B, P, T, ptr(counts), ptr(starts),
                                                            ptr(ends), cap, *CLEAN, st))
        total = lambda: int(counts.sum())
    else:
        ln = torch.tensor(lengths, dtype=torch.int64, device=dev)
        counts, row_off = torch.empty(B * P, dtype=torch.int32, device=dev), torch.empty(B * P + 1, dtype=torch.int64, device=dev)
        base, key = "notes_batch_onset", "notes_batch_onset_clean"
        fn = lambda: _lib.check(lib.mt_notes_batch_clean(ptr(frame), ptr(onset), 0.5, 0.5, ptr(ln), B, P, T, ptr(counts), ptr(row_off),
                                                         ptr(starts), ptr(ends), cap, *CLEAN, st))
        total = lambda: int(row_off[-1])
    ms = device_ms(fn, iters)
    out[key] = {"ms": round(ms, 4), "over_plain": round(ms / out[base]["ms"], 3), "notes": total()}
    if lengths is not None and out[key]["notes"] != out["onset_clean"]["n_est"]:
        raise SystemExit(f"{out['case']} ({key}): another number of notes than the cleaning matcher: {out}")


PEAK_REACHES = (1, 8)


def time_peak(out, frame, onset, ref, notes, lengths, iters):
    """The peak-picking entry points beside their _clean namesakes at (1, 0), called directly: the two matchers on both shapes,
    mt_heads_to_notes_* on the chunks, mt_notes_batch_* on the recordings."""
    import torch
    from music_transcription_amd import _lib
    B, P, T = frame.shape
    dev = frame.device
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr()
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=dev)
    c4 = torch.empty(B, 4, dtype=torch.int64, device=dev)
    cap = B * P * T // 2 + 1
    starts, ends = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    heads = (ptr(frame), ptr(onset), None, 0.5, 0.5, 0.5)
    families = [("note_match_counts", lambda f, tail: f(*heads, ptr(ref), ptr(ln), ptr(c4), B, P, T, 1, 0, *tail, st)),
                ("note_match_list", lambda f, tail: f(*heads, ptr(notes["on"]), ptr(notes["off"]), ptr(notes["ptr"]), ptr(ln), ptr(c4), B, P, T, 1, 0,
                                                      *tail, st))]
    if lengths is None:
        counts = torch.empty(P, dtype=torch.int32, device=dev)
        families.append(("heads_to_notes", lambda f, tail: f(*heads, B, P, T, ptr(counts), ptr(starts), ptr(ends), cap, 1, 0, *tail, st)))
    else:
        counts, row_off = torch.empty(B * P, dtype=torch.int32, device=dev), torch.empty(B * P + 1, dtype=torch.int64, device=dev)
        families.append(("notes_batch", lambda f, tail: f(ptr(frame), ptr(onset), 0.5, 0.5, ptr(ln), B, P, T, ptr(counts), ptr(row_off),
                                                          ptr(starts), ptr(ends), cap, 1, 0, *tail, st)))
    for family, call in families:
        edge = getattr(lib, f"mt_{family}_clean")
        base = device_ms(lambda: _lib.check(call(edge, ())), iters)
        out[f"{family}_clean_1_0"] = {"ms": round(base, 4)}
        for R in PEAK_REACHES:
            peak = getattr(lib, f"mt_{family}_peak")
            ms = device_ms(lambda: _lib.check(call(peak, (R,))), iters)
            out[f"{family}_peak_r{R}"] = {"ms": round(ms, 4), "peak_over_edge": round(ms / base, 3)}


def roll_notes(ref):
    """The runs of the (B, P, T) roll as a note list in ticks (320 per frame) on the device: {"on", "off", "ptr"}."""
    import torch
    B, P, T = ref.shape
    r = torch.nn.functional.pad(ref.reshape(B * P, T) > 0, (1, 1))
    rows, s = torch.nonzero(r[:, 1:] & ~r[:, :-1], as_tuple=True)          # row-major: every row's runs in time order
    _, e = torch.nonzero(~r[:, 1:] & r[:, :-1], as_tuple=True)
    ptr = torch.zeros(B * P + 1, dtype=torch.int64, device=ref.device)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=B * P), 0)
    return {"on": (320 * s).int().contiguous(), "off": (320 * e).int().contiguous(), "ptr": ptr}


def time_case(name, frame, onset, ref, lengths, iters, peak=False):
    from music_transcription_amd.notes import note_match_counts, note_match_list
    B, P, T = frame.shape
    valid = B * T if lengths is None else int(sum(lengths))
    out = {"case": name, "B": B, "P": P, "T": T, "valid_frames": valid}
    for dec, on in (("frame", None), ("onset", onset)):
        ms = device_ms(lambda: note_match_counts(frame, ref, 0.5, on, 0.5, lengths), iters)
        c = note_match_counts(frame, ref, 0.5, on, 0.5, lengths)
        nbytes = valid * P * 4 * (3 if on is not None else 2)
        cs = c.sum(0).tolist()
        out[dec] = {"ms": round(ms, 4), "read_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                    "n_ref": cs[0], "n_est": cs[1], "tp_onset": cs[2], "tp_onset_offset": cs[3]}
    notes = roll_notes(ref)
    out["list_notes"] = int(notes["on"].numel())
    for dec, on in (("frame", None), ("onset", onset)):
        ms = device_ms(lambda: note_match_list(frame, notes, 0.5, on, 0.5, lengths), iters)
        c = note_match_list(frame, notes, 0.5, on, 0.5, lengths)
        nbytes = valid * P * 4 * (2 if on is not None else 1) + 8 * out["list_notes"]
        cs = c.sum(0).tolist()
        out[dec + "_list"] = {"ms": round(ms, 4), "read_MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                              "list_over_roll": round(ms / out[dec]["ms"], 3), "n_ref": cs[0], "n_est": cs[1], "tp_onset": cs[2],
                              "tp_onset_offset": cs[3]}
        same = [out[dec][k] == out[dec + "_list"][k] for k in ("n_ref", "n_est", "tp_onset", "tp_onset_offset")]
        if not all(same):
            raise SystemExit(f"{name} ({dec}): the list matcher's counts differ from the roll matcher's on the roll's own runs: "
                             f"{out[dec]} vs {out[dec + '_list']}")
    time_offset_decoder(out, frame, onset, ref, notes, lengths, iters)
    if lengths is not None:
        time_notes_batch(out, frame, onset, lengths, iters)
    time_clean(out, frame, onset, ref, notes, lengths, iters)
    if peak:
        time_peak(out, frame, onset, ref, notes, lengths, iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--onset-detect", choices=["edge", "peak"], default="edge",
                    help="peak: also time the mt_*_peak entry points beside their _clean namesakes at (1, 0)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import music_transcription_amd  # noqa: F401  (loads libmt_hip.so)
    if not torch.cuda.is_available():
        raise SystemExit("note_metrics_bench measures on the GPU only")
    dev = "cuda"
    res = []
    frame, onset, ref = make_case(128, 88, 938, None, 1, dev)
    res.append(time_case("chunks 128 x 88 x 938", frame, onset, ref, None, args.iters, args.onset_detect == "peak"))
    minutes = np.random.default_rng(2).uniform(10.0, 25.0, size=8)
    minutes[0] = 25.0
    lengths = [int(m * 60 * FS) for m in minutes]
    frame, onset, ref = make_case(8, 88, max(lengths), lengths, 3, dev)
    res.append(time_case("recordings 8 x 10-25 min, padded", frame, onset, ref, lengths, args.iters, args.onset_detect == "peak"))
    res[-1]["lengths"] = lengths
    for r in res:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
