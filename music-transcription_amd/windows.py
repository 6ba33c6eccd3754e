"""Whole recordings in overlapping 30 s windows on ONE frame grid (DESIGN.md "Whole recordings in overlapping windows").

The reference's chunking (main.py:60-100, combine_piano_rolls main.py:164-186) runs each 480 000-sample chunk as 938 frames and
concatenates them, but a chunk spans 937.5 hops: chunk k's notes land 16 ms x k late.  Here every window starts on the 512-sample
hop, so window frame t IS global frame a_k + t, and each global frame is taken from exactly one window, away from its edges:

  * plan_windows: start frames and the kept local range of every window (host, integers only);
  * transcribe_windows: device recordings -> (88, 1 + n // 512) logits per recording; the windows of all recordings run in slabs,
    each slab one mt_mel_db_windows_f32 launch, one forward and one mt_stitch_windows launch per head;
  * collect_logits_windows: the same over a whole-file MaestroDataset, with evaluate.collect_logits' output.
Each window keeps its own -80 dB floor (chunk_max_power), as in training.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .frontend import get_frontend

SR, HOP, WINDOW_SAMPLES, N_PITCH = 16000, 512, 480000, 88
MIN_OVERLAP_FRAMES = 8       # n_fft 2048 centre padding reaches 2 frames into a window: O >= 8 keeps every kept frame interior
_ALIGN, _PAD = 64, 64        # floats: recording alignment and readable tail of the store (as rawdata.RecordingStore)


class WindowPlan(NamedTuple):
    """Frames of the hop grid: window k reads samples [hop * start[k], hop * start[k] + window_samples) (zero at or past n) and
    its local frames [lo[k], hi[k]) are global frames [start[k] + lo[k], start[k] + hi[k])."""
    start: np.ndarray        # int64 (K,)
    lo: np.ndarray           # int64 (K,)
    hi: np.ndarray           # int64 (K,)
    Tw: int                  # frames per window
    Tg: int                  # frames of the recording: 1 + n // hop
    O: int                   # overlap in frames
    S: int                   # stride in frames


def overlap_frames(overlap_s: float, sr: int = SR, hop: int = HOP, window_samples: int = WINDOW_SAMPLES) -> int:
    """round(overlap_s * sr / hop), refused outside [MIN_OVERLAP_FRAMES, Tw // 2] with the allowed range in seconds."""
    Tw = 1 + window_samples // hop
    o = float(overlap_s)
    O = int(round(o * sr / hop)) if np.isfinite(o) else -1
    if not MIN_OVERLAP_FRAMES <= O <= Tw // 2:
        raise ValueError(f"window overlap must be between {MIN_OVERLAP_FRAMES * hop / sr:g} s and {(Tw // 2) * hop / sr:g} s "
                         f"({MIN_OVERLAP_FRAMES}..{Tw // 2} frames of {hop} samples at {sr} Hz), got {overlap_s!r}")
    return O


def plan_windows(n_samples: int, overlap_s: float, sr: int = SR, hop: int = HOP, window_samples: int = WINDOW_SAMPLES) -> WindowPlan:
    """Windows of `window_samples` starting on the hop grid with `overlap_s` of overlap, the last one right-aligned to the
    recording's end (fewer than `hop` zero samples past n).  Consecutive windows a < a' meet in the middle of their overlap,
    a' + (a + Tw - a') // 2; window 0 owns from frame 0, the last window up to Tg."""
    n = int(n_samples)
    if n < 0:
        raise ValueError(f"n_samples must be >= 0, got {n}")
    Tw = 1 + window_samples // hop
    O = overlap_frames(overlap_s, sr, hop, window_samples)
    S = Tw - O
    Tg = 1 + n // hop
    L = max(0, -(-(n - window_samples) // hop))
    start = np.concatenate([np.arange(0, L, S, dtype=np.int64), np.array([L], np.int64)])
    bounds = start[1:] + (start[:-1] + Tw - start[1:]) // 2
    own0 = np.concatenate([[0], bounds]).astype(np.int64)
    own1 = np.concatenate([bounds, [Tg]]).astype(np.int64)
    return WindowPlan(start, own0 - start, own1 - start, Tw, Tg, O, S)


def _window_setup(model, n_mels: Optional[int], all_heads: bool, device, with_offset: bool = False):
    """-> (net, n_mels, frontend) of a window pass; refuses all_heads for a model without the onset head."""
    from .evaluate import require_heads
    net = getattr(model, "model", model)
    if with_offset and not all_heads:
        raise ValueError("with_offset=True needs all_heads=True (the offset logits come with the onset logits)")
    if all_heads:
        require_heads(net, "all_heads=True")
    n_mels = int(net.n_mels if n_mels is None else n_mels)
    return net, n_mels, get_frontend(SR, n_mels, HOP, device)


def _run_slab(net, fe, n_mels: int, slab, buf, offs, outs, all_heads: bool, dev, with_offset: bool = False):
    """One slab of window jobs on the current stream: mt_mel_db_windows_f32 on the store `buf` (offs[key] = first float of a
    recording), one forward with the slab's chunk_max_power, one mt_stitch_windows per head into outs [(R, 88, T_dst)]."""
    Tw = 1 + WINDOW_SAMPLES // HOP
    B = len(slab)
    R, T_dst = int(outs[0].shape[0]), int(outs[0].shape[2])
    rows, keys, ns, starts, lo, hi = (np.array(c) for c in zip(*slab))
    h64 = torch.empty((2, B), dtype=torch.int64, pin_memory=True)
    h64.copy_(torch.from_numpy(np.stack([np.array([offs[k] for k in keys.tolist()]) + HOP * starts, starts]).astype(np.int64)))
    h32 = torch.empty((6, B), dtype=torch.int32, pin_memory=True)      # win_len, rec_end, t_keep, dst_row, keep_lo, keep_hi
    h32.copy_(torch.from_numpy(np.stack([np.full(B, WINDOW_SAMPLES), ns - HOP * starts, np.full(B, Tw), rows, lo, hi]).astype(np.int32)))
    with torch.cuda.device(dev):
        d64, d32 = h64.to(dev, non_blocking=True), h32.to(dev, non_blocking=True)
        mel = torch.empty(B, 1, n_mels, Tw, dtype=torch.float32, device=dev)
        cmax = torch.empty(B, dtype=torch.float32, device=dev)
        check(lib.mt_mel_db_windows_f32(ptr(fe.plan), fe.desc, ptr(buf), ptr(d64[0]), ptr(d32[0]), ptr(d32[1]), B, WINDOW_SAMPLES, Tw,
                                        ptr(d32[2]), ptr(mel), ptr(cmax), _lib.stream_ptr()), "mt_mel_db_windows_f32")
        if all_heads:
            heads = net(mel, chunk_max_power=cmax, return_all_heads=True)
            srcs = (heads["frame"], heads["onset"]) + ((heads["offset"],) if with_offset else ())
        else:
            srcs = (net(mel, chunk_max_power=cmax),)
        for src, dst in zip(srcs, outs):
            check(lib.mt_stitch_windows(ptr(src.contiguous()), B, N_PITCH, Tw, ptr(d32[3]), ptr(d64[1]), ptr(d32[4]), ptr(d32[5]),
                                        ptr(dst), R, T_dst, _lib.stream_ptr()), "mt_stitch_windows")


@torch.no_grad()
def _run_windows(model, jobs, R: int, T_dst: int, store_of, n_mels: Optional[int], batch: int, all_heads: bool, device,
                 with_offset: bool = False):
    """jobs: [(dst_row, recording key, n_samples, start frame, lo, hi)].  store_of(keys) -> (store buffer, {key: offset}) for the
    recordings of one slab.  -> frame logits (R, 88, T_dst) [, onset logits [, offset logits]], padding 0."""
    net, n_mels, fe = _window_setup(model, n_mels, all_heads, device, with_offset)
    dev = torch.device(device)
    outs = [torch.zeros(R, N_PITCH, T_dst, dtype=torch.float32, device=dev) for _ in range((3 if with_offset else 2) if all_heads else 1)]
    for s0 in range(0, len(jobs), batch):
        slab = jobs[s0:s0 + batch]
        buf, offs = store_of([job[1] for job in slab])
        _run_slab(net, fe, n_mels, slab, buf, offs, outs, all_heads, dev, with_offset)
    if hasattr(net, "raise_on_handoff_timeout"):
        net.raise_on_handoff_timeout(sync=True)        # a timed-out recurrence would have left NaN logits: fail loudly, once per pass
    return outs


def _store(recordings: Sequence[torch.Tensor]):
    """The recordings side by side in one zero-padded buffer (64-float alignment and tail, as rawdata.RecordingStore) -> (buffer,
    offsets, sample counts)."""
    dev = recordings[0].device
    ns = [int(y.numel()) for y in recordings]
    offs, pos = [], 0
    for n in ns:
        offs.append(pos)
        pos += -(-max(n, 1) // _ALIGN) * _ALIGN
    store = torch.zeros(pos + _PAD, dtype=torch.float32, device=dev)
    for y, o, n in zip(recordings, offs, ns):
        store[o:o + n].copy_(y)
    return store, offs, ns


def _jobs(ns: Sequence[int], keys: Sequence, overlap_s: float):
    jobs = []
    for row, (n, key) in enumerate(zip(ns, keys)):
        p = plan_windows(int(n), overlap_s)
        jobs += [(row, key, int(n), int(a), int(lo), int(hi)) for a, lo, hi in zip(p.start, p.lo, p.hi)]
    return jobs


def transcribe_windows(model, recordings: Sequence[torch.Tensor], overlap_s: float, batch: int = 128, all_heads: bool = False,
                       n_mels: Optional[int] = None, with_offset: bool = False) -> List:
    """1-D float32 device recordings at 16 kHz -> per recording frame logits (88, 1 + n // 512) on the recording's own frame grid
    (the frames of one mel over the whole recording), on the device; all_heads=True: [(frame, onset)] (cnn_rnn_large with heads),
    and with with_offset=True [(frame, onset, offset)].  The windows of all recordings run in slabs of `batch`."""
    if not len(recordings):
        return []
    overlap_frames(overlap_s)
    dev = recordings[0].device
    if dev.type != "cuda" or any(y.dim() != 1 or y.dtype != torch.float32 or y.device != dev for y in recordings):
        raise ValueError("transcribe_windows expects 1-D float32 recordings on one CUDA device")
    store, offs, ns = _store(recordings)
    Tg = [1 + n // HOP for n in ns]
    outs = _run_windows(model, _jobs(ns, range(len(ns)), overlap_s), len(ns), max(Tg), lambda keys: (store, offs), n_mels, batch,
                        all_heads, dev, with_offset)
    res = []
    for r, t in enumerate(Tg):
        heads = [o[r] if t == o.shape[-1] else o[r, :, :t].contiguous() for o in outs]
        res.append(tuple(heads) if all_heads else heads[0])
    return res


@torch.no_grad()
def collect_logits_windows(model, dataset, indices: Sequence[int], overlap_s: float, device="cuda", max_batch: int = 128,
                           all_heads: bool = False, with_offset: bool = False):
    """evaluate.collect_logits for a whole-file MaestroDataset (chunk_length=None) through overlapping windows: the same tuples,
    [(index, logits (88, t_keep), roll (88, t_keep)[, onset logits[, offset logits]])] sorted by index (the offset logits with
    all_heads=True, with_offset=True), with the logits stitched on the recording's
    grid and trimmed to the item's t_keep, and the roll the item's full-file label roll.  Reuses the dataset's recording store."""
    if getattr(dataset, "chunk_length", 0) is not None or not hasattr(dataset, "store"):
        raise ValueError("collect_logits_windows needs a whole-file MaestroDataset (chunk_length=None)")
    overlap_frames(overlap_s)
    idx = sorted(int(i) for i in indices)
    if not idx:
        return []
    ds = dataset
    recs = [int(ds.rec[i]) for i in idx]
    ns = [int(ds.store.n[r]) for r in recs]
    t_keep = ds.t_keep[idx].astype(np.int64)
    T_dst = max(1 + n // HOP for n in ns)
    outs = _run_windows(model, _jobs(ns, recs, overlap_s), len(idx), T_dst, lambda keys: (ds.store.buf, ds.store.offsets(keys)),
                        ds.n_mels, max_batch, all_heads, device, with_offset)
    # labels: mt_roll_windows in full-file mode (column n is frame n), as MaestroDataset.get_batch builds them
    B, T_roll = len(idx), max(int(t_keep.max()), 1)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        d64 = torch.full((B,), -1, dtype=torch.int64).to(dev)
        d32 = torch.from_numpy(np.stack([np.array(recs), np.zeros(B), t_keep]).astype(np.int32)).to(dev)
        roll = torch.empty(B, N_PITCH, T_roll, dtype=torch.float32, device=dev)
        check(lib.mt_roll_windows(ptr(ds.spans), ptr(ds.pitch_off), ptr(ds.cols), ptr(d32[0]), ptr(d64), ptr(d32[1]), ptr(d32[2]), B, T_roll,
                                  ptr(roll), _lib.stream_ptr()), "mt_roll_windows")
    out = []
    for b, (i, t) in enumerate(zip(idx, t_keep.tolist())):
        item = [i, outs[0][b, :, :t].contiguous(), roll[b, :, :t].contiguous()]
        if all_heads:
            item += [o[b, :, :t].contiguous() for o in outs[1:]]
        out.append(tuple(item))
    return out
