"""Evaluation on the GPU: the hot loops of scripts/evaluate.py restructured.

  * `evaluate_dataset` = run_evaluation's headless loop (evaluate.py:335-379): per-sample framewise F1 over the valid
    frames (zero_division = 0), unweighted mean.  The reference runs batch 1; samples of EQUAL length are batched
    here (no padding arises, so results are per-sample identical) and the F1 counts are integer sums on the device.
  * `tune_threshold` = run_threshold_tuning (evaluate.py:556-618) with the same coarse-to-fine schedule, but the
    model runs ONCE: logits stay on the device and every candidate threshold is an integer-count pass
    (mt_f1_sweep_counts, up to 16 thresholds per pass).
  * `note_metrics_dataset` = note-level precision / recall / F1 (mir_eval's onset and onset+offset criteria on the frame grid)
    against the runs of the label roll (note_reference="roll") or the MIDI note list of whole recordings ("midi": re-struck keys
    are reference notes of their own, times in 100 us ticks), for the frame decoder or the onset-gated one; decoding and matching
    are one counting pass over the logits (notes.note_match_counts / note_match_list), samples of any length batched through `lengths`.
  * `tune_note_thresholds` = tune_threshold's schedule on note F1, over the frame threshold and (onset-gated decoder) the onset
    threshold at once: the model runs once, every round is one sweep pass per group (notes.note_sweep_counts: each cell's sigmoid is
    evaluated once for the whole grid).  `search_note_thresholds` is the search alone, on any callable.
  * `tune_note_decoder` = the same schedule over every parameter of the note decoder at once, whichever of the three decoders it
    is: up to three thresholds (frame, onset, offset) times a list of note-cleanup candidates, one grid pass per group and round
    (notes.note_grid_counts).  `search_note_decoder` is the search alone.  `smoothings=` adds a list of frame-smoothing penalty
    pairs to the candidates of every round: the discrete axis of the search is then cleanups x smoothings.  `peak_reaches=` adds a
    list of candidate reaches of the peak-picking onset detector, 0 = the edge rule, as its innermost factor.
  * `window_overlap` (seconds, whole-file datasets): every recording runs in overlapping 30 s windows stitched on its own
    frame grid (windows.collect_logits_windows) instead of one recurrence over the whole file;
  * recordings / chunks shard over ranks with no data-path collective (parallel.py); per-sample F1 values are
    gathered with one small all-reduce.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import lib, check, ptr
from .parallel import gather_values, shard_range


def _f1(tp, fp, fn) -> float:
    d = 2 * tp + fp + fn
    return 0.0 if d == 0 else 2.0 * tp / d


def require_heads(model, what: str) -> None:
    """Raise unless `model` is a CNNRNNModelLarge with its onset / offset heads (what the onset-gated decoder reads)."""
    from .model import CNNRNNModelLarge
    net = getattr(model, "model", model)
    if not isinstance(net, CNNRNNModelLarge) or not net.use_onset_offset_heads:
        raise ValueError(f"{what} needs the onset head: a cnn_rnn_large model with use_onset_offset_heads=True "
                         f"(got {type(net).__name__}{'' if not isinstance(net, CNNRNNModelLarge) else ' without heads'})")


@torch.no_grad()
def collect_logits(model, dataset, indices: Sequence[int], device="cuda", max_batch: int = 128, all_heads: bool = False,
                   with_offset: bool = False):
    """Forward every sample once; returns [(index, logits (88, T) on device, roll (88, T) on device)], with all_heads=True
    [(index, frame logits, roll, onset logits)] and with with_offset=True as well [(..., onset logits, offset logits)]."""
    if with_offset and not all_heads:
        raise ValueError("with_offset=True needs all_heads=True (the offset logits come with the onset logits)")
    if all_heads:
        require_heads(model, "collect_logits(all_heads=True)")
    by_len = defaultdict(list)
    for i in indices:
        mel, roll = dataset[i]
        by_len[int(mel.shape[-1])].append((i, mel, roll))
    out = []
    for T, items in by_len.items():
        for s in range(0, len(items), max_batch):
            grp = items[s:s + max_batch]
            mel = torch.stack([m for _, m, _ in grp]).to(device)                    # (b, 1, n_mels, T): equal T, no padding
            if all_heads:
                heads = model(mel, return_all_heads=True)
                for k, ((i, _, roll), lg, on) in enumerate(zip(grp, heads["frame"], heads["onset"])):
                    item = (i, lg.contiguous(), roll.to(device).float().contiguous(), on.contiguous())
                    out.append(item + (heads["offset"][k].contiguous(),) if with_offset else item)
            else:
                logits = model(mel)
                for (i, _, roll), lg in zip(grp, logits):
                    out.append((i, lg.contiguous(), roll.to(device).float().contiguous()))
    net = getattr(model, "model", model)
    if hasattr(net, "raise_on_handoff_timeout"):
        net.raise_on_handoff_timeout(sync=True)        # a timed-out recurrence would have left NaN logits: fail loudly, once per pass
    out.sort(key=lambda x: x[0])
    return out


def f1_at_thresholds(logits_rolls, thresholds: Sequence[float]) -> np.ndarray:
    """mean-over-samples F1 for each threshold; one counts pass per 16 thresholds per sample length group."""
    thresholds = [float(t) for t in thresholds]
    per_sample = np.zeros((len(logits_rolls), len(thresholds)))
    by_len = defaultdict(list)
    for n, (_, lg, roll) in enumerate(logits_rolls):
        by_len[lg.shape[-1]].append(n)
    for T, idxs in by_len.items():
        lg = torch.stack([logits_rolls[n][1] for n in idxs])
        rl = torch.stack([logits_rolls[n][2] for n in idxs])
        B, P, _ = lg.shape
        for k0 in range(0, len(thresholds), 16):
            th = torch.tensor(thresholds[k0:k0 + 16], dtype=torch.float32, device=lg.device)
            K = th.numel()
            counts = torch.empty(B, K, 3, dtype=torch.int64, device=lg.device)
            with torch.cuda.device(lg.device):
                check(lib.mt_f1_sweep_counts(ptr(lg), ptr(rl), None, ptr(th), K, ptr(counts), B, P, T, _lib.stream_ptr()), "mt_f1_sweep_counts")
            c = counts.cpu().numpy()
            for bi, n in enumerate(idxs):
                for k in range(K):
                    per_sample[n, k0 + k] = _f1(*[int(v) for v in c[bi, k]])
    return per_sample


def _collect(model, dataset, indices, device, window_overlap: Optional[float], all_heads: bool = False, with_offset: bool = False):
    """collect_logits, or with window_overlap (seconds) collect_logits_windows over a whole-file dataset."""
    if window_overlap is None:
        return collect_logits(model, dataset, indices, device, all_heads=all_heads, with_offset=with_offset)
    from .windows import collect_logits_windows
    return collect_logits_windows(model, dataset, indices, window_overlap, device, all_heads=all_heads, with_offset=with_offset)


def evaluate_dataset(model, dataset, threshold: float = 0.5, device="cuda", subset: Optional[int] = None,
                     rank: int = 0, world: int = 1, window_overlap: Optional[float] = None) -> Tuple[float, List[float]]:
    """-> (mean F1 over ALL samples, per-sample F1 list), identical on every rank.  window_overlap (seconds): a whole-file
    dataset runs in overlapping 30 s windows stitched on each recording's frame grid (windows.collect_logits_windows)."""
    n = len(dataset) if subset is None else min(subset, len(dataset))
    mine = list(shard_range(n, rank, world))
    lr = _collect(model, dataset, mine, device, window_overlap)
    vals = f1_at_thresholds(lr, [threshold])[:, 0] if lr else np.zeros(0)
    allv = gather_values(mine, vals.tolist(), n)
    return (float(np.mean(allv)) if allv else 0.0), allv


NOTE_METRIC_KEYS = tuple(f"{c}_{m}" for c in ("onset", "onset_offset") for m in ("precision", "recall", "f1"))


def note_metrics_dataset(model, dataset, threshold: float = 0.5, onset_threshold: Optional[float] = None, device="cuda",
                         subset: Optional[int] = None, max_batch: int = 128, rank: int = 0, world: int = 1,
                         window_overlap: Optional[float] = None, note_reference: str = "roll",
                         offset_threshold: Optional[float] = None, min_note_frames: int = 1, bridge_frames: int = 0,
                         smooth_on: float = 0.0, smooth_off: float = 0.0, refine_onsets: bool = False, refine_reach: int = 2,
                         onset_detect: str = "edge", peak_reach: int = 1) -> dict:
    """Note-level metrics of every sample, identical on every rank: {"mean": {key: value}, "per_sample": {key: [values]}} over
    NOTE_METRIC_KEYS (onset / onset_offset x precision / recall / f1).  onset_threshold=None: notes are the runs of
    sigmoid(frame) > threshold (the frame decoder); otherwise the onset-gated decoder with the onset head at onset_threshold.
    offset_threshold (needs onset_threshold): the offset-gated decoder, which also ends notes where the offset head fires.
    Reference notes: note_reference="roll", the runs of the dataset's label roll; "midi", the MIDI note list of each recording
    (dataset.ref_notes: a whole-file MaestroDataset built with onset_labels="midi").  Unweighted means over samples, as
    evaluate_dataset (window_overlap too).  min_note_frames / bridge_frames: the estimates are cleaned in the decoder (DESIGN.md 6c "Note cleanup"),
    whichever of the three it is; the result then names the two ("min_note_frames", "bridge_frames").  smooth_on / smooth_off: the frame
    head is smoothed before the decoder (DESIGN.md 6c "Frame smoothing"); the result then names those two as well.
    refine_onsets (onset-gated or offset-gated decoder, note_reference="midi"): the notes are decoded as lists, their onsets refined to
    sub-frame ticks (mt_refine_onsets with reach refine_reach; DESIGN.md 6c "Sub-frame onsets") and scored in ticks on the device
    (notes.notes_ticks_tables_device, notes.note_match_ticks_device: a maximum matching per pitch row, the counts of the host matcher
    notes.note_match_ticks) -- mt_note_match_list takes estimates on the frame grid only; the result then names "refine_reach".
    onset_detect="peak" (onset-gated or offset-gated decoder): notes open at the peaks of the onset logits over peak_reach frames
    (DESIGN.md 6c "Peak-picked onsets"), on either path; the result then names "onset_detect" and "peak_reach"."""
    from .notes import (check_cleanup, check_onset_detect, check_smoothing, note_match_counts, note_match_list, note_match_ticks_device,
                        note_prf, notes_ticks_tables_device)
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    peak = check_onset_detect(onset_detect, peak_reach, onset_threshold is not None)
    _check_note_reference(dataset, note_reference)
    onset, offset = onset_threshold is not None, offset_threshold is not None
    if offset and not onset:
        raise ValueError("offset_threshold: the offset-gated decoder needs onset_threshold as well")
    if refine_onsets and (not onset or note_reference != "midi"):
        raise ValueError("refine_onsets: sub-frame onsets are read off the onset head and scored against the MIDI note list in ticks: "
                         "it needs onset_threshold (the onset-gated or offset-gated decoder) and note_reference='midi'")
    n = len(dataset) if subset is None else min(subset, len(dataset))
    mine = list(shard_range(n, rank, world))
    lr = _collect(model, dataset, mine, device, window_overlap, all_heads=onset, with_offset=offset)
    vals = {k: [] for k in NOTE_METRIC_KEYS}
    match = note_match_list if note_reference == "midi" else note_match_counts
    for frame, on, ref, lengths, off in _note_groups(lr, dataset, onset, note_reference, max_batch, offset):
        if refine_onsets:
            est = notes_ticks_tables_device(frame, on, threshold, onset_threshold, lengths, offset_logits=off,
                                            offset_threshold=offset_threshold if offset else 0.5, min_note_frames=clean[0],
                                            bridge_frames=clean[1], smooth_on=smooth[0], smooth_off=smooth[1], refine_reach=refine_reach,
                                            onset_detect=onset_detect, peak_reach=peak_reach)
            counts = note_match_ticks_device(est, ref, lengths=None)     # (the whole reference list, as the host matcher scores it)
        else:
            counts = match(frame, ref, threshold, on, onset_threshold if onset else 0.5, lengths, offset_logits=off,
                           offset_threshold=offset_threshold if offset else 0.5, min_note_frames=clean[0], bridge_frames=clean[1],
                           smooth_on=smooth[0], smooth_off=smooth[1], onset_detect=onset_detect, peak_reach=peak_reach)
        for m in note_prf(counts):
            for c in ("onset", "onset_offset"):
                for k, v in zip(("precision", "recall", "f1"), m[c]):
                    vals[f"{c}_{k}"].append(v)
    per = {k: gather_values(mine, v, n) for k, v in vals.items()}
    out = {"mean": {k: (float(np.mean(v)) if v else 0.0) for k, v in per.items()}, "per_sample": per}
    if clean != (1, 0):
        out["min_note_frames"], out["bridge_frames"] = clean
    if smooth != (0.0, 0.0):
        out["smooth_on"], out["smooth_off"] = smooth
    if refine_onsets:
        out["refine_reach"] = int(refine_reach)
    if peak:
        out["onset_detect"], out["peak_reach"] = "peak", peak
    return out


def _refuse_smoothing(who: str, smooth_on, smooth_off) -> None:
    """The tuners search thresholds (and cleanup) on the raw frame head: frame smoothing is refused, before any GPU work."""
    from .notes import check_smoothing
    if check_smoothing(smooth_on, smooth_off) != (0.0, 0.0):
        raise ValueError(f"{who}: the tuners do not smooth the frame head (smooth_on / smooth_off): tune without smoothing, then evaluate "
                         "with it (note_metrics_dataset(..., smooth_on=, smooth_off=))")


def _refuse_peak(who: str, onset_detect, reaches: bool = False) -> None:
    """The tuners run the sweep and grid kernels, which have no peak mode to fix: onset_detect="peak" is refused, before any GPU work
    (reaches: the tuner has peak_reaches=, the grid's axis of candidate reaches, and the message says so)."""
    from .notes import refuse_peak
    refuse_peak(onset_detect, who, reaches)


def _check_note_reference(dataset, note_reference: str) -> None:
    if note_reference not in ("roll", "midi"):
        raise ValueError(f"note_reference must be 'roll' or 'midi', got {note_reference!r}")
    if note_reference == "midi" and (getattr(dataset, "onset_labels", None) != "midi" or getattr(dataset, "chunk_length", 0) is not None):
        raise ValueError("note_reference='midi' scores against the MIDI note list of whole recordings: it needs "
                         "MaestroDataset(chunk_length=None, onset_labels='midi') (scripts/evaluate.py --data_source full)")


def _note_groups(lr, dataset, onset: bool, note_reference: str, max_batch: int, offset: bool = False):
    """The collected samples in groups of max_batch, one counts pass each: (frame (b, 88, T), onset or None, reference roll or note
    list, lengths, offset or None); unequal lengths padded to the group's longest and masked by `lengths`."""
    for s in range(0, len(lr), max_batch):
        grp = lr[s:s + max_batch]
        lengths = [int(x[1].shape[-1]) for x in grp]
        T = max(lengths)
        pad = lambda t: torch.nn.functional.pad(t, (0, T - t.shape[-1]))
        frame = torch.stack([pad(x[1]) for x in grp])
        on = torch.stack([pad(x[3]) for x in grp]) if onset else None
        ref = dataset.ref_notes([x[0] for x in grp]) if note_reference == "midi" else torch.stack([pad(x[2]) for x in grp])
        off = torch.stack([pad(x[4]) for x in grp]) if offset else None
        yield frame, on, ref, lengths, off


def tune_threshold(model, dataset, device="cuda", subset: Optional[int] = None, tune_range=(0.05, 0.95), tune_step=0.1,
                   tune_min_step=0.01, tune_rounds=6, rank: int = 0, world: int = 1, log=print, window_overlap: Optional[float] = None,
                   smooth_on: float = 0.0, smooth_off: float = 0.0, onset_detect: str = "edge"):
    """Coarse-to-fine search of evaluate.py:556-618 (same candidate grids, same strict-improvement rule, same window
    and stopping rule); returns (best_threshold, best_mean_f1).  window_overlap: as evaluate_dataset.  Frame smoothing
    (smooth_on, smooth_off) other than (0, 0) is refused, and so is onset_detect="peak": the frame F1 decodes no notes."""
    _refuse_smoothing("tune_threshold", smooth_on, smooth_off)
    _refuse_peak("tune_threshold", onset_detect)
    n = len(dataset) if subset is None else min(subset, len(dataset))
    mine = list(shard_range(n, rank, world))
    lr = _collect(model, dataset, mine, device, window_overlap)          # the only forward passes
    tune_min, tune_max = tune_range
    step = tune_step
    best_t, best_f1 = 0.5, -1.0
    for rnd in range(1, tune_rounds + 1):
        ths = np.arange(tune_min, tune_max + step / 2, step)
        local = f1_at_thresholds(lr, ths) if lr else np.zeros((0, len(ths)))
        means = []
        for k in range(len(ths)):
            allv = gather_values(mine, local[:, k].tolist(), n)
            means.append(float(np.mean(allv)) if allv else 0.0)
        rb_t, rb_f = best_t, best_f1
        for t, f in zip(ths, means):
            if f > rb_f:
                rb_f, rb_t = f, float(t)
        best_t, best_f1 = rb_t, rb_f
        if log:
            log(f"=== Round {rnd}/{tune_rounds} | range=[{tune_min:.4f}, {tune_max:.4f}] step={step:.4f} -> t={best_t:.4f} f1={best_f1:.6f}")
        tune_min = max(0.01, best_t - 2 * step)
        tune_max = min(0.99, best_t + 2 * step)
        step = step / 2
        if step < tune_min_step:
            break
    return best_t, best_f1


def search_note_thresholds(mean_f1, two_axes: bool = True, tune_range=(0.05, 0.95), tune_step=0.1, tune_min_step=0.01, tune_rounds=6, log=None):
    """tune_threshold's coarse-to-fine schedule on the frame threshold and, with two_axes, the onset threshold at once (no GPU in
    here).  mean_f1(frame_ths, onset_ths) -> (Kf, Ko) array of the objective; onset_ths is None and Ko = 1 without two_axes.  A
    round's candidates on each axis are np.arange(min, max + step / 2, step); pairs are visited frame-major and replace the best
    only on strict improvement, starting from (0.5, 0.5) at -1; the next window on each axis is best +- 2 step clipped to
    [0.01, 0.99]; the step halves, and the search ends when it falls below tune_min_step or after tune_rounds.
    -> (frame threshold, onset threshold or None, best value)."""
    f_min, f_max = tune_range
    o_min, o_max = tune_range
    step = tune_step
    best_f, best_o, best = 0.5, 0.5, -1.0
    for rnd in range(1, tune_rounds + 1):
        fts = np.arange(f_min, f_max + step / 2, step)
        ots = np.arange(o_min, o_max + step / 2, step) if two_axes else None
        means = np.asarray(mean_f1(fts, ots), dtype=np.float64).reshape(len(fts), len(ots) if two_axes else 1)
        for i, t in enumerate(fts):
            for j in range(means.shape[1]):
                if means[i, j] > best:
                    best, best_f = float(means[i, j]), float(t)
                    if two_axes:
                        best_o = float(ots[j])
        if log:
            log(f"=== Round {rnd}/{tune_rounds} | frame=[{f_min:.4f}, {f_max:.4f}]" + (f" onset=[{o_min:.4f}, {o_max:.4f}]" if two_axes else "")
                + f" step={step:.4f} -> t={best_f:.4f}" + (f" onset_t={best_o:.4f}" if two_axes else "") + f" f1={best:.6f}")
        f_min, f_max = max(0.01, best_f - 2 * step), min(0.99, best_f + 2 * step)
        o_min, o_max = max(0.01, best_o - 2 * step), min(0.99, best_o + 2 * step)
        step = step / 2
        if step < tune_min_step:
            break
    return best_f, (best_o if two_axes else None), best


def tune_note_thresholds(model, dataset, device="cuda", subset: Optional[int] = None, decoder: str = "onset", note_reference: str = "roll",
                         objective: str = "onset", tune_range=(0.05, 0.95), tune_step=0.1, tune_min_step=0.01, tune_rounds=6,
                         rank: int = 0, world: int = 1, log=print, window_overlap: Optional[float] = None, max_batch: int = 128,
                         min_note_frames: int = 1, bridge_frames: int = 0, smooth_on: float = 0.0, smooth_off: float = 0.0,
                         onset_detect: str = "edge"):
    """The thresholds of the note decoder that maximise the mean note F1 (`objective`: "onset" or "onset_offset"; unweighted mean
    over samples, as note_metrics_dataset) by search_note_thresholds: decoder="onset" searches (frame, onset) pairs, "frame" the
    frame threshold alone.  The model runs once; every round is one sweep pass over each group of note_metrics_dataset.
    -> (frame threshold, onset threshold or None, best mean F1), identical on every rank.  A candidate at or past 1 (the schedule's
    last grid point can be) decodes no note and scores 0, as it does for tune_threshold.  The sweep kernels do not clean notes:
    anything but (min_note_frames, bridge_frames) = (1, 0) is refused, and so is frame smoothing (smooth_on, smooth_off) other than (0, 0).
    Nor do they pick peaks: onset_detect="peak" is refused."""
    from .notes import check_cleanup, note_prf, note_sweep_counts
    _refuse_smoothing("tune_note_thresholds", smooth_on, smooth_off)
    _refuse_peak("tune_note_thresholds", onset_detect)
    if check_cleanup(min_note_frames, bridge_frames) != (1, 0):
        raise ValueError("tune_note_thresholds: the threshold sweeps do not clean notes (min_note_frames / bridge_frames): tune "
                         "without cleanup, then evaluate with it (note_metrics_dataset(..., min_note_frames=, bridge_frames=))")
    if decoder == "onset_offset":
        raise ValueError("tune_note_thresholds does not cover decoder='onset_offset': the threshold sweeps are not extended to the "
                         "offset head (tune with decoder='onset', then pass offset_threshold to note_metrics_dataset)")
    if decoder not in ("onset", "frame"):
        raise ValueError(f"decoder must be 'onset' or 'frame', got {decoder!r}")
    if objective not in ("onset", "onset_offset"):
        raise ValueError(f"objective must be 'onset' or 'onset_offset', got {objective!r}")
    _check_note_reference(dataset, note_reference)
    onset = decoder == "onset"
    n = len(dataset) if subset is None else min(subset, len(dataset))
    mine = list(shard_range(n, rank, world))
    lr = _collect(model, dataset, mine, device, window_overlap, all_heads=onset)          # the only forward passes

    def mean_f1(fts, ots):
        fts = np.asarray(fts, dtype=np.float64)
        ots = np.asarray(ots, dtype=np.float64) if onset else np.full(1, 0.5)
        if (fts <= 0.0).any() or (ots <= 0.0).any():
            raise ValueError("tune_note_thresholds: candidate thresholds must be positive (tune_range)")
        fi, oj = np.flatnonzero(np.float32(fts) < 1.0), np.flatnonzero(np.float32(ots) < 1.0)
        K = len(fts) * len(ots)
        local = np.zeros((len(lr), len(fts), len(ots)))                                   # thresholds >= 1: no notes, F1 0
        at = 0
        if len(fi) and len(oj):
            for frame, on, ref, lengths, _ in _note_groups(lr, dataset, onset, note_reference, max_batch):
                counts = note_sweep_counts(frame, ref, fts[fi], on, ots[oj] if onset else None, lengths)
                f1 = np.array([m[objective][2] for m in note_prf(counts)]).reshape(len(lengths), len(fi), len(oj))
                local[at:at + len(lengths), fi[:, None], oj[None, :]] = f1
                at += len(lengths)
        flat_idx = [i * K + k for i in mine for k in range(K)]
        allv = gather_values(flat_idx, local.reshape(-1).tolist(), n * K)
        return np.asarray(allv).reshape(n, len(fts), len(ots)).mean(axis=0) if n else np.zeros((len(fts), len(ots)))

    return search_note_thresholds(mean_f1, onset, tune_range, tune_step, tune_min_step, tune_rounds, log)


def search_note_decoder(mean_f1, n_axes: int = 3, n_clean: int = 1, tune_range=(0.05, 0.95), tune_step=0.1, tune_min_step=0.01,
                        tune_rounds=6, log=None):
    """search_note_thresholds' schedule on 1-3 threshold axes (frame; frame, onset; frame, onset, offset) times a fixed list of
    n_clean cleanup candidates that is part of every round (no GPU in here).  mean_f1(frame_ths, onset_ths, offset_ths) ->
    (Kf, Ko, Kk, n_clean) array of the objective; an axis past n_axes is passed as None and has one cell.  A round's candidates on
    each axis are np.arange(min, max + step / 2, step); cells are visited frame-major, then onset, then offset, then cleanup in
    the given order, and replace the best only on strict improvement, starting from all thresholds at 0.5 and cleanup 0 at -1; the
    next window on each axis is best +- 2 step clipped to [0.01, 0.99]; the step halves, and the search ends when it falls below
    tune_min_step or after tune_rounds.  -> (frame, onset or None, offset or None thresholds, cleanup index, best value)."""
    if n_axes not in (1, 2, 3):
        raise ValueError(f"n_axes must be 1, 2 or 3, got {n_axes!r}")
    if n_clean < 1:
        raise ValueError(f"n_clean must be at least 1, got {n_clean!r}")
    names = ("frame", "onset", "offset")[:n_axes]
    lo, hi = [tune_range[0]] * n_axes, [tune_range[1]] * n_axes
    step = tune_step
    best_t, best_c, best = [0.5] * n_axes, 0, -1.0
    for rnd in range(1, tune_rounds + 1):
        grids = [np.arange(lo[a], hi[a] + step / 2, step) for a in range(n_axes)]
        shape = tuple(len(g) for g in grids) + (1,) * (3 - n_axes) + (n_clean,)
        means = np.asarray(mean_f1(*(grids + [None] * (3 - n_axes))), dtype=np.float64).reshape(shape)
        for idx in np.ndindex(*shape):                                       # C order: frame-major, ..., cleanup last
            if means[idx] > best:
                best, best_c = float(means[idx]), idx[3]
                best_t = [float(grids[a][idx[a]]) for a in range(n_axes)]
        if log:
            log(f"=== Round {rnd}/{tune_rounds} | " + " ".join(f"{n}=[{lo[a]:.4f}, {hi[a]:.4f}]" for a, n in enumerate(names))
                + f" step={step:.4f} -> " + " ".join(f"{n}_t={best_t[a]:.4f}" for a, n in enumerate(names))
                + f" cleanup={best_c} f1={best:.6f}")
        for a in range(n_axes):
            lo[a], hi[a] = max(0.01, best_t[a] - 2 * step), min(0.99, best_t[a] + 2 * step)
        step = step / 2
        if step < tune_min_step:
            break
    thr = best_t + [None] * (3 - n_axes)
    return thr[0], thr[1], thr[2], best_c, best


NOTE_DECODER_AXES = {"frame": 1, "onset": 2, "onset_offset": 3}


def decoder_candidate(index: int, cleanups: Sequence, smoothings: Sequence, reaches: Optional[Sequence] = None):
    """Entry `index` of the tuner's discrete axis cleanups x smoothings, cleanup-major -> (cleanup, smoothing); with reaches, of
    cleanups x smoothings x reaches, reaches innermost -> (cleanup, smoothing, reach)."""
    n_reach = 1 if reaches is None else len(reaches)
    if not 0 <= index < len(cleanups) * len(smoothings) * n_reach:
        raise ValueError(f"index {index} outside {len(cleanups)} x {len(smoothings)}" + (f" x {n_reach}" if reaches is not None else "")
                         + " candidates")
    pair = cleanups[index // n_reach // len(smoothings)], smoothings[index // n_reach % len(smoothings)]
    return pair if reaches is None else (*pair, reaches[index % n_reach])


def fold_smoothings(f1: np.ndarray) -> np.ndarray:
    """(n, Kf, Ks, Ko, Kk, Kc) values as notes.note_grid_counts(smoothings=...) orders them -> (n, Kf, Ko, Kk, Kc * Ks), the last
    axis cleanup-major: what search_note_decoder takes with n_clean = Kc * Ks and decoder_candidate reads back."""
    n, Kf, Ks, Ko, Kk, Kc = f1.shape
    return np.ascontiguousarray(np.transpose(f1, (0, 1, 3, 4, 5, 2))).reshape(n, Kf, Ko, Kk, Kc * Ks)


def fold_reaches(f1: np.ndarray) -> np.ndarray:
    """(n, Kf, Ks, Ko, Kk, Kc, Kr) values as notes.note_grid_counts(smoothings=..., peak_reaches=...) orders them -> (n, Kf, Ko, Kk,
    Kc * Ks * Kr), the last axis cleanup-major and reaches innermost: what search_note_decoder takes with n_clean = Kc * Ks * Kr and
    decoder_candidate(..., reaches) reads back.  Without smoothings: the same on a Ks axis of length 1."""
    n, Kf, Ks, Ko, Kk, Kc, Kr = f1.shape
    return np.ascontiguousarray(np.transpose(f1, (0, 1, 3, 4, 5, 2, 6))).reshape(n, Kf, Ko, Kk, Kc * Ks * Kr)


def tune_note_decoder(model, dataset, device="cuda", subset: Optional[int] = None, decoder: str = "onset", note_reference: str = "roll",
                      objective: str = "onset", cleanups=((1, 0),), tune_range=(0.05, 0.95), tune_step=0.1, tune_min_step=0.01,
                      tune_rounds=6, rank: int = 0, world: int = 1, log=print, window_overlap: Optional[float] = None, max_batch: int = 128,
                      smooth_on: float = 0.0, smooth_off: float = 0.0, smoothings=None, onset_detect: str = "edge",
                      peak_reaches=None, refine_onsets: bool = False, refine_reach: int = 2):
    """Every parameter of the note decoder at once, for the best mean note F1 (`objective`: "onset" or "onset_offset"; unweighted
    mean over samples, as note_metrics_dataset) by search_note_decoder: the thresholds of the heads that `decoder` reads ("frame":
    frame; "onset": frame, onset; "onset_offset": frame, onset, offset) times the candidates `cleanups`, a list of
    (min_note_frames, bridge_frames) pairs that takes part in every round.  The model runs once; every round is one
    notes.note_grid_counts call over each group of note_metrics_dataset, so each cell is what the single-configuration kernels count.
    -> (frame threshold, onset threshold or None, offset threshold or None, (min_note_frames, bridge_frames), best mean F1),
    identical on every rank.  A candidate threshold at or past 1 decodes no note and scores 0, as in tune_note_thresholds.
    smoothings: a list of (smooth_on, smooth_off) frame-smoothing candidates (DESIGN.md 6c "Smoothing in the decoder grid") that takes
    part in every round as `cleanups` does: the search's discrete axis is cleanups x smoothings, cleanup-major, every round still one
    note_grid_counts call per group, and the result is (frame threshold, onset threshold or None, offset threshold or None,
    (min_note_frames, bridge_frames), (smooth_on, smooth_off), best mean F1).  A single smoothing (smooth_on, smooth_off) other than
    (0, 0) is refused either way: the penalties are tuned through `smoothings`, not fixed beside the search.
    peak_reaches: a list of candidate reaches in [0, 8] of the peak-picking onset detector, 0 = the edge rule (decoder "onset" or
    "onset_offset"; DESIGN.md 6c "Peak picking in the decoder grid"), the innermost factor of the discrete axis: cleanups x smoothings x
    reaches, every round still one note_grid_counts call per group.  The result then names the detector before the best value:
    (..., (min_note_frames, bridge_frames), [(smooth_on, smooth_off),] (onset_detect, peak_reach), best mean F1), ("edge", 0) or
    ("peak", R); [R] fixes a reach while the rest is tuned.  A fixed onset_detect="peak" is refused, as a fixed smoothing is.
    refine_onsets (decoder "onset" or "onset_offset", note_reference="midi"; DESIGN.md 6c "Decoder grid in ticks"): the objective is the
    figure note_metrics_dataset(refine_onsets=True, refine_reach=...) reports -- every cell's notes with sub-frame onsets, scored in
    ticks -- and every round is one notes.note_grid_ticks_counts call per group in place of note_grid_counts; the search and the result
    are the same.  The tick grid has no smoothing axis: with `smoothings` it raises.  Without refine_onsets nothing changes."""
    from .notes import (_check_refine, _smoothing_list, check_cleanup, check_peak_reaches, check_smoothing, note_grid_counts,
                        note_grid_ticks_counts, note_prf)
    _refuse_peak("tune_note_decoder", onset_detect, reaches=True)
    if refine_onsets:
        if decoder not in ("onset", "onset_offset") or note_reference != "midi":
            raise ValueError("tune_note_decoder: refine_onsets: sub-frame onsets are read off the onset head and scored against the MIDI note "
                             "list in ticks: it needs decoder 'onset' or 'onset_offset' and note_reference='midi'")
        if smoothings is not None:
            raise ValueError("tune_note_decoder: refine_onsets cannot be combined with smoothings: the tick grid (note_grid_ticks_counts) "
                             "reads frame logits, and the packed-paths frame axis that carries the smoothing candidates is not part of it")
        _check_refine(True, refine_reach, True)
    if peak_reaches is not None:
        if decoder == "frame":
            raise ValueError("tune_note_decoder: peak_reaches needs decoder 'onset' or 'onset_offset': peaks are picked on the onset head, "
                             "and the frame decoder has none")
        reaches = [int(r) for r in check_peak_reaches(peak_reaches)]
    if smoothings is None:
        _refuse_smoothing("tune_note_decoder", smooth_on, smooth_off)
    else:
        if check_smoothing(smooth_on, smooth_off) != (0.0, 0.0):
            raise ValueError("tune_note_decoder: smooth_on / smooth_off cannot be combined with smoothings: the candidates are `smoothings`")
        smoothings = _smoothing_list(smoothings)
    if decoder not in NOTE_DECODER_AXES:
        raise ValueError(f"decoder must be 'frame', 'onset' or 'onset_offset', got {decoder!r}")
    if objective not in ("onset", "onset_offset"):
        raise ValueError(f"objective must be 'onset' or 'onset_offset', got {objective!r}")
    cleanups = [check_cleanup(*c) for c in cleanups]
    if not cleanups:
        raise ValueError("cleanups: expected at least one (min_note_frames, bridge_frames) pair")
    _check_note_reference(dataset, note_reference)
    n_axes = NOTE_DECODER_AXES[decoder]
    onset, offset = n_axes >= 2, n_axes >= 3
    n = len(dataset) if subset is None else min(subset, len(dataset))
    mine = list(shard_range(n, rank, world))
    lr = _collect(model, dataset, mine, device, window_overlap, all_heads=onset, with_offset=offset)      # the only forward passes

    def mean_f1(fts, ots, kts):
        axes = [np.asarray(t, dtype=np.float64) if t is not None else np.full(1, 0.5) for t in (fts, ots, kts)]
        if any((t <= 0.0).any() for t in axes):
            raise ValueError("tune_note_decoder: candidate thresholds must be positive (tune_range)")
        below = [np.flatnonzero(np.float32(t) < 1.0) for t in axes]
        n_disc = len(cleanups) * (1 if smoothings is None else len(smoothings)) * (1 if peak_reaches is None else len(reaches))
        shape = tuple(len(t) for t in axes) + (n_disc,)
        K = int(np.prod(shape))
        local = np.zeros((len(lr),) + shape)                                               # thresholds >= 1: no notes, F1 0
        at = 0
        if all(len(v) for v in below):
            fi, oj, kk = below
            for frame, on, ref, lengths, off in _note_groups(lr, dataset, onset, note_reference, max_batch, offset):
                if refine_onsets:
                    counts = note_grid_ticks_counts(frame, on, ref, axes[0][fi], axes[1][oj], off, axes[2][kk] if offset else None, cleanups,
                                                    None if peak_reaches is None else reaches, lengths, refine_reach)
                else:
                    counts = note_grid_counts(frame, ref, axes[0][fi], on, axes[1][oj] if onset else None, off,
                                              axes[2][kk] if offset else None, cleanups, lengths, smoothings=smoothings,
                                              peak_reaches=None if peak_reaches is None else reaches)
                f1 = np.array([m[objective][2] for m in note_prf(counts)])
                if peak_reaches is not None:
                    f1 = fold_reaches(f1.reshape(len(lengths), len(fi), 1 if smoothings is None else len(smoothings), len(oj), len(kk),
                                                 len(cleanups), len(reaches)))
                elif smoothings is None:
                    f1 = f1.reshape(len(lengths), len(fi), len(oj), len(kk), len(cleanups))
                else:
                    f1 = fold_smoothings(f1.reshape(len(lengths), len(fi), len(smoothings), len(oj), len(kk), len(cleanups)))
                local[at:at + len(lengths), fi[:, None, None], oj[None, :, None], kk[None, None, :]] = f1
                at += len(lengths)
        flat_idx = [i * K + k for i in mine for k in range(K)]
        allv = gather_values(flat_idx, local.reshape(-1).tolist(), n * K)
        return np.asarray(allv).reshape((n,) + shape).mean(axis=0) if n else np.zeros(shape)

    if peak_reaches is not None:
        smooths = [(0.0, 0.0)] if smoothings is None else smoothings
        thr, othr, kthr, d, best = search_note_decoder(mean_f1, n_axes, len(cleanups) * len(smooths) * len(reaches), tune_range, tune_step,
                                                       tune_min_step, tune_rounds, log)
        clean, smooth, reach = decoder_candidate(d, cleanups, smooths, reaches)
        detect = ("peak" if reach else "edge", reach)
        return (thr, othr, kthr, clean, detect, best) if smoothings is None else (thr, othr, kthr, clean, smooth, detect, best)
    if smoothings is None:
        thr, othr, kthr, c, best = search_note_decoder(mean_f1, n_axes, len(cleanups), tune_range, tune_step, tune_min_step, tune_rounds, log)
        return thr, othr, kthr, cleanups[c], best
    thr, othr, kthr, d, best = search_note_decoder(mean_f1, n_axes, len(cleanups) * len(smoothings), tune_range, tune_step, tune_min_step,
                                                   tune_rounds, log)
    clean, smooth = decoder_candidate(d, cleanups, smoothings)
    return thr, othr, kthr, clean, smooth, best
