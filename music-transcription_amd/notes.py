"""Note-level evaluation and onset-gated note decoding on the GPU (csrc/notes.hip; DESIGN.md "Note-level F1").

  * `note_match_counts` = the counting half of mir_eval.transcription.precision_recall_f1_overlap on the 32 ms frame grid, for a
    batch of pitch rolls in one pass over the logits: per sample {n_ref, n_est, tp_onset, tp_onset_offset}.  Reference notes are
    the runs of the label roll; estimated notes come from the frame decoder (runs of sigmoid(frame) > threshold, as
    mt_roll_to_notes) or, given onset logits, from the onset-gated decoder.
  * `note_match_list` = the same counts against a note list in ticks of 100 us (the MIDI notes of MaestroDataset.ref_notes), in
    which re-struck keys are notes of their own: mir_eval's criteria in integers, a maximum matching per criterion.
  * `note_prf` turns those counts into precision / recall / F1 on the host (0 for an empty denominator, as mir_eval).
  * `heads_to_notes_device` = transcribe.notes_from_logits_device with the onset-gated decoder (mt_heads_to_notes).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr

SR, HOP = 16000, 512
FS = SR / HOP                      # frames per second of the model's grid (one frame = 32 ms)


def _rows(x: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA tensor")
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise ValueError(f"{name}: expected (B, P, T) or (P, T), got {tuple(x.shape)}")
    return x.detach().float().contiguous()


def _check_threshold(t: float, name: str) -> float:
    t = float(t)
    if not 0.0 < t < 1.0:
        raise ValueError(f"{name} must lie in (0, 1), got {t}")
    return t


def note_match_counts(frame_logits: torch.Tensor, ref_roll: torch.Tensor, threshold: float = 0.5, onset_logits: Optional[torch.Tensor] = None,
                      onset_threshold: float = 0.5, lengths=None) -> torch.Tensor:
    """(B, P, T) frame logits (and onset logits for the onset-gated decoder) and (B, P, T) reference roll on the device -> (B, 4)
    int64 device tensor {n_ref, n_est, tp_onset, tp_onset_offset}.  lengths (B,) = valid frames per sample (None: all T)."""
    x = _rows(frame_logits, "frame_logits")
    ref = _rows(ref_roll, "ref_roll")
    on = None if onset_logits is None else _rows(onset_logits, "onset_logits")
    if ref.shape != x.shape or (on is not None and on.shape != x.shape):
        raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, ref {tuple(ref.shape)}, onset {None if on is None else tuple(on.shape)}")
    thr = _check_threshold(threshold, "threshold")
    othr = _check_threshold(onset_threshold, "onset_threshold") if on is not None else 0.5
    B, P, T = x.shape
    dev = x.device
    ln = None
    if lengths is not None:
        ln = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(dev).contiguous()
        if ln.numel() != B:
            raise ValueError(f"lengths has {ln.numel()} entries for a batch of {B}")
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.mt_note_match_counts(ptr(x), ptr(on), thr, othr, ptr(ref), ptr(ln), ptr(counts), B, P, T, _lib.stream_ptr()),
              "mt_note_match_counts")
    return counts


TICKS_PER_FRAME = 320              # one frame in ticks of 100 us


def note_match_list(frame_logits: torch.Tensor, ref_notes: Dict[str, torch.Tensor], threshold: float = 0.5,
                    onset_logits: Optional[torch.Tensor] = None, onset_threshold: float = 0.5, lengths=None) -> torch.Tensor:
    """note_match_counts against a note list: ref_notes = {"on", "off"} int32 ticks of 100 us and "ptr" int64 (B * P + 1,) on the
    device, row (b, p) owning on/off[ptr[b*P + p]:ptr[b*P + p + 1]] sorted by onset (MaestroDataset.ref_notes).  An estimated
    note [s, e) in frames has times 320 s, 320 e; onsets match within 500 ticks, offsets within max(500, 0.2 reference length).
    Notes that start at or past a sample's valid frames are not counted.  -> (B, 4) int64 {n_ref, n_est, tp_onset, tp_onset_offset}."""
    x = _rows(frame_logits, "frame_logits")
    on = None if onset_logits is None else _rows(onset_logits, "onset_logits")
    if on is not None and on.shape != x.shape:
        raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, onset {tuple(on.shape)}")
    thr = _check_threshold(threshold, "threshold")
    othr = _check_threshold(onset_threshold, "onset_threshold") if on is not None else 0.5
    B, P, T = x.shape
    dev = x.device
    r_on, r_off, r_ptr = (ref_notes[k] for k in ("on", "off", "ptr"))
    for t, dt, name in ((r_on, torch.int32, "on"), (r_off, torch.int32, "off"), (r_ptr, torch.int64, "ptr")):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"ref_notes[{name!r}]: expected a 1-d {dt} tensor on {dev}")
    if r_ptr.numel() != B * P + 1 or r_on.numel() != r_off.numel():
        raise ValueError(f"ref_notes: ptr has {r_ptr.numel()} entries for {B} x {P} rows, on / off have {r_on.numel()} / {r_off.numel()}")
    # the kernel indexes on / off through ptr: refuse a table that points outside them (one small read-back, evaluation only)
    bad = (r_ptr[0] != 0) | (r_ptr[-1] != r_on.numel()) | (r_ptr[1:] < r_ptr[:-1]).any()
    if bool(bad):
        raise ValueError("ref_notes: ptr must rise from 0 to the number of notes")
    if r_on.numel() == 0:                                   # no notes at all: the kernel still wants readable tables
        r_on = r_off = torch.zeros(1, dtype=torch.int32, device=dev)
    ln = None
    if lengths is not None:
        ln = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(dev).contiguous()
        if ln.numel() != B:
            raise ValueError(f"lengths has {ln.numel()} entries for a batch of {B}")
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.mt_note_match_list(ptr(x), ptr(on), thr, othr, ptr(r_on.contiguous()), ptr(r_off.contiguous()), ptr(r_ptr.contiguous()),
                                     ptr(ln), ptr(counts), B, P, T, _lib.stream_ptr()), "mt_note_match_list")
    return counts


def _prf(tp: int, n_ref: int, n_est: int) -> Tuple[float, float, float]:
    p = tp / n_est if n_est else 0.0
    r = tp / n_ref if n_ref else 0.0
    f = 2.0 * tp / (n_ref + n_est) if (n_ref + n_est) else 0.0
    return p, r, f


def note_prf(counts) -> List[Dict[str, Tuple[float, float, float]]]:
    """(B, 4) counts -> per sample {"onset": (P, R, F1), "onset_offset": (P, R, F1)}."""
    c = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    c = np.asarray(c, dtype=np.int64).reshape(-1, 4)
    return [{"onset": _prf(int(tp_on), int(n_ref), int(n_est)), "onset_offset": _prf(int(tp_onoff), int(n_ref), int(n_est))}
            for n_ref, n_est, tp_on, tp_onoff in c]


def heads_to_notes_device(frame_logits: torch.Tensor, onset_logits: torch.Tensor, threshold: float = 0.5, onset_threshold: float = 0.5,
                          fs: float = FS, min_midi: int = 21) -> List[Tuple[int, float, float]]:
    """(n_chunks, 88, T) frame and onset logits ON THE DEVICE -> notes of the onset-gated decoder over the chunks concatenated in
    time, in the reference's note order (pitch-major, then time); only counts and two ints per note reach the host."""
    x = _rows(frame_logits, "frame_logits")
    on = _rows(onset_logits, "onset_logits")
    if on.shape != x.shape:
        raise ValueError(f"frame {tuple(x.shape)} and onset {tuple(on.shape)} logits differ in shape")
    thr, othr = _check_threshold(threshold, "threshold"), _check_threshold(onset_threshold, "onset_threshold")
    NB, P, T = x.shape
    dev = x.device
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    cap = max(1024, NB * 64)
    while True:
        starts, ends = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib.mt_heads_to_notes(ptr(x), ptr(on), thr, othr, NB, P, T, ptr(counts), ptr(starts), ptr(ends), cap, _lib.stream_ptr()),
                  "mt_heads_to_notes")
        c = counts.cpu().numpy()
        total = int(c.sum())
        if total <= cap:
            break
        cap = total
    s, e = starts[:total].cpu().numpy(), ends[:total].cpu().numpy()
    pitches = np.repeat(np.arange(P) + min_midi, c)
    return [(int(pp), float(a) / fs, float(b) / fs) for pp, a, b in zip(pitches, s, e)]
