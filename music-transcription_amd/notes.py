"""Note-level evaluation and onset-gated note decoding on the GPU (csrc/notes.hip; DESIGN.md "Note-level F1").

  * `note_match_counts` = the counting half of mir_eval.transcription.precision_recall_f1_overlap on the 32 ms frame grid, for a
    batch of pitch rolls in one pass over the logits: per sample {n_ref, n_est, tp_onset, tp_onset_offset}.  Reference notes are
    the runs of the label roll; estimated notes come from the frame decoder (runs of sigmoid(frame) > threshold, as
    mt_roll_to_notes) or, given onset logits, from the onset-gated decoder.
  * `note_match_list` = the same counts against a note list in ticks of 100 us (the MIDI notes of MaestroDataset.ref_notes), in
    which re-struck keys are notes of their own: mir_eval's criteria in integers, a maximum matching per criterion.
  * `note_sweep_counts` = either of them for a whole grid of (frame, onset) thresholds in one pass over the logits
    (mt_note_sweep_counts / mt_note_sweep_list): every cell's sigmoid is evaluated once, whatever the size of the grid.
  * `note_grid_counts` = either of them for a grid of every decoder parameter -- frame, onset and offset thresholds times a list of
    cleanup pairs, any of the three decoders -- in one pass over the logits (mt_note_grid_counts / mt_note_grid_list).
  * `note_prf` turns those counts into precision / recall / F1 on the host (0 for an empty denominator, as mir_eval).
  * `heads_to_notes_device` = transcribe.notes_from_logits_device with the onset-gated decoder (mt_heads_to_notes).
  * `offset_logits=` on the three calls above selects the offset-gated decoder: the onset-gated notes, ended where
    the offset head fires (mt_note_match_counts_off / mt_note_match_list_off / mt_heads_to_notes_off).
  * `notes_batch_device` = either decoder over a padded batch of whole recordings with `lengths` (mt_notes_batch): the notes of all
    recordings in two device-to-host copies.
  * `min_note_frames=`, `bridge_frames=` on the two matchers and the two note-list calls = note cleanup inside the decoder
    (DESIGN.md 6c "Note cleanup"; the mt_*_clean kernels): gaps of the activity of at most bridge_frames are bridged before decoding, notes
    shorter than min_note_frames dropped after it.  (1, 0) is no cleanup and calls exactly the entry points above.
  * `smooth_frame_logits` = the frame head of every pitch row replaced by the Viterbi path of a two-state HMM, as logits of +-64
    (DESIGN.md 6c "Frame smoothing"; mt_frame_smooth / mt_frame_smooth_chunks).  `smooth_on=`, `smooth_off=` (switching penalties in
    logits) on the two matchers and the two note-list calls smooth the frame head first and then proceed as above; the onset and
    offset heads are edge detectors and stay as they are.  (0, 0) is no smoothing and launches nothing.
  * `smooth_frame_paths` = those paths for up to 16 (threshold, on, off) candidates per launch, packed 64 frames to a word
    (mt_frame_smooth_paths), and `smoothings=` on `note_grid_counts` = a list of penalty pairs as one more axis of the grid, which
    then reads such words as its frame axis (mt_note_grid_counts_paths / mt_note_grid_list_paths; DESIGN.md 6c "Smoothing in the
    decoder grid").
  * `refine_onsets_device` = sub-frame onsets in ticks of 100 us for the notes of any onset-gated decoder, from the three onset-head values
    around the peak near each note's start (mt_refine_onsets; DESIGN.md 6c "Sub-frame onsets"); `refine_onsets=` on the two note-list
    calls stamps the notes with them.  `note_match_ticks_device` scores such off-grid estimates against a note list on the device
    (mt_note_match_ticks: a maximum matching per pitch row, one wave per row, one lane per connected component), from the device
    tables of `notes_ticks_tables_device`; `note_match_ticks` is the same on the host, and the specification of the kernel.
  * `onset_detect="peak"`, `peak_reach=R` on the two matchers and the note-list calls = a note opens at every local maximum of the
    onset logits over R frames that passes the onset threshold, not at the rising edges of the thresholded onset mask (DESIGN.md 6c
    "Peak-picked onsets"; the mt_*_peak entry points): the detector for an onset head trained against triangular targets, on which
    the edge rule merges re-struck keys.  "edge" calls exactly the entry points above.  The sweep kernel has no peak mode.
  * `peak_reaches=` on `note_grid_counts` = a list of candidate reaches as the grid's last axis, 0 = the edge rule, so one pass scores
    both detectors (the mt_note_grid_*_peak entry points; DESIGN.md 6c "Peak picking in the decoder grid").
  * `note_grid_ticks_counts` = the counts of `notes_ticks_tables_device` + `note_match_ticks_device` -- refined onsets, scored in ticks --
    at every cell of such a grid: one launch pair decodes every cell into its refined note list (`notes_grid_ticks_tables_device`,
    mt_notes_grid_ticks) and one launch scores all of them (`note_match_ticks_cells_device`, mt_note_match_ticks_cells); DESIGN.md 6c
    "Decoder grid in ticks".
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence, Tuple

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


def _heads(frame_logits, onset_logits, offset_logits, threshold, onset_threshold, offset_threshold, onset_required=False, ref_roll=None,
           mismatch="shape mismatch: frame {frame}, onset {onset}"):
    """The checked heads of a decoder call -> (x, on, off, thr, othr, kthr, ref): the contiguous (B, P, T) logits (on / off None
    without them), their thresholds (0.5 for an absent head) and the reference roll (None without ref_roll).  The offset-gated
    decoder opens its notes at onset edges, so offset logits without onset logits are refused before anything else; then shapes,
    then thresholds.  `mismatch` is the calling function's own message for logits that differ in shape."""
    if offset_logits is not None and onset_logits is None:
        raise ValueError("offset_logits: the offset-gated decoder needs onset_logits as well")
    x = _rows(frame_logits, "frame_logits")
    ref = None if ref_roll is None else _rows(ref_roll, "ref_roll")
    on = _rows(onset_logits, "onset_logits") if onset_required or onset_logits is not None else None
    if (ref is not None and ref.shape != x.shape) or (on is not None and on.shape != x.shape):
        shapes = {"frame": tuple(x.shape), "ref": None if ref is None else tuple(ref.shape), "onset": None if on is None else tuple(on.shape)}
        raise ValueError(mismatch.format(**shapes))
    thr = _check_threshold(threshold, "threshold")
    othr = _check_threshold(onset_threshold, "onset_threshold") if on is not None else 0.5
    if offset_logits is None:
        return x, on, None, thr, othr, 0.5, ref
    off = _rows(offset_logits, "offset_logits")
    if off.shape != x.shape:
        raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, offset {tuple(off.shape)}")
    return x, on, off, thr, othr, _check_threshold(offset_threshold, "offset_threshold"), ref


MAX_MIN_NOTE_FRAMES, MAX_BRIDGE_FRAMES = 64, 63     # CLEAN_MAX_* of csrc/note_decode.h: both stages look one 64-frame window ahead
FRAME_MS = 1000.0 * HOP / SR                        # 32 ms


def check_cleanup(min_note_frames=1, bridge_frames=0) -> Tuple[int, int]:
    """The checked (min_note_frames, bridge_frames) of a decoder call; (1, 0) = no cleanup.  Raises before any GPU work."""
    m, g = min_note_frames, bridge_frames
    for v, name in ((m, "min_note_frames"), (g, "bridge_frames")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer number of frames, got {v!r}")
    if not 1 <= m <= MAX_MIN_NOTE_FRAMES:
        raise ValueError(f"min_note_frames must lie in [1, {MAX_MIN_NOTE_FRAMES}], got {m}")
    if not 0 <= g <= MAX_BRIDGE_FRAMES:
        raise ValueError(f"bridge_frames must lie in [0, {MAX_BRIDGE_FRAMES}], got {g}")
    return int(m), int(g)


def cleanup_frames(min_note_ms: float = 0.0, bridge_gap_ms: float = 0.0) -> Tuple[int, int]:
    """Milliseconds -> (min_note_frames, bridge_frames) on the 32 ms grid, exactly: a note is dropped iff it is shorter than
    min_note_ms (M = max(1, ceil(ms / 32))) and a gap bridged iff it is no longer than bridge_gap_ms (G = floor(ms / 32))."""
    from fractions import Fraction
    out = []
    for ms, name in ((min_note_ms, "min_note_ms"), (bridge_gap_ms, "bridge_gap_ms")):
        if isinstance(ms, bool) or not isinstance(ms, (int, float, np.integer, np.floating)) or not np.isfinite(ms) or ms < 0:
            raise ValueError(f"{name} must be a finite number of milliseconds >= 0, got {ms!r}")
        out.append(Fraction(ms) / Fraction(FRAME_MS))                       # (exact: a float is a fraction)
    m, g = max(1, int(np.ceil(out[0]))), int(np.floor(out[1]))
    if m > MAX_MIN_NOTE_FRAMES:
        raise ValueError(f"min_note_ms must be at most {MAX_MIN_NOTE_FRAMES * FRAME_MS:g} ms ({MAX_MIN_NOTE_FRAMES} frames of "
                         f"{FRAME_MS:g} ms), got {min_note_ms}")
    if g > MAX_BRIDGE_FRAMES:
        raise ValueError(f"bridge_gap_ms must be below {(MAX_BRIDGE_FRAMES + 1) * FRAME_MS:g} ms (at most {MAX_BRIDGE_FRAMES} frames of "
                         f"{FRAME_MS:g} ms), got {bridge_gap_ms}")
    return m, g


MAX_PEAK_REACH = 8                                  # PEAK_MAX_REACH of csrc/note_decode.h
ONSET_DETECTORS = ("edge", "peak")


def check_onset_detect(onset_detect="edge", peak_reach=1, has_onset: bool = True) -> int:
    """The checked onset detector of a decoder call -> 0 for "edge" (the rising edges of the onset mask), the reach R in [1, 8] for
    "peak" (the local maxima of the onset logits over R frames; DESIGN.md 6c "Peak-picked onsets").  has_onset: the call has an onset
    head; "peak" without one is refused.  Raises before any GPU work."""
    if onset_detect not in ONSET_DETECTORS:
        raise ValueError(f"onset_detect must be one of {ONSET_DETECTORS}, got {onset_detect!r}")
    if isinstance(peak_reach, bool) or not isinstance(peak_reach, (int, np.integer)) or not 1 <= peak_reach <= MAX_PEAK_REACH:
        raise ValueError(f"peak_reach must be an integer number of frames in [1, {MAX_PEAK_REACH}], got {peak_reach!r}")
    if onset_detect == "edge":
        return 0
    if not has_onset:
        raise ValueError("onset_detect='peak': peaks are picked on the onset head, and the frame decoder has none (pass onset_logits)")
    return int(peak_reach)


def refuse_peak(onset_detect, who: str, reaches: bool = False) -> None:
    """The calls that run the sweep and grid kernels take onset_detect only to refuse "peak": the sweep kernel has no peak mode, and the
    grid's is an axis of candidate reaches (reaches=True: the call has a peak_reaches= argument, which the message names)."""
    if check_onset_detect(onset_detect):
        raise ValueError(f"{who}: onset_detect='peak' is not supported here: peak detection inside the sweep and grid kernels is out of "
                         "scope (they decode with the edge rule only); tune with 'edge' or score single configurations"
                         + ("; peak_reaches= is the way in: a list of candidate reaches as one more axis of the grid, 0 = the edge rule"
                            if reaches else ""))


def check_peak_reaches(peak_reaches, has_onset: bool = True) -> np.ndarray:
    """The checked candidate reaches of a decoder grid -> int32 array: a non-empty list of integers in [0, 8], 0 = the edge rule, R >= 1 =
    onset_detect="peak" at peak_reach=R (DESIGN.md 6c "Peak picking in the decoder grid").  Raises before any GPU work."""
    if isinstance(peak_reaches, (str, bytes)) or not hasattr(peak_reaches, "__len__") or len(peak_reaches) == 0:
        raise ValueError(f"peak_reaches: expected a non-empty list of reaches in [0, {MAX_PEAK_REACH}], got {peak_reaches!r}")
    for r in peak_reaches:
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r <= MAX_PEAK_REACH:
            raise ValueError(f"peak_reaches: a reach is an integer number of frames in [0, {MAX_PEAK_REACH}] (0 = the edge rule), got {r!r}")
    if not has_onset:
        raise ValueError("peak_reaches: peaks are picked on the onset head, and the frame decoder has none (pass onset_logits)")
    return np.asarray([int(r) for r in peak_reaches], dtype=np.int32)


MAX_SMOOTH_PENALTY = 64.0                           # logits; csrc/smooth.hip counts evidence in steps of 1/64 logit, capped at +-64 logits


def check_smoothing(smooth_on=0.0, smooth_off=0.0) -> Tuple[float, float]:
    """The checked (smooth_on, smooth_off) of a decoder call: the penalties, in logits, that the frame smoothing charges for switching
    a pitch on and off; (0, 0) = no smoothing.  Raises before any GPU work."""
    out = []
    for v, name in ((smooth_on, "smooth_on"), (smooth_off, "smooth_off")):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(np.float32(v)) <= MAX_SMOOTH_PENALTY:
            raise ValueError(f"{name} must be a penalty of 0 to {MAX_SMOOTH_PENALTY:g} logits, got {v!r}")
        out.append(float(np.float32(v)))
    return out[0], out[1]


def _decode(family: str, clean: Tuple[int, int], x, on, off, thrs, rest, offset_head: bool = True, peak: int = 0) -> None:
    """Call the entry point of `family` (mt_note_match_counts, mt_note_match_list, mt_heads_to_notes, mt_notes_batch) that serves a
    decoder call: `family` itself or, with offset logits, `family`_off at no cleanup (1, 0), `family`_clean otherwise.  thrs = the
    (frame, onset, offset) thresholds, rest = the arguments after the heads and thresholds, the stream last (the cleanup goes before
    it).  offset_head=False: a family without an offset head, whose _clean takes two heads as well.  peak = check_onset_detect's
    result: other than 0, `family`_peak at that reach, whatever the cleanup (its arguments are _clean's, the reach before the stream)."""
    two, three = (ptr(x), ptr(on), *thrs[:2]), (ptr(x), ptr(on), ptr(off), *thrs)
    if peak:
        name, args = family + "_peak", (*(three if offset_head else two), *rest[:-1], *clean, peak, rest[-1])
    elif clean != (1, 0):
        name, args = family + "_clean", (*(three if offset_head else two), *rest[:-1], *clean, rest[-1])
    elif off is None:
        name, args = family, (*two, *rest)
    else:
        name, args = family + "_off", (*three, *rest)
    check(getattr(lib, name)(*args), name)


def _lengths(lengths, B: int, dev) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    ln = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).to(dev).contiguous()
    if ln.numel() != B:
        raise ValueError(f"lengths has {ln.numel()} entries for a batch of {B}")
    return ln


SMOOTH_SPLIT_WAVES = (2, 16)                        # mt_frame_smooth_split / mt_frame_smooth_chunks_split: waves per row


def _smoothed(x: torch.Tensor, thr: float, smooth: Tuple[float, float], ln: Optional[torch.Tensor], chunks: bool,
              waves: Optional[int] = None) -> torch.Tensor:
    """The checked, contiguous (B, P, T) frame logits x smoothed into a new tensor; frames at or past a row's length are not written
    (they hold x's values when there are lengths).  waves None: the library picks its kernel; an integer: the _split entry points."""
    B, P, T = x.shape
    out = torch.empty_like(x) if ln is None else x.clone()
    with torch.cuda.device(x.device):
        if waves is not None and chunks:
            check(lib.mt_frame_smooth_chunks_split(ptr(x), ptr(out), thr, *smooth, B, P, T, waves, _lib.stream_ptr()), "mt_frame_smooth_chunks_split")
        elif waves is not None:
            check(lib.mt_frame_smooth_split(ptr(x), ptr(out), thr, *smooth, ptr(ln), B, P, T, waves, _lib.stream_ptr()), "mt_frame_smooth_split")
        elif chunks:
            check(lib.mt_frame_smooth_chunks(ptr(x), ptr(out), thr, *smooth, B, P, T, _lib.stream_ptr()), "mt_frame_smooth_chunks")
        else:
            check(lib.mt_frame_smooth(ptr(x), ptr(out), thr, *smooth, ptr(ln), B, P, T, _lib.stream_ptr()), "mt_frame_smooth")
    return out


def smooth_frame_logits(frame_logits: torch.Tensor, threshold: float = 0.5, on_penalty: float = 0.0, off_penalty: float = 0.0, lengths=None,
                        chunks: bool = False, waves: Optional[int] = None) -> torch.Tensor:
    """(B, P, T) or (P, T) frame logits ON THE DEVICE -> a float tensor of the same shape that holds, per pitch row, the Viterbi path
    of a two-state (off / on) HMM as logits: +64 where the path is on, -64 where it is off (DESIGN.md 6c "Frame smoothing").  The
    evidence of a frame is its logit minus logit(threshold); switching on costs on_penalty, switching off off_penalty (logits, 0 to
    64), so a blip survives only if its evidence pays for both and a dropout is bridged only if its counter-evidence is smaller than
    both.  Every consumer of frame logits reads the path from the result at any threshold.  lengths (B,): valid frames per row of the
    batch (None: all T); frames past them keep the input's values.  chunks=True: the B chunks are one recording of B * T frames per
    pitch, as heads_to_notes_device concatenates them (no lengths then).  (0, 0) returns frame_logits itself and launches nothing.
    waves: None lets the library choose between one wave64 per row and several (DESIGN.md 6c "Long rows: segments per wave"); an
    integer in [2, 16] asks for that many through mt_frame_smooth_split / mt_frame_smooth_chunks_split.  The same bits either way."""
    smooth = check_smoothing(on_penalty, off_penalty)
    thr = _check_threshold(threshold, "threshold")
    if waves is not None and (isinstance(waves, bool) or not isinstance(waves, (int, np.integer))
                              or not SMOOTH_SPLIT_WAVES[0] <= waves <= SMOOTH_SPLIT_WAVES[1]):
        raise ValueError(f"waves must be None or an integer in [{SMOOTH_SPLIT_WAVES[0]}, {SMOOTH_SPLIT_WAVES[1]}], got {waves!r}")
    if chunks and lengths is not None:
        raise ValueError("lengths: chunks=True concatenates whole chunks, which have no lengths")
    if smooth == (0.0, 0.0):
        return frame_logits
    x = _rows(frame_logits, "frame_logits")
    return _smoothed(x, thr, smooth, _lengths(lengths, x.shape[0], x.device), chunks,
                     None if waves is None else int(waves)).reshape(frame_logits.shape)


SMOOTH_MAX_K = 16                                   # mt_frame_smooth_paths: candidates per call


def _smoothing_list(smoothings) -> List[Tuple[float, float]]:
    """The checked, non-empty list of (on, off) penalty pairs of a smoothing axis."""
    try:
        pairs = [tuple(s) for s in smoothings]
    except TypeError:
        raise ValueError(f"smoothings: expected a list of (smooth_on, smooth_off) pairs, got {smoothings!r}") from None
    if not pairs or any(len(s) != 2 for s in pairs):
        raise ValueError("smoothings: expected a non-empty list of (smooth_on, smooth_off) pairs")
    return [check_smoothing(*s) for s in pairs]


def _paths(x: torch.Tensor, thr: np.ndarray, pairs: Sequence[Tuple[float, float]], ln: Optional[torch.Tensor]) -> torch.Tensor:
    """mt_frame_smooth_paths on checked arguments: x contiguous (B, P, T), thr float32 (K,), K = len(pairs) <= 16 -> (K, B, P, W) int64."""
    B, P, T = x.shape
    K = len(pairs)
    out = torch.empty(2, K, B, P, (T + 63) // 64, dtype=torch.int64, device=x.device)          # paths | the kernel's scratch
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    on, off = (np.ascontiguousarray([s[i] for s in pairs], dtype=np.float32) for i in (0, 1))
    with torch.cuda.device(x.device):
        check(lib.mt_frame_smooth_paths(ptr(x), thr.ctypes.data, on.ctypes.data, off.ctypes.data, K, ptr(ln), B, P, T, ptr(out[0]), ptr(out[1]),
                                        _lib.stream_ptr()), "mt_frame_smooth_paths")
    return out[0]


def smooth_frame_paths(frame_logits: torch.Tensor, thresholds, smoothings, lengths=None) -> torch.Tensor:
    """(B, P, T) or (P, T) frame logits ON THE DEVICE -> (K, B, P, W) int64 device tensor, W = ceil(T / 64): the Viterbi paths of
    smooth_frame_logits for K candidates at once, packed 64 frames to a word (mt_frame_smooth_paths; DESIGN.md 6c "Smoothing in the
    decoder grid").  Bit l of [k, b, p, w] is 1 iff smooth_frame_logits at (thresholds[k], *smoothings[k]) is +64 at frame 64 w + l;
    bits at or past a sample's length are 0.  smoothings: a list of (on, off) penalty pairs as check_smoothing takes them; thresholds:
    one value for all of them or one value per pair.  (0, 0) goes through the kernel as any other pair: its path is the thresholded
    activity.  More than 16 candidates are cut into several launches.  The kernel's scratch (as large as the result) is allocated here."""
    pairs = _smoothing_list(smoothings)
    thr = _threshold_array(thresholds, "thresholds")
    if len(thr) == 1:
        thr = np.repeat(thr, len(pairs))
    if len(thr) != len(pairs):
        raise ValueError(f"thresholds: expected one value or one per pair of smoothings, got {len(thr)} for {len(pairs)}")
    x = _rows(frame_logits, "frame_logits")
    ln = _lengths(lengths, x.shape[0], x.device)
    tiles = [_paths(x, thr[k0:k0 + SMOOTH_MAX_K], pairs[k0:k0 + SMOOTH_MAX_K], ln) for k0 in range(0, len(pairs), SMOOTH_MAX_K)]
    return tiles[0] if len(tiles) == 1 else torch.cat(tiles)


def _note_tables(ref_notes: Dict[str, torch.Tensor], B: int, P: int, dev, who: str = "ref_notes", sorted_rows: bool = False):
    """The checked, contiguous (on, off, ptr) of a note list for B x P rows.  sorted_rows: `on` must also be non-decreasing inside
    every row (checked on the device, in the same read-back as ptr)."""
    r_on, r_off, r_ptr = (ref_notes[k] for k in ("on", "off", "ptr"))
    for t, dt, name in ((r_on, torch.int32, "on"), (r_off, torch.int32, "off"), (r_ptr, torch.int64, "ptr")):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{who}[{name!r}]: expected a 1-d {dt} tensor on {dev}")
    n = r_on.numel()
    if r_ptr.numel() != B * P + 1 or n != r_off.numel():
        raise ValueError(f"{who}: ptr has {r_ptr.numel()} entries for {B} x {P} rows, on / off have {n} / {r_off.numel()}")
    # the kernel indexes on / off through ptr: refuse a table that points outside them (one small read-back, evaluation only)
    bad = (r_ptr[0] != 0) | (r_ptr[-1] != n) | (r_ptr[1:] < r_ptr[:-1]).any()
    if sorted_rows and n > 1:
        first = torch.zeros(n + 1, dtype=torch.bool, device=dev)       # a row's first note may lie before its predecessor
        first[r_ptr[:-1].clamp(0, n)] = True                           # (clamped: ptr is not known to be good yet; n = an empty last row)
        bad = bad.to(torch.int32) + 2 * ((r_on[1:] < r_on[:-1]) & ~first[1:n]).any()
    bad = int(bad)
    if bad & 1:
        raise ValueError(f"{who}: ptr must rise from 0 to the number of notes")
    if bad:
        raise ValueError(f"{who}: on must be non-decreasing inside every row")
    if n == 0:                                              # no notes at all: the kernel still wants readable tables
        r_on = r_off = torch.zeros(1, dtype=torch.int32, device=dev)
    return r_on.contiguous(), r_off.contiguous(), r_ptr.contiguous()


def note_match_counts(frame_logits: torch.Tensor, ref_roll: torch.Tensor, threshold: float = 0.5, onset_logits: Optional[torch.Tensor] = None,
                      onset_threshold: float = 0.5, lengths=None, offset_logits: Optional[torch.Tensor] = None,
                      offset_threshold: float = 0.5, min_note_frames: int = 1, bridge_frames: int = 0, smooth_on: float = 0.0,
                      smooth_off: float = 0.0, onset_detect: str = "edge", peak_reach: int = 1) -> torch.Tensor:
    """(B, P, T) frame logits (and onset logits for the onset-gated decoder) and (B, P, T) reference roll on the device -> (B, 4)
    int64 device tensor {n_ref, n_est, tp_onset, tp_onset_offset}.  lengths (B,) = valid frames per sample (None: all T).  With
    offset_logits (and onset_logits) the estimates come from the offset-gated decoder (mt_note_match_counts_off).  With
    (min_note_frames, bridge_frames) other than (1, 0) the estimates are cleaned in the decoder (mt_note_match_counts_clean).  With
    (smooth_on, smooth_off) other than (0, 0) the frame head is smoothed first (smooth_frame_logits, over the same lengths).
    onset_detect="peak" (needs onset_logits): notes open at the peaks of the onset logits over peak_reach frames
    (mt_note_match_counts_peak; DESIGN.md 6c "Peak-picked onsets")."""
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    peak = check_onset_detect(onset_detect, peak_reach, onset_logits is not None)
    x, on, off, thr, othr, kthr, ref = _heads(frame_logits, onset_logits, offset_logits, threshold, onset_threshold, offset_threshold,
                                              ref_roll=ref_roll, mismatch="shape mismatch: frame {frame}, ref {ref}, onset {onset}")
    B, P, T = x.shape
    dev = x.device
    ln = _lengths(lengths, B, dev)
    if smooth != (0.0, 0.0):
        x = _smoothed(x, thr, smooth, ln, False)
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _decode("mt_note_match_counts", clean, x, on, off, (thr, othr, kthr), (ptr(ref), ptr(ln), ptr(counts), B, P, T, _lib.stream_ptr()),
                peak=peak)
    return counts


TICKS_PER_FRAME = 320              # one frame in ticks of 100 us


def note_match_list(frame_logits: torch.Tensor, ref_notes: Dict[str, torch.Tensor], threshold: float = 0.5,
                    onset_logits: Optional[torch.Tensor] = None, onset_threshold: float = 0.5, lengths=None,
                    offset_logits: Optional[torch.Tensor] = None, offset_threshold: float = 0.5, min_note_frames: int = 1,
                    bridge_frames: int = 0, smooth_on: float = 0.0, smooth_off: float = 0.0, onset_detect: str = "edge",
                    peak_reach: int = 1) -> torch.Tensor:
    """note_match_counts against a note list: ref_notes = {"on", "off"} int32 ticks of 100 us and "ptr" int64 (B * P + 1,) on the
    device, row (b, p) owning on/off[ptr[b*P + p]:ptr[b*P + p + 1]] sorted by onset (MaestroDataset.ref_notes).  An estimated
    note [s, e) in frames has times 320 s, 320 e; onsets match within 500 ticks, offsets within max(500, 0.2 reference length).
    Notes that start at or past a sample's valid frames are not counted.  -> (B, 4) int64 {n_ref, n_est, tp_onset, tp_onset_offset}.
    With offset_logits (and onset_logits) the estimates come from the offset-gated decoder (mt_note_match_list_off); with
    (min_note_frames, bridge_frames) other than (1, 0) they are cleaned in the decoder (mt_note_match_list_clean); with
    (smooth_on, smooth_off) other than (0, 0) the frame head is smoothed first (smooth_frame_logits, over the same lengths);
    with onset_detect="peak" (needs onset_logits) notes open at the peaks of the onset logits over peak_reach frames
    (mt_note_match_list_peak)."""
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    peak = check_onset_detect(onset_detect, peak_reach, onset_logits is not None)
    x, on, off, thr, othr, kthr, _ = _heads(frame_logits, onset_logits, offset_logits, threshold, onset_threshold, offset_threshold)
    B, P, T = x.shape
    dev = x.device
    r_on, r_off, r_ptr = _note_tables(ref_notes, B, P, dev)
    ln = _lengths(lengths, B, dev)
    if smooth != (0.0, 0.0):
        x = _smoothed(x, thr, smooth, ln, False)
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _decode("mt_note_match_list", clean, x, on, off, (thr, othr, kthr),
                (ptr(r_on), ptr(r_off), ptr(r_ptr), ptr(ln), ptr(counts), B, P, T, _lib.stream_ptr()), peak=peak)
    return counts


SWEEP_MAX_K, SWEEP_MAX_PAIRS = 16, 64              # mt_note_sweep_*: thresholds per axis, pairs per call


def _threshold_array(values, name: str) -> np.ndarray:
    a = np.atleast_1d(np.asarray(values, dtype=np.float64)).astype(np.float32)
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"{name}: expected a non-empty 1-d list of thresholds")
    for t in a:
        _check_threshold(t, name)
    return a


def note_sweep_counts(frame_logits: torch.Tensor, ref, thresholds, onset_logits: Optional[torch.Tensor] = None, onset_thresholds=None,
                      lengths=None, onset_detect: str = "edge") -> torch.Tensor:
    """note_match_counts (ref = a (B, P, T) roll) or note_match_list (ref = the {"on", "off", "ptr"} note list) at every pair of
    `thresholds` x `onset_thresholds` -> (B, Kf, Ko, 4) int64 device tensor; [b, i, j] is exactly what the single call returns at
    (thresholds[i], onset_thresholds[j]).  Without onset logits (the frame decoder) Ko = 1 and onset_thresholds is not read.  The
    logits are read, and their sigmoids evaluated, once per call of the kernel; a grid past its limits (16 per axis, 64 pairs) is
    cut into several calls here.  Nothing is allocated on the device but the result, and with a roll nothing synchronises (a note
    list's ptr table is checked with one small read-back, as in note_match_list).  onset_detect: "edge" only; the sweep kernel has no
    peak mode and "peak" raises."""
    refuse_peak(onset_detect, "note_sweep_counts")
    x = _rows(frame_logits, "frame_logits")
    on = None if onset_logits is None else _rows(onset_logits, "onset_logits")
    if on is not None and on.shape != x.shape:
        raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, onset {tuple(on.shape)}")
    B, P, T = x.shape
    dev = x.device
    tf = _threshold_array(thresholds, "thresholds")
    if on is not None:
        if onset_thresholds is None:
            raise ValueError("onset_thresholds: needed with onset_logits")
        to = _threshold_array(onset_thresholds, "onset_thresholds")
    else:
        to = np.full(1, 0.5, np.float32)
    as_list = isinstance(ref, dict)
    if as_list:
        r_on, r_off, r_ptr = _note_tables(ref, B, P, dev)
    else:
        roll = _rows(ref, "ref_roll")
        if roll.shape != x.shape:
            raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, ref {tuple(roll.shape)}")
    ln = _lengths(lengths, B, dev)
    Kf, Ko = len(tf), len(to)
    out = torch.empty(B, Kf, Ko, 4, dtype=torch.int64, device=dev)
    ko = min(Ko, SWEEP_MAX_K)                                # tiles of kf x ko <= 64 pairs, the onset axis as wide as it goes
    kf = min(Kf, SWEEP_MAX_K, SWEEP_MAX_PAIRS // ko)
    with torch.cuda.device(dev):
        for i0 in range(0, Kf, kf):
            for j0 in range(0, Ko, ko):
                a, b = np.ascontiguousarray(tf[i0:i0 + kf]), np.ascontiguousarray(to[j0:j0 + ko])
                whole = len(a) == Kf and len(b) == Ko
                c = out if whole else torch.empty(B, len(a), len(b), 4, dtype=torch.int64, device=dev)
                tb = b.ctypes.data if on is not None else None
                if as_list:
                    check(lib.mt_note_sweep_list(ptr(x), ptr(on), a.ctypes.data, len(a), tb, len(b), ptr(r_on), ptr(r_off), ptr(r_ptr), ptr(ln),
                                                 ptr(c), B, P, T, _lib.stream_ptr()), "mt_note_sweep_list")
                else:
                    check(lib.mt_note_sweep_counts(ptr(x), ptr(on), a.ctypes.data, len(a), tb, len(b), ptr(roll), ptr(ln), ptr(c), B, P, T,
                                                   _lib.stream_ptr()), "mt_note_sweep_counts")
                if not whole:
                    out[:, i0:i0 + len(a), j0:j0 + len(b)] = c
    return out


GRID_MAX_K, GRID_MAX_CONFIGS = 16, 64              # mt_note_grid_*: values per axis, configurations per call


def note_grid_counts(frame_logits: torch.Tensor, ref, thresholds, onset_logits: Optional[torch.Tensor] = None, onset_thresholds=None,
                     offset_logits: Optional[torch.Tensor] = None, offset_thresholds=None, cleanups=None, lengths=None,
                     smoothings=None, onset_detect: str = "edge", peak_reaches=None) -> torch.Tensor:
    """note_match_counts (ref = a (B, P, T) roll) or note_match_list (ref = the {"on", "off", "ptr"} note list) at every cell of
    `thresholds` x `onset_thresholds` x `offset_thresholds` x `cleanups` -> (B, Kf, Ko, Kk, Kc, 4) int64 device tensor; [b, i, j, k, c]
    is exactly what the single call returns at (thresholds[i], onset_thresholds[j], offset_thresholds[k]) with (min_note_frames,
    bridge_frames) = cleanups[c] (mt_note_grid_counts / mt_note_grid_list).  cleanups: a list of (min_note_frames, bridge_frames)
    pairs as check_cleanup takes them, None = [(1, 0)].  Without offset logits (the onset-gated decoder) Kk = 1 and offset_thresholds
    is not read; without onset logits either (the frame decoder) Ko = 1 as well.  The logits are read, and their sigmoids evaluated,
    once per call of the kernel; a grid past its limits (16 per axis, 64 configurations) is cut into several calls here and pasted
    together.  With a roll nothing synchronises (a note list's ptr table is checked with one small read-back, as in note_match_list).
    smoothings: a non-empty list of (smooth_on, smooth_off) pairs as check_smoothing takes them adds an axis Ks after the frame axis ->
    (B, Kf, Ks, Ko, Kk, Kc, 4); [b, i, s, j, k, c] is exactly what the single call returns with smooth_on, smooth_off = smoothings[s] as
    well.  The Kf * Ks frame candidates are cut into tiles of at most 16; per tile one mt_frame_smooth_paths launch packs their Viterbi
    paths into bit masks (smooth_frame_paths), which mt_note_grid_counts_paths / mt_note_grid_list_paths read as their frame axis in
    place of thresholds (DESIGN.md 6c "Smoothing in the decoder grid").  (0, 0) goes the same way: its path is the threshold's
    activity.  None: no such axis, and the calls above.
    peak_reaches: a non-empty list of integers in [0, 8] (needs onset_logits) adds a last axis Kr before the 4 counts -> (B, Kf, Ko, Kk,
    Kc, Kr, 4), with smoothings (B, Kf, Ks, Ko, Kk, Kc, Kr, 4); [..., r, :] is exactly what the single call returns at
    onset_detect="peak", peak_reach=peak_reaches[r] and the cell's other parameters, and for a reach of 0 the edge call (the
    mt_note_grid_*_peak entry points; DESIGN.md 6c "Peak picking in the decoder grid").  None: no such axis, and the calls above.
    onset_detect: "edge" only; "peak" raises, the detector being an axis of the grid (peak_reaches) and not a mode of it."""
    refuse_peak(onset_detect, "note_grid_counts", reaches=True)
    reach = None if peak_reaches is None else check_peak_reaches(peak_reaches, onset_logits is not None)
    if offset_logits is not None and onset_logits is None:
        raise ValueError("offset_logits: the offset-gated decoder needs onset_logits as well")
    x = _rows(frame_logits, "frame_logits")
    heads = {}
    for name, lg, ths in (("onset", onset_logits, onset_thresholds), ("offset", offset_logits, offset_thresholds)):
        if lg is None:
            heads[name] = (None, np.full(1, 0.5, np.float32))
            continue
        h = _rows(lg, f"{name}_logits")
        if h.shape != x.shape:
            raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, {name} {tuple(h.shape)}")
        if ths is None:
            raise ValueError(f"{name}_thresholds: needed with {name}_logits")
        heads[name] = (h, _threshold_array(ths, f"{name}_thresholds"))
    (on, to), (off, tk) = heads["onset"], heads["offset"]
    tf = _threshold_array(thresholds, "thresholds")
    smooth = None if smoothings is None else _smoothing_list(smoothings)
    pairs = [(1, 0)] if cleanups is None else [check_cleanup(*c) for c in cleanups]
    if not pairs:
        raise ValueError("cleanups: expected a non-empty list of (min_note_frames, bridge_frames) pairs")
    cl = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    B, P, T = x.shape
    dev = x.device
    as_list = isinstance(ref, dict)
    if as_list:
        r_on, r_off, r_ptr = _note_tables(ref, B, P, dev)
    else:
        roll = _rows(ref, "ref_roll")
        if roll.shape != x.shape:
            raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, ref {tuple(roll.shape)}")
    ln = _lengths(lengths, B, dev)
    Ko, Kk, Kc, Kr = len(to), len(tk), len(cl), 1 if reach is None else len(reach)
    kr = min(Kr, GRID_MAX_K)                                 # tiles of kf x ko x kk x kc x kr <= 64, the inner axes as wide as they go
    kc = min(Kc, GRID_MAX_K, GRID_MAX_CONFIGS // kr)
    kk = min(Kk, GRID_MAX_K, GRID_MAX_CONFIGS // (kr * kc))
    ko = min(Ko, GRID_MAX_K, GRID_MAX_CONFIGS // (kr * kc * kk))
    tail = (4,) if reach is None else (Kr, 4)                # a result's last axes

    def tiles(out, head):
        """Fill out (B, Kf, Ko, Kk, Kc, *tail) tile by tile; head(i0, n) = the arguments of entries i0 .. i0 + n of the frame axis (those
        before thr_onset) and the suffix of the entry points that take them."""
        Kf = out.shape[1]
        kf = min(Kf, GRID_MAX_K, GRID_MAX_CONFIGS // (kr * kc * kk * ko))
        for i0, j0, k0, c0, r0 in itertools.product(range(0, Kf, kf), range(0, Ko, ko), range(0, Kk, kk), range(0, Kc, kc), range(0, Kr, kr)):
            n = min(kf, Kf - i0)
            b, k, c = (np.ascontiguousarray(v) for v in (to[j0:j0 + ko], tk[k0:k0 + kk], cl[c0:c0 + kc]))
            r = None if reach is None else np.ascontiguousarray(reach[r0:r0 + kr])
            whole = (n, len(b), len(k), len(c)) == (Kf, Ko, Kk, Kc) and (r is None or len(r) == Kr) and out.is_contiguous()
            t = out if whole else torch.empty(B, n, len(b), len(k), len(c), *(() if r is None else (len(r),)), 4, dtype=torch.int64,
                                              device=dev)
            first, suffix = head(i0, n)
            axes = (*first, b.ctypes.data if on is not None else None, len(b), k.ctypes.data if off is not None else None, len(k),
                    c.ctypes.data, len(c), *(() if r is None else (r.ctypes.data, len(r))))
            if r is not None:
                suffix += "_peak"
            if as_list:
                name = "mt_note_grid_list" + suffix
                check(getattr(lib, name)(*axes, ptr(r_on), ptr(r_off), ptr(r_ptr), ptr(ln), ptr(t), B, P, T, _lib.stream_ptr()), name)
            else:
                name = "mt_note_grid_counts" + suffix
                check(getattr(lib, name)(*axes, ptr(roll), ptr(ln), ptr(t), B, P, T, _lib.stream_ptr()), name)
            if not whole:
                at = (slice(None), slice(i0, i0 + n), slice(j0, j0 + len(b)), slice(k0, k0 + len(k)), slice(c0, c0 + len(c)))
                out[at if r is None else (*at, slice(r0, r0 + len(r)))] = t

    with torch.cuda.device(dev):
        if smooth is None:
            out = torch.empty(B, len(tf), Ko, Kk, Kc, *tail, dtype=torch.int64, device=dev)

            tiles(out, lambda i0, n: ((ptr(x), ptr(on), ptr(off), tf[i0:].ctypes.data, n), ""))         # (tf: contiguous float32)
            return out
        Ks = len(smooth)
        cand_thr = np.repeat(tf, Ks)                         # candidate i * Ks + s = (thresholds[i], smoothings[s]): frame-major
        cand = smooth * len(tf)
        out = torch.empty(B, len(cand), Ko, Kk, Kc, *tail, dtype=torch.int64, device=dev)
        for q0 in range(0, len(cand), SMOOTH_MAX_K):
            paths = _paths(x, cand_thr[q0:q0 + SMOOTH_MAX_K], cand[q0:q0 + SMOOTH_MAX_K], ln)
            tiles(out[:, q0:q0 + len(paths)], lambda i0, n: ((ptr(paths[i0:i0 + n]), n, ptr(on), ptr(off)), "_paths"))
    return out.reshape(B, len(tf), Ks, Ko, Kk, Kc, *tail)


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


def heads_to_notes_device(frame_logits: torch.Tensor, onset_logits: Optional[torch.Tensor], threshold: float = 0.5,
                          onset_threshold: float = 0.5, fs: float = FS, min_midi: int = 21, offset_logits: Optional[torch.Tensor] = None,
                          offset_threshold: float = 0.5, min_note_frames: int = 1, bridge_frames: int = 0, smooth_on: float = 0.0,
                          smooth_off: float = 0.0, refine_onsets: bool = False, refine_reach: int = 2, onset_detect: str = "edge",
                          peak_reach: int = 1) -> List[Tuple[int, float, float]]:
    """(n_chunks, 88, T) frame and onset logits ON THE DEVICE -> notes of the onset-gated decoder over the chunks concatenated in
    time, in the reference's note order (pitch-major, then time); only counts and two ints per note reach the host.  With
    offset_logits: the notes of the offset-gated decoder (mt_heads_to_notes_off), which end where the offset head fires.  With
    (min_note_frames, bridge_frames) other than (1, 0): the cleaned notes (mt_heads_to_notes_clean), and then onset_logits may be
    None: the frame decoder's notes, cleaned.  With (smooth_on, smooth_off) other than (0, 0) the frame head is smoothed first, over
    the chunks concatenated in time (smooth_frame_logits, chunks=True).  refine_onsets=True: one more launch (mt_refine_onsets, reach
    refine_reach) gives every note a sub-frame onset; its start is then on_tick / 1e4 seconds, its end unchanged (e / fs), and the
    ticks ride in the note copy.  The frame decoder has no onset head to refine from: it raises.  onset_detect="peak" (needs
    onset_logits): notes open at the peaks of the onset logits over peak_reach frames, neighbours across chunk boundaries
    (mt_heads_to_notes_peak; DESIGN.md 6c "Peak-picked onsets"); the refined tick of a peak is the same at every refine_reach."""
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    reach = _check_refine(refine_onsets, refine_reach, onset_logits)
    peak = check_onset_detect(onset_detect, peak_reach, onset_logits is not None)
    x, on, off, thr, othr, kthr, _ = _heads(frame_logits, onset_logits, offset_logits, threshold, onset_threshold, offset_threshold,
                                            onset_required=clean == (1, 0), mismatch="frame {frame} and onset {onset} logits differ in shape")
    if smooth != (0.0, 0.0):
        x = _smoothed(x, thr, smooth, None, True)
    c, s, e, tick = _heads_to_notes_raw(x, on, off, (thr, othr, kthr), clean, reach, peak)
    pitches = np.repeat(np.arange(x.shape[1]) + min_midi, c)
    if reach is not None:
        return [(int(pp), float(a) / TICKS_PER_SECOND, float(b) / fs) for pp, a, b in zip(pitches, tick, e)]
    return [(int(pp), float(a) / fs, float(b) / fs) for pp, a, b in zip(pitches, s, e)]


def _heads_to_notes_raw(x, on, off, thrs, clean, reach: Optional[int], peak: int = 0, on_device: bool = False):
    """The mt_heads_to_notes family on checked (NB, P, T) heads -> host arrays (counts (P,), starts, ends, ticks); ticks None without
    `reach`, else mt_refine_onsets' onsets of the same notes, which ride in the note copy.  peak: check_onset_detect's result.
    on_device (needs `reach`): starts, ends and ticks stay int32 device tensors; only the counts (the capacity check) reach the host."""
    NB, P, T = x.shape
    dev = x.device
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    cap = max(1024, NB * 64)
    while True:
        if reach is None:
            starts, ends = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        else:
            se = torch.empty(3, cap, dtype=torch.int32, device=dev)                            # starts | ends | ticks: one copy
            starts, ends = se[0], se[1]
        with torch.cuda.device(dev):
            _decode("mt_heads_to_notes", clean, x, on, off, thrs, (NB, P, T, ptr(counts), ptr(starts), ptr(ends), cap, _lib.stream_ptr()),
                    peak=peak)
        c = counts.cpu().numpy()
        total = int(c.sum())
        if total <= cap:
            break
        cap = total
    if reach is None:
        return c, starts[:total].cpu().numpy(), ends[:total].cpu().numpy(), None
    row_off = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    row_off[1:] = torch.cumsum(counts, 0)
    _refine(starts, ends, row_off, total, on, None, True, reach, se[2])
    if on_device:
        return c, se[0, :total], se[1, :total], se[2, :total]
    s, e, tick = se[:, :total].cpu().numpy()
    return c, s, e, tick


def notes_batch_device(frame_logits: torch.Tensor, onset_logits: Optional[torch.Tensor] = None, threshold: float = 0.5,
                       onset_threshold: float = 0.5, lengths=None, fs: float = FS, min_midi: int = 21, min_note_frames: int = 1,
                       bridge_frames: int = 0, smooth_on: float = 0.0, smooth_off: float = 0.0, refine_onsets: bool = False,
                       refine_reach: int = 2, onset_detect: str = "edge", peak_reach: int = 1) -> List[List[Tuple[int, float, float]]]:
    """(B, P, T) frame logits of B whole recordings ON THE DEVICE, padded to T, with lengths (B,) valid frames each (None: all T) ->
    one note list per recording: what transcribe.notes_from_logits_device (onset_logits None) or heads_to_notes_device returns on
    that recording's rows trimmed to its length.  The padding is never read.  One launch of mt_notes_batch, one device-to-host copy
    of the counts and offsets and one of the notes; a second launch only when the first capacity guess was short.  With
    (min_note_frames, bridge_frames) other than (1, 0) the notes are cleaned in the decoder (mt_notes_batch_clean).  With
    (smooth_on, smooth_off) other than (0, 0) the frame head is smoothed first (smooth_frame_logits, over the same lengths).
    refine_onsets=True (onset-gated decoder only): as in heads_to_notes_device, a note's start is its refined on_tick / 1e4 seconds.
    onset_detect="peak" (needs onset_logits): notes open at the peaks of the onset logits over peak_reach frames (mt_notes_batch_peak)."""
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    reach = _check_refine(refine_onsets, refine_reach, onset_logits)
    peak = check_onset_detect(onset_detect, peak_reach, onset_logits is not None)
    x, on, _, thr, othr, _, _ = _heads(frame_logits, onset_logits, None, threshold, onset_threshold, 0.5,
                                       mismatch="frame {frame} and onset {onset} logits differ in shape")
    B, P, T = x.shape
    ln = _lengths(lengths, B, x.device)
    if smooth != (0.0, 0.0):
        x = _smoothed(x, thr, smooth, ln, False)
    off, c, s, e, tick = _notes_batch_raw(x, on, ln, thr, othr, clean, reach, peak)
    if reach is not None:
        s, fs_on = tick, float(TICKS_PER_SECOND)            # starts in ticks
    else:
        fs_on = fs
    pitches = np.tile(np.arange(P) + min_midi, B)
    out = []
    for b in range(B):
        lo, hi = int(off[b * P]), int(off[(b + 1) * P])
        pp = np.repeat(pitches[b * P:(b + 1) * P], c[b * P:(b + 1) * P])
        out.append([(int(q), float(a) / fs_on, float(z) / fs) for q, a, z in zip(pp, s[lo:hi], e[lo:hi])])
    return out


def _notes_batch_raw(x, on, ln, thr, othr, clean, reach: Optional[int], peak: int = 0, on_device: bool = False):
    """mt_notes_batch / mt_notes_batch_clean on checked (B, P, T) heads -> host arrays (row_off (B * P + 1,), counts (B * P,), starts,
    ends, ticks); ticks None without `reach`, else mt_refine_onsets' onsets of the same notes, which ride in the note copy.  peak:
    check_onset_detect's result (mt_notes_batch_peak).  on_device (needs `reach`): row_off, starts, ends and ticks stay device tensors
    (int64, int32 x 3); the one read-back is the capacity check (row_off and counts, as before)."""
    B, P, T = x.shape
    dev = x.device
    rows = B * P
    meta = torch.empty(rows + 1 + (rows + 1) // 2, dtype=torch.int64, device=dev)      # row_off (rows + 1) | counts (rows int32): one copy
    row_off, counts = meta[:rows + 1], meta[rows + 1:].view(torch.int32)[:rows]
    cap = max(1024, (B * T) // 16)
    while True:
        se = torch.empty(2 if reach is None else 3, cap, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _decode("mt_notes_batch", clean, x, on, None, (thr, othr, 0.5),
                    (ptr(ln), B, P, T, ptr(counts), ptr(row_off), ptr(se[0]), ptr(se[1]), cap, _lib.stream_ptr()), offset_head=False, peak=peak)
        host = meta.cpu().numpy()
        off, c = host[:rows + 1], host[rows + 1:].view(np.int32)[:rows]
        total = int(off[rows])
        if total <= cap:
            break
        cap = total
    if reach is None:
        s, e = se[:, :total].cpu().numpy()
        return off, c, s, e, None
    _refine(se[0], se[1], row_off, total, on, ln, False, reach, se[2])
    if on_device:
        return row_off, c, se[0, :total], se[1, :total], se[2, :total]
    s, e, tick = se[:, :total].cpu().numpy()
    return off, c, s, e, tick


def notes_ticks_device(frame_logits: torch.Tensor, onset_logits: torch.Tensor, threshold: float = 0.5, onset_threshold: float = 0.5,
                       lengths=None, offset_logits: Optional[torch.Tensor] = None, offset_threshold: float = 0.5, min_note_frames: int = 1,
                       bridge_frames: int = 0, smooth_on: float = 0.0, smooth_off: float = 0.0, refine_reach: int = 2,
                       onset_detect: str = "edge", peak_reach: int = 1) -> Dict[str, np.ndarray]:
    """The notes of a padded batch (B, P, T) with refined onsets, as a note list on the host for note_match_ticks: {"on", "off"} int32
    ticks of 100 us (on = mt_refine_onsets' sub-frame onset, off = 320 e) and "ptr" int64 (B * P + 1,), in the layout of
    MaestroDataset.ref_notes.  The onset-gated decoder goes through mt_notes_batch* and one refinement launch for the whole batch; with
    offset_logits (the batched extractor reads two heads) every recording is decoded on its own valid frames with
    mt_heads_to_notes_off / _clean and refined there.  onset_detect="peak": the mt_*_peak entry points of either path, over peak_reach frames."""
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    reach = _check_refine(True, refine_reach, onset_logits)
    peak = check_onset_detect(onset_detect, peak_reach, onset_logits is not None)
    x, on, off, thr, othr, kthr, _ = _heads(frame_logits, onset_logits, offset_logits, threshold, onset_threshold, offset_threshold,
                                            mismatch="frame {frame} and onset {onset} logits differ in shape")
    B, P, T = x.shape
    ln = _lengths(lengths, B, x.device)
    if smooth != (0.0, 0.0):
        x = _smoothed(x, thr, smooth, ln, False)
    if off is None:
        ptrs, _, _, e, tick = _notes_batch_raw(x, on, ln, thr, othr, clean, reach, peak)
        return {"on": tick.astype(np.int32), "off": (e * TICKS_PER_FRAME).astype(np.int32), "ptr": ptrs.astype(np.int64)}
    lens = [T] * B if ln is None else [min(max(int(v), 0), T) for v in ln.cpu().numpy()]
    ons, offs, ptrs = [], [], [np.zeros(1, np.int64)]
    for b, L in enumerate(lens):
        if L == 0:
            c, e, tick = np.zeros(P, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
        else:
            cut = lambda h: h[b:b + 1, :, :L].contiguous()
            c, _, e, tick = _heads_to_notes_raw(cut(x), cut(on), cut(off), (thr, othr, kthr), clean, reach, peak)
        ons.append(tick)
        offs.append(e * TICKS_PER_FRAME)
        ptrs.append(ptrs[-1][-1] + np.cumsum(c, dtype=np.int64))
    return {"on": np.concatenate(ons).astype(np.int32), "off": np.concatenate(offs).astype(np.int32), "ptr": np.concatenate(ptrs)}


def notes_ticks_tables_device(frame_logits: torch.Tensor, onset_logits: torch.Tensor, threshold: float = 0.5, onset_threshold: float = 0.5,
                              lengths=None, offset_logits: Optional[torch.Tensor] = None, offset_threshold: float = 0.5,
                              min_note_frames: int = 1, bridge_frames: int = 0, smooth_on: float = 0.0, smooth_off: float = 0.0,
                              refine_reach: int = 2, onset_detect: str = "edge", peak_reach: int = 1) -> Dict[str, torch.Tensor]:
    """notes_ticks_device with the three tables left ON THE DEVICE, for note_match_ticks_device: the same arguments, the same notes,
    {"on", "off"} int32 and "ptr" int64 device tensors.  Onset-gated decoder: mt_notes_batch*, mt_refine_onsets, off = 320 ends and
    ptr = the extractor's row_off; the only read-back is the extractor's capacity check.  With offset_logits every recording is still
    decoded on its own (the batched extractor reads two heads), its notes stay on the device, and the tables are put together there;
    per recording the counts of its 88 rows reach the host (the capacity check of mt_heads_to_notes_*), and lengths once."""
    clean = check_cleanup(min_note_frames, bridge_frames)
    smooth = check_smoothing(smooth_on, smooth_off)
    reach = _check_refine(True, refine_reach, onset_logits)
    peak = check_onset_detect(onset_detect, peak_reach, onset_logits is not None)
    x, on, off, thr, othr, kthr, _ = _heads(frame_logits, onset_logits, offset_logits, threshold, onset_threshold, offset_threshold,
                                            mismatch="frame {frame} and onset {onset} logits differ in shape")
    B, P, T = x.shape
    dev = x.device
    ln = _lengths(lengths, B, dev)
    if smooth != (0.0, 0.0):
        x = _smoothed(x, thr, smooth, ln, False)
    if off is None:
        row_off, _, _, e, tick = _notes_batch_raw(x, on, ln, thr, othr, clean, reach, peak, on_device=True)
        return {"on": tick.contiguous(), "off": e * TICKS_PER_FRAME, "ptr": row_off.clone()}
    lens = [T] * B if ln is None else [min(max(int(v), 0), T) for v in ln.cpu().numpy()]
    ons, offs, ptrs = [], [], [np.zeros(1, np.int64)]
    for b, L in enumerate(lens):
        c = np.zeros(P, np.int32)
        if L:
            cut = lambda h: h[b:b + 1, :, :L].contiguous()
            c, _, e, tick = _heads_to_notes_raw(cut(x), cut(on), cut(off), (thr, othr, kthr), clean, reach, peak, on_device=True)
            ons.append(tick)
            offs.append(e * TICKS_PER_FRAME)
        ptrs.append(ptrs[-1][-1] + np.cumsum(c, dtype=np.int64))
    none = torch.zeros(0, dtype=torch.int32, device=dev)
    return {"on": torch.cat(ons + [none]), "off": torch.cat(offs + [none]), "ptr": torch.from_numpy(np.concatenate(ptrs)).to(dev)}


def note_match_ticks_device(est_notes: Dict[str, torch.Tensor], ref_notes: Dict[str, torch.Tensor], lengths=None) -> torch.Tensor:
    """note_match_ticks on the device (mt_note_match_ticks; DESIGN.md 6c "Sub-frame onsets", Scoring): both arguments {"on", "off"} int32
    ticks of 100 us and "ptr" int64 DEVICE tensors in the layout of MaestroDataset.ref_notes, the same number of rows on both sides, a
    multiple of 88 -> (B, 4) int64 device tensor {n_ref, n_est, tp_onset, tp_onset_offset}, equal to note_match_ticks on the same
    lists.  lengths (B,) frames, None = no clipping: reference notes with on >= 320 lengths[b] are not counted and reference offsets
    are clipped there, as in note_match_list; estimates are taken as given.  The tables are checked as note_match_list checks its
    reference, and `on` must be non-decreasing inside every row on both sides (the kernel searches it); one small read-back per side
    does both, and a bad table raises ValueError before any launch.  The kernel's workspace is allocated here."""
    for d, who in ((est_notes, "est_notes"), (ref_notes, "ref_notes")):
        for k in ("on", "off", "ptr"):
            if not torch.is_tensor(d[k]) or not d[k].is_cuda:
                raise ValueError(f"{who}[{k!r}]: expected a CUDA tensor")
    dev = est_notes["ptr"].device
    rows = est_notes["ptr"].numel() - 1
    if rows <= 0 or rows % _lib.N_PITCH or ref_notes["ptr"].numel() - 1 != rows:
        raise ValueError(f"note_match_ticks_device: {rows} estimated and {ref_notes['ptr'].numel() - 1} reference rows "
                         f"(expected equal multiples of {_lib.N_PITCH})")
    B, P = rows // _lib.N_PITCH, _lib.N_PITCH
    n_est, n_ref = est_notes["on"].numel(), ref_notes["on"].numel()
    e_on, e_off, e_ptr = _note_tables(est_notes, B, P, dev, "est_notes", sorted_rows=True)
    r_on, r_off, r_ptr = _note_tables(ref_notes, B, P, dev, "ref_notes", sorted_rows=True)
    ln = _lengths(lengths, B, dev)
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.mt_note_match_ticks_workspace(n_est, n_ref)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.mt_note_match_ticks(ptr(e_on), ptr(e_off), ptr(e_ptr), ptr(r_on), ptr(r_off), ptr(r_ptr), ptr(ln), ptr(counts), B, P,
                                      ptr(ws), ws.numel(), _lib.stream_ptr()), "mt_note_match_ticks")
    return counts


def _grid_ticks_tables(x, on, off, ln, axes, refine_reach: int):
    """mt_notes_grid_ticks on checked heads and one tile of axes (tf, to, tk, cl, reach: contiguous arrays, at most 64 cells) -> device
    tensors (row_off int64 (K * B * P + 1,), on_tick, off_tick int32 (total,)).  One read-back per launch pair: the total of the count
    pass, which is also the capacity check; a second pair only when the first guess was short."""
    tf, to, tk, cl, reach = axes
    B, P, T = x.shape
    dev = x.device
    K = len(tf) * len(to) * len(tk) * len(cl) * len(reach)
    rows = K * B * P
    row_off = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(rows, dtype=torch.int32, device=dev)
    cap = K * max(1024, (B * T) // 16)
    while True:
        if cap >= 2 ** 31:
            raise ValueError(f"note_grid_ticks_counts: {cap} notes in one tile of the grid do not fit 31 bits; score fewer cells per call")
        tab = torch.empty(2, cap, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib.mt_notes_grid_ticks(ptr(x), ptr(on), ptr(off), tf.ctypes.data, len(tf), to.ctypes.data, len(to),
                                          tk.ctypes.data if off is not None else None, len(tk), cl.ctypes.data, len(cl), reach.ctypes.data,
                                          len(reach), refine_reach, ptr(ln), B, P, T, ptr(counts), ptr(row_off), ptr(tab[0]), ptr(tab[1]), cap,
                                          _lib.stream_ptr()), "mt_notes_grid_ticks")
        total = int(row_off[rows])
        if total <= cap:
            return row_off, tab[0, :total], tab[1, :total]
        cap = total


def _grid_ticks_axes(frame_logits, onset_logits, offset_logits, thresholds, onset_thresholds, offset_thresholds, cleanups, peak_reaches,
                     lengths, refine_reach):
    """The checked arguments the two tick-grid calls share -> (x, on, off, ln, (tf, to, tk, cl, reach), refine_reach)."""
    if onset_logits is None:
        raise ValueError("onset_logits: refined onsets are read off the onset head; the tick grid needs the onset or the offset-gated decoder")
    rr = _check_refine(True, refine_reach, onset_logits)
    reach = np.zeros(1, np.int32) if peak_reaches is None else check_peak_reaches(peak_reaches, True)
    x = _rows(frame_logits, "frame_logits")
    heads = []
    for name, lg, ths in (("onset", onset_logits, onset_thresholds), ("offset", offset_logits, offset_thresholds)):
        if lg is None:
            heads.append((None, np.full(1, 0.5, np.float32)))
            continue
        h = _rows(lg, f"{name}_logits")
        if h.shape != x.shape:
            raise ValueError(f"shape mismatch: frame {tuple(x.shape)}, {name} {tuple(h.shape)}")
        if ths is None:
            raise ValueError(f"{name}_thresholds: needed with {name}_logits")
        heads.append((h, _threshold_array(ths, f"{name}_thresholds")))
    (on, to), (off, tk) = heads
    tf = _threshold_array(thresholds, "thresholds")
    pairs = [(1, 0)] if cleanups is None else [check_cleanup(*c) for c in cleanups]
    if not pairs:
        raise ValueError("cleanups: expected a non-empty list of (min_note_frames, bridge_frames) pairs")
    cl = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    if x.shape[1] != _lib.N_PITCH:
        raise ValueError(f"frame_logits: the tick grid scores against a note list of {_lib.N_PITCH} pitch rows, got {x.shape[1]}")
    return x, on, off, _lengths(lengths, x.shape[0], x.device), (tf, to, tk, cl, reach), rr


def notes_grid_ticks_tables_device(frame_logits: torch.Tensor, onset_logits: torch.Tensor, thresholds, onset_thresholds,
                                   offset_logits: Optional[torch.Tensor] = None, offset_thresholds=None, cleanups=None, peak_reaches=None,
                                   lengths=None, refine_reach: int = 2) -> Dict[str, torch.Tensor]:
    """The refined note lists of every cell of a decoder grid in one launch pair (mt_notes_grid_ticks; DESIGN.md 6c "Decoder grid in
    ticks"), for at most 64 cells with at most 16 values per axis: {"on", "off"} int32 and "ptr" int64 (K * B * 88 + 1,) DEVICE tensors,
    cell-major -- rows [cell * B * 88, (cell + 1) * B * 88) are, element for element, notes_ticks_tables_device's tables at the cell's
    parameters (onset_detect="peak", peak_reach=R for a reach R >= 1, "edge" for 0; no smoothing), ptr counted from the stacked table's
    start.  The cell index runs frame-major over thresholds x onset_thresholds x offset_thresholds x cleanups x peak_reaches (None =
    [0], the edge rule).  With offset_logits: the offset-gated decoder on each recording's valid frames, without the loop over
    recordings.  "cells" = K."""
    x, on, off, ln, axes, rr = _grid_ticks_axes(frame_logits, onset_logits, offset_logits, thresholds, onset_thresholds, offset_thresholds,
                                                cleanups, peak_reaches, lengths, refine_reach)
    K = int(np.prod([len(a) for a in axes]))
    if K > GRID_MAX_CONFIGS or max(len(a) for a in axes) > GRID_MAX_K:
        raise ValueError(f"notes_grid_ticks_tables_device: at most {GRID_MAX_K} values per axis and {GRID_MAX_CONFIGS} cells per call, got "
                         f"{[len(a) for a in axes]}; note_grid_ticks_counts tiles larger grids")
    row_off, t_on, t_off = _grid_ticks_tables(x, on, off, ln, [np.ascontiguousarray(a) for a in axes], rr)
    return {"on": t_on, "off": t_off, "ptr": row_off, "cells": K}


def note_match_ticks_cells_device(est_notes: Dict[str, torch.Tensor], ref_notes: Dict[str, torch.Tensor], cells: int,
                                  lengths=None, checked: bool = True) -> torch.Tensor:
    """note_match_ticks_device for K = `cells` estimate tables stacked cell-major (K * B * 88 rows, as notes_grid_ticks_tables_device
    leaves them) against one reference of B * 88 rows -> (K, B, 4) int64 device tensor; [k] is what note_match_ticks_device returns on
    cell k's slice (mt_note_match_ticks_cells).  ref_notes is checked as note_match_ticks_device checks it, and so are the estimates
    (one small read-back per side); checked=False leaves the estimates to the kernel's own checks, which touch nothing on a bad row and
    set bit 63 of the four counts of its (cell, recording)."""
    for d, who in ((est_notes, "est_notes"), (ref_notes, "ref_notes")):
        for k in ("on", "off", "ptr"):
            if not torch.is_tensor(d[k]) or not d[k].is_cuda:
                raise ValueError(f"{who}[{k!r}]: expected a CUDA tensor")
    K = int(cells)
    dev = ref_notes["ptr"].device
    rows = ref_notes["ptr"].numel() - 1
    if K < 1 or rows <= 0 or rows % _lib.N_PITCH or est_notes["ptr"].numel() - 1 != K * rows:
        raise ValueError(f"note_match_ticks_cells_device: {est_notes['ptr'].numel() - 1} estimated rows for {K} cells of {rows} reference "
                         f"rows (expected cells * rows, rows a multiple of {_lib.N_PITCH})")
    B, P = rows // _lib.N_PITCH, _lib.N_PITCH
    n_est, n_ref = est_notes["on"].numel(), ref_notes["on"].numel()
    r_on, r_off, r_ptr = _note_tables(ref_notes, B, P, dev, "ref_notes", sorted_rows=True)
    if checked:
        e_on, e_off, e_ptr = _note_tables(est_notes, K * B, P, dev, "est_notes", sorted_rows=True)
    else:
        e_on, e_off, e_ptr = (est_notes[k].contiguous() for k in ("on", "off", "ptr"))
        if n_est == 0:
            e_on = e_off = torch.zeros(1, dtype=torch.int32, device=dev)
    return _match_cells(e_on, e_off, e_ptr, n_est, r_on, r_off, r_ptr, n_ref, _lengths(lengths, B, dev), K, B, P)


def _match_cells(e_on, e_off, e_ptr, n_est: int, r_on, r_off, r_ptr, n_ref: int, ln, K: int, B: int, P: int) -> torch.Tensor:
    """mt_note_match_ticks_cells on checked, contiguous tables -> (K, B, 4) int64 device tensor.  The workspace is allocated here."""
    dev = e_ptr.device
    counts = torch.empty(K, B, 4, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.mt_note_match_ticks_cells_workspace(n_est, n_ref, K)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.mt_note_match_ticks_cells(ptr(e_on), ptr(e_off), ptr(e_ptr), ptr(r_on), ptr(r_off), ptr(r_ptr), ptr(ln), ptr(counts), K, B, P,
                                            ptr(ws), ws.numel(), _lib.stream_ptr()), "mt_note_match_ticks_cells")
    return counts


def note_grid_ticks_counts(frame_logits: torch.Tensor, onset_logits: torch.Tensor, ref_notes: Dict[str, torch.Tensor], thresholds,
                           onset_thresholds, offset_logits: Optional[torch.Tensor] = None, offset_thresholds=None, cleanups=None,
                           peak_reaches=None, lengths=None, refine_reach: int = 2) -> torch.Tensor:
    """note_match_ticks_device(notes_ticks_tables_device(cell, lengths), ref_notes) at every cell of `thresholds` x `onset_thresholds` x
    `offset_thresholds` x `cleanups` [x `peak_reaches`] -> (B, Kf, Ko, Kk, Kc[, Kr], 4) int64 device tensor, the axes, their conventions
    and the tiling rule those of note_grid_counts (16 values per axis and 64 cells per kernel call, the inner axes as wide as they go):
    the note-level counts of the path evaluation reports with refine_onsets -- refined onsets, scored in ticks by a maximum matching --
    for a whole decoder grid (DESIGN.md 6c "Decoder grid in ticks").  Per tile one mt_notes_grid_ticks launch pair decodes every cell
    into its refined note list (the logits read and their sigmoids evaluated once per window, not once per cell; one read-back, the
    total of the count pass) and one mt_note_match_ticks_cells launch scores all of them.  (B, 88, T) logits of the onset-gated or,
    with offset_logits, the offset-gated decoder; ref_notes: {"on", "off", "ptr"} device tables, checked as note_match_ticks_device
    checks them (one small read-back per call).  lengths bound the decoding only: the whole reference list is scored, as
    evaluate.note_metrics_dataset(refine_onsets=True) scores it.  peak_reaches: as in note_grid_counts, None = the edge rule and no such axis.  Frame
    smoothing is not an axis here (the packed-paths frame axis is out of scope)."""
    x, on, off, ln, (tf, to, tk, cl, reach), rr = _grid_ticks_axes(frame_logits, onset_logits, offset_logits, thresholds, onset_thresholds,
                                                                   offset_thresholds, cleanups, peak_reaches, lengths, refine_reach)
    B, P, T = x.shape
    dev = x.device
    for k in ("on", "off", "ptr"):
        if not torch.is_tensor(ref_notes[k]) or not ref_notes[k].is_cuda:
            raise ValueError(f"ref_notes[{k!r}]: expected a CUDA tensor")
    n_ref = ref_notes["on"].numel()
    r_on, r_off, r_ptr = _note_tables(ref_notes, B, P, dev, "ref_notes", sorted_rows=True)
    Kf, Ko, Kk, Kc, Kr = len(tf), len(to), len(tk), len(cl), len(reach)
    kr = min(Kr, GRID_MAX_K)                                 # tiles of kf x ko x kk x kc x kr <= 64, the inner axes as wide as they go
    kc = min(Kc, GRID_MAX_K, GRID_MAX_CONFIGS // kr)
    kk = min(Kk, GRID_MAX_K, GRID_MAX_CONFIGS // (kr * kc))
    ko = min(Ko, GRID_MAX_K, GRID_MAX_CONFIGS // (kr * kc * kk))
    kf = min(Kf, GRID_MAX_K, GRID_MAX_CONFIGS // (kr * kc * kk * ko))
    out = torch.empty(B, Kf, Ko, Kk, Kc, Kr, 4, dtype=torch.int64, device=dev)
    for i0, j0, k0, c0, r0 in itertools.product(range(0, Kf, kf), range(0, Ko, ko), range(0, Kk, kk), range(0, Kc, kc), range(0, Kr, kr)):
        axes = [np.ascontiguousarray(v) for v in (tf[i0:i0 + kf], to[j0:j0 + ko], tk[k0:k0 + kk], cl[c0:c0 + kc], reach[r0:r0 + kr])]
        shape = [len(a) for a in axes]
        K = int(np.prod(shape))
        row_off, e_on, e_off = _grid_ticks_tables(x, on, off, ln, axes, rr)
        n_est = e_on.numel()
        if n_est == 0:                                       # no notes at all: the kernel still wants readable tables
            e_on = e_off = torch.zeros(1, dtype=torch.int32, device=dev)
        c = _match_cells(e_on, e_off, row_off, n_est, r_on, r_off, r_ptr, n_ref, None, K, B, P)    # (the whole reference list)
        out[:, i0:i0 + shape[0], j0:j0 + shape[1], k0:k0 + shape[2], c0:c0 + shape[3], r0:r0 + shape[4]] = \
            c.reshape(*shape, B, 4).permute(5, 0, 1, 2, 3, 4, 6)
    return out if peak_reaches is not None else out[:, :, :, :, :, 0]


TICKS_PER_SECOND = 10000           # ticks of 100 us
MAX_REFINE_REACH = 8               # mt_refine_onsets: frames the peak search may walk from a note's start


def _check_refine(refine_onsets, refine_reach, onset_logits) -> Optional[int]:
    """The checked reach of a decoder call with refine_onsets, None without.  Raises before any GPU work."""
    if not refine_onsets:
        return None
    if onset_logits is None:
        raise ValueError("refine_onsets: sub-frame onsets are read off the onset head, and the frame decoder has none (pass onset_logits)")
    if isinstance(refine_reach, bool) or not isinstance(refine_reach, (int, np.integer)) or not 0 <= refine_reach <= MAX_REFINE_REACH:
        raise ValueError(f"refine_reach must be an integer number of frames in [0, {MAX_REFINE_REACH}], got {refine_reach!r}")
    return int(refine_reach)


def _refine(starts, ends, row_off, n: int, on: torch.Tensor, ln: Optional[torch.Tensor], chunks: bool, reach: int, out: torch.Tensor) -> None:
    """mt_refine_onsets on checked arguments: on contiguous (NB, P, T) f32, starts / ends / out int32 with at least n entries."""
    NB, P, T = on.shape
    with torch.cuda.device(on.device):
        check(lib.mt_refine_onsets(ptr(starts), ptr(ends), ptr(row_off), P if chunks else NB * P, n, ptr(on), NB, P, T, ptr(ln), int(chunks),
                                   reach, ptr(out), _lib.stream_ptr()), "mt_refine_onsets")


def refine_onsets_device(starts: torch.Tensor, ends: torch.Tensor, row_off: torch.Tensor, onset_logits: torch.Tensor, lengths=None,
                         chunks: bool = False, reach: int = 2) -> torch.Tensor:
    """Sub-frame onsets of decoded notes ON THE DEVICE -> int32 device tensor on_tick (n,), ticks of 100 us (mt_refine_onsets; DESIGN.md
    6c "Sub-frame onsets").  starts / ends: int32 (n,) frames [s, e) of the notes of any onset-gated decoder; row_off: int64
    (rows + 1,) rising from 0 to n, the notes of row r at row_off[r]:row_off[r + 1].  onset_logits (B, P, T): chunks=False a padded
    batch (rows = B * P, lengths (B,) valid frames, None = all T; the padding is never read), chunks=True the B chunks concatenated in
    time (rows = P, no lengths).  Per note the peak of sigmoid(onset) is searched from s over at most `reach` frames (0..8) inside the
    note, and the onset is 320 k + rint(320 shift) with the shift of the triangle through the peak and its neighbours, clamped to
    [0, 320 e - 1].  One read-back (row_off's last entry) checks the tables; the result stays on the device."""
    if onset_logits is None:
        raise ValueError("refine_onsets_device: needs the onset head's logits")
    reach = _check_refine(True, reach, onset_logits)
    on = _rows(onset_logits, "onset_logits")
    NB, P, T = on.shape
    dev = on.device
    if chunks and lengths is not None:
        raise ValueError("lengths: chunks=True concatenates whole chunks, which have no lengths")
    rows = P if chunks else NB * P
    for t, dt, name in ((starts, torch.int32, "starts"), (ends, torch.int32, "ends"), (row_off, torch.int64, "row_off")):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{name}: expected a 1-d {dt} tensor on {dev}")
    n = int(starts.numel())
    if ends.numel() != n or row_off.numel() != rows + 1:
        raise ValueError(f"refine_onsets_device: {n} starts, {ends.numel()} ends, row_off of {row_off.numel()} entries for {rows} rows")
    if bool((row_off[0] != 0) | (row_off[-1] != n) | (row_off[1:] < row_off[:-1]).any()):
        raise ValueError("row_off must rise from 0 to the number of notes")
    out = torch.empty(n, dtype=torch.int32, device=dev)
    _refine(starts.contiguous(), ends.contiguous(), row_off.contiguous(), n, on, _lengths(lengths, NB, dev), chunks, reach, out)
    return out


def _max_matching(adj: List[List[int]], n_right: int) -> int:
    """Size of a maximum matching of a bipartite graph, adj[i] = the right vertices of left vertex i (augmenting paths)."""
    match, size = [-1] * n_right, 0
    for root in range(len(adj)):
        if not adj[root]:
            continue
        seen = [False] * n_right
        stack, path, found = [[root, 0]], [], False         # depth-first without recursion: stack[d] = [left vertex, next edge], path[d] = its right vertex
        while stack and not found:
            i, it = stack[-1]
            if it == len(adj[i]):
                stack.pop()
                if path:
                    path.pop()
                continue
            stack[-1][1] = it + 1
            j = adj[i][it]
            if seen[j]:
                continue
            seen[j] = True
            path.append(j)
            if match[j] < 0:
                found = True
            else:
                stack.append([match[j], 0])
        if found:
            for (i, _), j in zip(stack, path):
                match[j] = i
            size += 1
    return size


def note_match_ticks(est_notes, ref_notes) -> np.ndarray:
    """Score estimated notes whose onsets lie off the frame grid (refine_onsets_device) against a note list, on the host.  Both
    arguments are {"on", "off", "ptr"} in the layout of MaestroDataset.ref_notes (ticks of 100 us, ptr with rows + 1 entries rising from
    0, the same number of rows on both sides, a multiple of 88; tensors or arrays) -> (B, 4) uint64 {n_ref, n_est, tp_onset,
    tp_onset_offset}, B = rows / 88.  mt_note_match_list's criteria: onsets match when |d on| <= 500 ticks, and for tp_onset_offset
    also 5 |d off| <= max(2500, reference length); each tp is a maximum matching, found per pitch row with augmenting paths.
    mt_note_match_list's streaming matcher relies on at most two frame-grid estimates inside a +-500 tick window, which refined
    onsets do not guarantee.  This host matcher is the specification of the device one, note_match_ticks_device, which
    evaluation uses; rows need not be sorted here."""
    def host(d, name):
        out = []
        for k in ("on", "off", "ptr"):
            v = d[k]
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            out.append(np.asarray(v, dtype=np.int64).reshape(-1))
        on, off, pt = out
        if pt.size < 1 or pt[0] != 0 or pt[-1] != on.size or on.size != off.size or (np.diff(pt) < 0).any():
            raise ValueError(f"{name}: ptr must rise from 0 to the number of notes, on / off of equal length")
        return on, off, pt
    e_on, e_off, e_ptr = host(est_notes, "est_notes")
    r_on, r_off, r_ptr = host(ref_notes, "ref_notes")
    rows = e_ptr.size - 1
    if r_ptr.size - 1 != rows or rows % _lib.N_PITCH:
        raise ValueError(f"note_match_ticks: {rows} estimated and {r_ptr.size - 1} reference rows (expected equal multiples of {_lib.N_PITCH})")
    counts = np.zeros((rows // _lib.N_PITCH, 4), dtype=np.uint64)
    for r in range(rows):
        eo, ef = e_on[e_ptr[r]:e_ptr[r + 1]], e_off[e_ptr[r]:e_ptr[r + 1]]
        ro, rf = r_on[r_ptr[r]:r_ptr[r + 1]], r_off[r_ptr[r]:r_ptr[r + 1]]
        c = counts[r // _lib.N_PITCH]
        c[0] += np.uint64(ro.size)
        c[1] += np.uint64(eo.size)
        if not ro.size or not eo.size:
            continue
        near = np.abs(ro[:, None] - eo[None, :]) <= 500
        if not near.any():
            continue
        both = near & (5 * np.abs(rf[:, None] - ef[None, :]) <= np.maximum(2500, rf - ro)[:, None])
        c[2] += np.uint64(_max_matching([np.flatnonzero(row).tolist() for row in near], eo.size))
        c[3] += np.uint64(_max_matching([np.flatnonzero(row).tolist() for row in both], eo.size))
    return counts
