"""MAESTRO recordings -> training batches on the device, without a preprocessed cache (the reference's MaestroDataset /
HybridMaestroDataset, data/dataset.py:9-200 and data/cached_dataset.py:91-141).

One split lives on the GPU:
  * audio: every recording decoded and resampled once (transcribe.load_audio_device) into ONE f32 device buffer with a
    per-recording (offset, n_samples) table (RecordingStore).  A split larger than `max_resident_bytes` keeps an LRU of
    whole recordings and re-decodes an evicted one when a batch needs it: same bytes, slower;
  * labels: per recording and pitch the sorted, disjoint frame spans in which the pitch sounds (label_spans: note spans
    int(start*fs):int(end*fs), the sustain-pedal running maximum, instrument widths int(fs*end_time), drums dropped),
    built on the host in float64 exactly as midi.Instrument.get_piano_roll renders them, and kilobytes per recording;
  * per chunk: the column grid round(linspace(start, end, int((end-start)*fs)) * fs) of pretty_midi's `times`, built on
    the host with numpy itself at construction (4 bytes per frame), so the device needs no float64 index arithmetic.
A batch is then two launches (csrc/rawbatch.hip): mt_mel_db_windows_f32 (mel of the ragged windows, trimmed and padded)
and mt_roll_windows (labels), with the same bytes a cache record written by preprocess_and_cache holds, collated as
data.collate_fn does.  A chunk is sliced from the recording resampled once, as the cache writer does; the reference
resamples each slice on its own (librosa.load(offset, duration), soxr).
With MaestroDataset(augment=Augment(...)) one more launch (csrc/augment.hip, mt_augment_windows) plays every window at a drawn
speed and adds noise before the mel launch reads it, and the labels go through a column table built for the batch's speeds.
"""
from __future__ import annotations

import os
import pickle
import warnings
from collections import OrderedDict
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import BatchSampler, Dataset, RandomSampler, SequentialSampler

from . import _lib
from ._lib import check, lib, ptr
from .frontend import get_frontend
from .midi import MidiFile
from .preprocess import build_chunk_index, read_maestro_csv, wav_duration
from .transcribe import load_audio_device

PITCH_LO, N_PITCH = 21, 88
_ALIGN = 64                  # floats: recordings start on 256-byte boundaries of the store
_PAD = 64                    # readable floats past the last recording (the mel kernel reads whole sample pairs)


# ------------------------------------------------------------------ labels
def _pedal_extend(start, end, ped_on, ped_off):
    """label_spans' pedal rule on one axis (frames or seconds): a note [start, end) that sounds inside a pedal interval
    [on, off) lasts to max(end, off).  Only the last interval starting before the note's end can reach past it."""
    if not len(ped_on):
        return end.copy()
    k = np.searchsorted(ped_on, end, side="left") - 1               # last pedal interval starting before the note's end
    has = k >= 0
    kk = np.where(has, k, 0)
    g0 = np.maximum(start, ped_on[kk])                               # the note's first frame inside the interval
    ext = has & (g0 < np.minimum(end, ped_off[kk]))
    return np.where(ext, np.maximum(end, ped_off[kk]), end)


def _instrument_notes(midi: MidiFile, fs: float):
    """The per-instrument work label_spans and label_notes share: (per non-drum instrument with notes, a dict of its kept notes:
    pitch row p, frames [a, end) and seconds [t0, t1), both pedal-extended), the full-file roll width, whether any instrument has
    notes.  Kept = pitch in range and a < b on the frame grid."""
    out, full_width, has_notes = [], 0, False
    for inst in midi.instruments:
        if not inst.notes:
            continue
        has_notes = True
        t_end = inst.get_end_time()
        width = int(fs * t_end)
        full_width = max(full_width, width)
        if inst.is_drum:
            continue
        pitch = np.array([n.pitch for n in inst.notes], dtype=np.int64)
        t0 = np.array([n.start for n in inst.notes], dtype=np.float64)
        t1 = np.array([n.end for n in inst.notes], dtype=np.float64)
        a = np.minimum((t0 * fs).astype(np.int64), width)
        b = np.minimum((t1 * fs).astype(np.int64), width)
        ons, offs, ons_t, offs_t, t_on, s_on, on = [], [], [], [], 0, 0.0, False
        for number, value, t in inst.control_changes:
            if number != 64:
                continue
            now, cur = int(t * fs), value >= 64
            if not on and cur:
                t_on, s_on, on = now, t, True
            elif on and not cur:
                ons.append(t_on)
                offs.append(now)
                ons_t.append(s_on)
                offs_t.append(t)
                on = False
        end = _pedal_extend(a, b, np.array(ons, dtype=np.int64), np.minimum(np.array(offs, dtype=np.int64), width))
        t_off = _pedal_extend(t0, t1, np.array(ons_t, dtype=np.float64), np.minimum(np.array(offs_t, dtype=np.float64), t_end))
        keep = (a < b) & (pitch >= PITCH_LO) & (pitch < PITCH_LO + N_PITCH)
        out.append({"p": pitch[keep] - PITCH_LO, "a": a[keep], "end": end[keep], "t0": t0[keep], "t1": t_off[keep]})
    return out, full_width, has_notes


def label_spans(midi: MidiFile, fs: float):
    """Active frame spans of `midi` on the grid of get_piano_roll(fs): (spans int32 (K, 2) of [u, v), pitch_off int64 (89,)
    -- pitch row p (MIDI 21 + p) owns spans[pitch_off[p]:pitch_off[p + 1]], sorted and disjoint --, the full-file roll
    width int(fs * end_time) over the instruments with notes (drums included, as get_piano_roll's width), and whether any
    instrument has notes (a roll of width 0 otherwise).

    Per non-drum instrument of width W: a note covers [int(start*fs), int(end*fs)); a sustain pedal interval [t_on, t_off)
    (CC 64 crossing 64 upwards, then downwards; one still down at the end sustains nothing) extends a note that sounds in it
    to min(t_off, W) from its first frame there (np.maximum.accumulate over non-negative velocities).  Only the last pedal
    interval starting before a note's end can reach past it: the intervals are disjoint and ordered."""
    insts, full_width, has_notes = _instrument_notes(midi, fs)
    u = np.concatenate([i["a"] for i in insts]) if insts else np.zeros(0, np.int64)
    v = np.concatenate([i["end"] for i in insts]) if insts else np.zeros(0, np.int64)
    p = np.concatenate([i["p"] for i in insts]) if insts else np.zeros(0, np.int64)
    spans, pitch_off = _merge_spans(u, v, p)
    return spans, pitch_off, full_width, has_notes


def _merge_spans(u, v, p):
    """Per pitch row, the union of the frame spans [u, v) as sorted, disjoint spans: (spans int32 (K, 2), pitch_off int64 (89,))."""
    # merge per pitch: keyed by pitch * BIG + frame, overlapping or touching spans join
    big = int(max(int(v.max()) if v.size else 0, 1)) + 2
    order = np.lexsort((u, p))
    u, v, p = u[order] + p[order] * big, v[order] + p[order] * big, p[order]
    if u.size:
        reach = np.maximum.accumulate(v)
        start = np.ones(u.size, dtype=bool)
        start[1:] = u[1:] > reach[:-1]
        mu, mv, mp = u[start], np.maximum.reduceat(v, np.flatnonzero(start)), p[start]
        spans = np.stack([mu - mp * big, mv - mp * big], 1).astype(np.int32)
    else:
        mp = p
        spans = np.zeros((0, 2), np.int32)
    pitch_off = np.searchsorted(mp, np.arange(N_PITCH + 1), side="left").astype(np.int64)
    return spans, pitch_off


TICKS_PER_SECOND = 10000     # note times in ticks of 100 us: one model frame (512 / 16000 s) is exactly 320 ticks
TICKS_PER_FRAME = 320
ONSET_WIDTH_RANGE = (2, 8)   # mt_onset_regress_windows: half-width of the onset triangle in frames


class NoteTable(NamedTuple):
    """label_notes' result.  Pitch row p owns entries pitch_off[p]:pitch_off[p + 1], sorted by onset (on_tick strictly rising)."""
    on_frame: np.ndarray      # int32: int(start * fs), the frame label_spans starts the note's span at
    end_frame: np.ndarray     # int32: the pedal-extended end of that span, un-cut (merging [on_frame, end_frame) gives label_spans)
    on_tick: np.ndarray       # int32: round(start * 1e4)
    off_tick: np.ndarray      # int32: round(pedal-extended end * 1e4), cut at the pitch's next onset; > on_tick
    pitch_off: np.ndarray     # int64 (89,)


def label_notes(midi: MidiFile, fs: float) -> NoteTable:
    """The notes behind label_spans, kept apart: what the merge into runs of the roll throws away.  Same instruments, pitch
    range, a < b and pedal rule as label_spans (shared code).  Per pitch row, sorted by onset: a note sounds from its note-on
    to its pedal-extended end (label_spans' rule on seconds: a note that sounds inside a pedal interval lasts to that
    interval's end); notes with the same (pitch, on_tick) collapse into the longest one; then a note is cut at the next
    onset of its pitch (a key cannot sound twice); off_tick >= on_tick + 1."""
    insts, _, _ = _instrument_notes(midi, fs)
    cat = lambda k, dt: np.concatenate([i[k] for i in insts]).astype(dt) if insts else np.zeros(0, dt)
    p, a, end = cat("p", np.int64), cat("a", np.int64), cat("end", np.int64)
    on = np.round(cat("t0", np.float64) * TICKS_PER_SECOND).astype(np.int64)
    off = np.round(cat("t1", np.float64) * TICKS_PER_SECOND).astype(np.int64)
    order = np.lexsort((-off, on, p))                                # per pitch by onset, the longest of equal onsets first
    p, a, end, on, off = p[order], a[order], end[order], on[order], off[order]
    first = np.ones(p.size, dtype=bool)
    first[1:] = (p[1:] != p[:-1]) | (on[1:] != on[:-1])
    if p.size:
        at = np.flatnonzero(first)
        a, end = np.minimum.reduceat(a, at), np.maximum.reduceat(end, at)   # the collapsed note covers its duplicates' frames
        p, on, off = p[first], on[first], off[first]
        nxt = np.full(p.size, np.iinfo(np.int64).max)
        same = p[1:] == p[:-1]
        nxt[:-1][same] = on[1:][same]
        off = np.maximum(np.minimum(off, nxt), on + 1)
    pitch_off = np.searchsorted(p, np.arange(N_PITCH + 1), side="left").astype(np.int64)
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    return NoteTable(i32(a), i32(end), i32(on), i32(off), pitch_off)


def onset_spans(notes: NoteTable):
    """The note-ons as a span table for mt_roll_windows: point spans [on_frame, on_frame + 1), de-duplicated per pitch, hence
    sorted and disjoint.  (spans int32 (K, 2), pitch_off int64 (89,))."""
    rows = np.repeat(np.arange(N_PITCH), np.diff(notes.pitch_off))
    key = np.unique(rows.astype(np.int64) * (1 << 32) + notes.on_frame.astype(np.int64))
    p, f = key >> 32, key & 0xFFFFFFFF
    spans = np.stack([f, f + 1], 1).astype(np.int32) if key.size else np.zeros((0, 2), np.int32)
    return spans, np.searchsorted(p, np.arange(N_PITCH + 1), side="left").astype(np.int64)


def column_grid(start_time: float, end_time: float, fs: float) -> np.ndarray:
    """pretty_midi's column boundaries for midi.chunk_roll: round(linspace(start, end, int((end - start) * fs)) * fs)."""
    times = np.linspace(start_time, end_time, int((end_time - start_time) * fs))
    return np.array(np.round(np.asarray(times, dtype=np.float64) * fs), dtype=np.int64)


def roll_from_spans(spans: np.ndarray, pitch_off: np.ndarray, t_keep: int, cols: Optional[np.ndarray]) -> np.ndarray:
    """Host rendering of mt_roll_windows' rule for one window (tests / documentation): (88, t_keep) float32 {0, 1}."""
    out = np.zeros((N_PITCH, t_keep), np.float32)
    if cols is None:
        s = np.arange(t_keep)
        e = s + 1
        valid = np.ones(t_keep, bool)
    else:
        n = np.arange(t_keep)
        valid = n + 1 < len(cols)
        s = np.where(valid, cols[np.minimum(n, len(cols) - 1)], 0)
        e = np.where(valid, cols[np.minimum(n + 1, len(cols) - 1)], 0)
        e = np.where(e == s, s + 1, e)
    for p in range(N_PITCH):
        sp = spans[pitch_off[p]:pitch_off[p + 1]]
        if not len(sp):
            continue
        k = np.searchsorted(sp[:, 1], s, side="right")               # first span with v > s
        hit = (k < len(sp)) & (sp[np.minimum(k, len(sp) - 1), 0] < e)
        out[p] = (valid & hit).astype(np.float32)
    return out


# ------------------------------------------------------------------ augmentation
AUG_TAPS, AUG_PHASES, AUG_BETA = 32, 256, 10.0
AUG_MAX_DEV = 0.03           # mt_augment_windows takes speeds within 1 +- 0.03 (50 cents = 1.0293)
_ONE_Q32 = 1 << 32


def augment_table(beta: float = AUG_BETA) -> np.ndarray:
    """mt_augment_windows' interpolation table, float64 (AUG_PHASES + 1, AUG_TAPS): tab[ph][j] = sinc(t) * kaiser_beta(t / 16) at
    t = j - 15 - ph / P (a full-band sinc, no cutoff narrowing), every row normalised to unit sum, rows 0 and P exact unit
    impulses at taps 15 and 16 (speed 1 copies the window).  The device holds it as float32."""
    half = AUG_TAPS // 2
    ph = np.arange(AUG_PHASES + 1, dtype=np.float64)[:, None] / AUG_PHASES
    t = np.arange(AUG_TAPS, dtype=np.float64)[None, :] - (half - 1) - ph
    u = np.clip(1.0 - (t / half) ** 2, 0.0, None)
    tab = np.sinc(t) * np.i0(beta * np.sqrt(u)) / np.i0(beta)
    tab /= tab.sum(axis=1, keepdims=True)
    tab[0] = 0.0
    tab[0, half - 1] = 1.0
    tab[AUG_PHASES] = 0.0
    tab[AUG_PHASES, half] = 1.0
    return tab


def augmented_cols(start_time: float, end_time: float, fs: float, rate_q32: int) -> np.ndarray:
    """column_grid for a window played at speed r = rate_q32 / 2^32: output time t0 + d shows source time t0 + r * d, so column
    n samples source frame round((t0 + r * (times[n] - t0)) * fs), in float64.  r = 1 is column_grid itself."""
    if int(rate_q32) == _ONE_Q32:
        return column_grid(start_time, end_time, fs)
    times = np.asarray(np.linspace(start_time, end_time, int((end_time - start_time) * fs)), dtype=np.float64)
    r = float(int(rate_q32)) / float(_ONE_Q32)
    return np.array(np.round((start_time + r * (times - start_time)) * fs), dtype=np.int64)


class Augment:
    """Per-window training augmentation of MaestroDataset's chunks, on the GPU (csrc/augment.hip):
      * pitch_cents c: each window is played at speed 2^(cents / 1200), cents ~ U(-c, c) -- pitch and tempo move together and the
        labels' columns move with the audio.  0 <= c <= 50, so no note leaves its semitone and the label rows stay what they are;
      * snr_db (lo, hi) or None: white noise at a signal-to-noise ratio ~ U(lo, hi) dB against the window's own power.
    Draws come from `generator` (a CPU torch.Generator; a fresh default-seeded one when None).  A level change is not offered:
    the mel is normalised to the chunk maximum and clamped 80 dB under it, so gain is invisible to the model."""

    def __init__(self, pitch_cents: float = 10.0, snr_db=None, generator: Optional[torch.Generator] = None):
        pitch_cents = float(pitch_cents)
        if not 0.0 <= pitch_cents <= 50.0:
            raise ValueError(f"Augment: pitch_cents must be in [0, 50] (the labels' pitches never change), got {pitch_cents}")
        if snr_db is not None:
            try:
                lo, hi = (float(v) for v in snr_db)
            except (TypeError, ValueError):
                raise ValueError(f"Augment: snr_db must be None or a (lo, hi) pair in dB, got {snr_db!r}") from None
            if not 0.0 <= lo <= hi:
                raise ValueError(f"Augment: snr_db needs 0 <= lo <= hi, got ({lo}, {hi})")
            snr_db = (lo, hi)
        self.pitch_cents, self.snr_db = pitch_cents, snr_db
        self.generator = generator if generator is not None else torch.Generator()

    def draw(self, n: int):
        """The draws of one batch of n windows: (rate_q32 uint64 (n,), snr_db float64 (n,) -- NaN without noise --, seed < 2^31).
        Order of the generator's use: n cents, n SNRs (only with snr_db), one seed."""
        g = self.generator
        cents = (torch.rand(n, dtype=torch.float64, generator=g).numpy() * 2.0 - 1.0) * self.pitch_cents
        rate = np.rint(np.exp2(cents / 1200.0) * float(_ONE_Q32)).astype(np.uint64)
        if self.snr_db is not None:
            lo, hi = self.snr_db
            snr = lo + (hi - lo) * torch.rand(n, dtype=torch.float64, generator=g).numpy()
        else:
            snr = np.full(n, np.nan)
        seed = int(torch.randint(0, 1 << 31, (1,), generator=g).item())
        return rate, snr, seed


# ------------------------------------------------------------------ audio
class RecordingStore:
    """Decoded recordings in one f32 device buffer (64-bit offsets), LRU of whole recordings when over budget."""

    def __init__(self, paths: Sequence[str], sr: int, device, est_samples: Sequence[int], max_resident_bytes: Optional[int] = None):
        self.paths, self.sr, self.device = list(paths), int(sr), torch.device(device)
        if max_resident_bytes is None:
            max_resident_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        want = sum(int(n) + 2 * _ALIGN for n in est_samples)
        self.capacity = int(min(int(max_resident_bytes) // 4, want))
        self.capacity -= self.capacity % _ALIGN
        self.buf = torch.zeros(self.capacity + _PAD, dtype=torch.float32, device=self.device)
        self.n = [0] * len(self.paths)                      # decoded samples per recording
        self.loc: "OrderedDict[int, int]" = OrderedDict()  # resident recording -> offset (LRU order, most recent last)
        self.decodes = 0
        self._warned = False
        for r in range(len(self.paths)):
            self._load(r, ())

    @property
    def resident_bytes(self) -> int:
        return sum(self.n[r] for r in self.loc) * 4

    def _load(self, r: int, pinned) -> None:
        y = load_audio_device(self.paths[r], self.sr, self.device)
        self.decodes += 1
        n = int(y.numel())
        self.n[r] = n
        off = self._alloc(n, pinned)
        self.buf[off:off + n].copy_(y)
        self.loc[r] = off

    def _alloc(self, n: int, pinned) -> int:
        need = -(-max(n, 1) // _ALIGN) * _ALIGN
        if need > self.capacity:
            raise RuntimeError(f"RecordingStore: a recording of {n} samples exceeds max_resident_bytes ({self.capacity * 4} B)")
        while True:
            pos = 0                                         # first fit between the resident recordings
            for off, r in sorted((o, k) for k, o in self.loc.items()):
                if off - pos >= need:
                    return pos
                pos = off + -(-max(self.n[r], 1) // _ALIGN) * _ALIGN
            if self.capacity - pos >= need:
                return pos
            victim = next((k for k in self.loc if k not in pinned), None)
            if victim is None:
                raise _NoRoom()
            if not self._warned:
                warnings.warn(f"RecordingStore: the split does not fit in max_resident_bytes ({self.capacity * 4} B); evicted recordings "
                              f"are decoded again when a batch needs them (same data, slower)", RuntimeWarning, stacklevel=4)
                self._warned = True
            del self.loc[victim]

    def offsets(self, recs: Sequence[int]) -> Dict[int, int]:
        """Make `recs` resident (together) and return their offsets in `buf` (floats).  When the free space around the
        batch's resident recordings is too fragmented, the store is emptied and the batch's recordings are loaded side by side."""
        pinned = sorted(set(int(r) for r in recs))
        try:
            for r in pinned:
                if r in self.loc:
                    self.loc.move_to_end(r)
                else:
                    self._load(r, pinned)
        except _NoRoom:
            self.loc.clear()
            try:
                for r in pinned:
                    self._load(r, pinned)
            except _NoRoom:
                raise RuntimeError(f"RecordingStore: max_resident_bytes ({self.capacity * 4} B) cannot hold the recordings of one batch") from None
        return {r: self.loc[r] for r in pinned}


class _NoRoom(Exception):
    pass


def _in_worker() -> bool:
    return torch.utils.data.get_worker_info() is not None


# ------------------------------------------------------------------ datasets
class MaestroDataset(Dataset):
    """The reference's MaestroDataset (same arguments; items (mel (1, n_mels, T), roll (88, T)) CPU tensors, the bytes
    preprocess_and_cache writes for the same chunk), built on the device.  get_batch(indices) gives collate_fn's batch with
    mel and roll on the device in one launch of each kernel; DeviceBatchLoader is the DataLoader for it.  chunk_length=None:
    one item per recording (whole file).

    onset_labels="midi" keeps every recording's note list (label_notes) on the device as well: get_batch then returns the
    labels as {"frame": roll, "onset": onset_roll}, the onset roll marking the MIDI note-ons (re-struck keys included) on
    the roll's column grid, and ref_notes(indices) gives the note lists notes.note_match_list scores against.  The default
    "roll" builds neither table and returns what it always did.

    onset_target="regress" (with onset_labels="midi") replaces the onset roll by a regression target (mt_onset_regress_windows,
    DESIGN.md 6c "Sub-frame onsets"): a triangle of half-width onset_width frames (2..8) around every note-on, measured from the
    centre of the mel's own frame t (sample 512 t of the window), so that the head's values around a peak tell where inside the
    frame the key went down.  No column table is involved: for chunk items the point target inherits the reference's stretched
    column grid, the regression target does not.  Under augmentation the frame centres are mapped to source time with the
    window's speed; the triangle's width is kept in source time, hence up to 3 % narrower or wider in mel frames.  The default
    "point" is the onset roll above, launch for launch."""

    def __init__(self, root_dir, csv_path=None, year=None, split="train", sr=16000, n_mels=229, hop_length=512, subset_size=None,
                 chunk_length=None, overlap=0.0, return_waveform=False, device=None, max_resident_bytes=None, onset_labels="roll",
                 augment=None, onset_target="point", onset_width=2):
        if return_waveform:
            raise NotImplementedError("return_waveform=True is the AST experiment's data path (out of scope)")
        if onset_labels not in ("roll", "midi"):
            raise ValueError(f"onset_labels must be 'roll' or 'midi', got {onset_labels!r}")
        if onset_target not in ("point", "regress"):
            raise ValueError(f"onset_target must be 'point' or 'regress', got {onset_target!r}")
        if onset_target == "regress":
            if onset_labels != "midi":
                raise ValueError("onset_target='regress' is built from the MIDI note-ons: it needs onset_labels='midi'")
            if isinstance(onset_width, bool) or not isinstance(onset_width, (int, np.integer)) \
                    or not ONSET_WIDTH_RANGE[0] <= onset_width <= ONSET_WIDTH_RANGE[1]:
                raise ValueError(f"onset_width must be an integer number of frames in [{ONSET_WIDTH_RANGE[0]}, {ONSET_WIDTH_RANGE[1]}] (at 1 the "
                                 f"triangle's side values clamp at 0 and the sub-frame time cannot be recovered), got {onset_width!r}")
            if int(hop_length) * TICKS_PER_SECOND != TICKS_PER_FRAME * int(sr):
                raise ValueError(f"onset_target='regress': the target is computed in exact units of 12.5 us on the grid of {TICKS_PER_FRAME} "
                                 f"ticks per frame (sr 16000, hop 512); got sr {sr}, hop {hop_length}")
        self.onset_target, self.onset_width = onset_target, int(onset_width)
        if augment is not None:
            if not isinstance(augment, Augment):
                raise TypeError(f"augment must be an Augment or None, got {type(augment).__name__}")
            if chunk_length is None:
                raise ValueError("MaestroDataset: augment needs chunk_length (whole-file items have no column table to move the "
                                 "labels with the audio, and augmentation is a training feature)")
        self.onset_labels, self.augment, self.last_augment = onset_labels, augment, None
        self._aug_tab = None                                # mt_augment_windows' phase table, uploaded with the first augmented batch
        self.root_dir, self.sr, self.n_mels, self.hop_length = root_dir, int(sr), int(n_mels), int(hop_length)
        self.chunk_length, self.overlap, self.return_waveform = chunk_length, overlap, return_waveform
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.rows = read_maestro_csv(root_dir, split, year, subset_size, csv_path)
        paths = [os.path.join(root_dir, r["audio_filename"]) for r in self.rows]
        durations = [wav_duration(p) for p in paths]
        self.chunks = build_chunk_index(durations, chunk_length, overlap, self.sr) if chunk_length is not None else []
        fs = self.sr / self.hop_length
        self.store = RecordingStore(paths, self.sr, self.device, [int(np.ceil(d * self.sr)) + 1 for d in durations], max_resident_bytes)
        # labels: span tables of every recording, one device array
        spans, poffs, fullw, notes, base = [], [], [], [], 0
        tables = []                                         # onset_labels="midi": every recording's NoteTable
        for r in self.rows:
            midi = MidiFile(os.path.join(root_dir, r["midi_filename"]))
            sp, po, fw, hn = label_spans(midi, fs)
            if onset_labels == "midi":
                tables.append(label_notes(midi, fs))
            spans.append(sp)
            poffs.append(po + base)
            fullw.append(fw)
            notes.append(hn)
            base += len(sp)
        n_rec = np.array(self.store.n, dtype=np.int64)
        if chunk_length is not None:
            c = self.chunks
            self.rec = np.array([x["file_idx"] for x in c], dtype=np.int64)
            self.start = np.array([x["start_sample"] for x in c], dtype=np.int64)
            self.win_len = np.array([x["end_sample"] - x["start_sample"] for x in c], dtype=np.int64)
            self.chunk_t0 = np.array([x["start_time"] for x in c], dtype=np.float64)
            self.chunk_t1 = np.array([x["end_time"] for x in c], dtype=np.float64)
            grids = [column_grid(x["start_time"], x["end_time"], fs) for x in c]
            self.ncols = np.array([len(g) for g in grids], dtype=np.int64)
            self.col_off = np.concatenate([[0], np.cumsum(self.ncols)[:-1]]).astype(np.int64) if c else np.zeros(0, np.int64)
            roll_w = np.where(np.array([notes[f] for f in self.rec], dtype=bool), self.ncols, 0) if c else np.zeros(0, np.int64)
            cols = np.concatenate(grids).astype(np.int32) if grids and self.ncols.sum() else np.zeros(1, np.int32)
        else:
            self.rec = np.arange(len(self.rows), dtype=np.int64)
            self.start = np.zeros(len(self.rows), dtype=np.int64)
            self.win_len = n_rec.copy()
            self.ncols = np.zeros(len(self.rows), dtype=np.int64)
            self.col_off = np.full(len(self.rows), -1, dtype=np.int64)
            roll_w = np.array([fw if hn else 0 for fw, hn in zip(fullw, notes)], dtype=np.int64)
            cols = np.zeros(1, np.int32)
        self.t_keep = np.minimum(1 + self.win_len // self.hop_length, roll_w).astype(np.int64)
        if self.win_len.size and int(self.win_len.max()) * 4 + 8 >= 0x7FFFFFFF:
            raise ValueError("MaestroDataset: a window longer than 2^29 samples")
        dev = self.device
        sp_all = np.concatenate(spans) if base else np.zeros((1, 2), np.int32)
        self.spans = torch.from_numpy(np.ascontiguousarray(sp_all, dtype=np.int32)).to(dev)
        self.pitch_off = torch.from_numpy(np.concatenate(poffs) if poffs else np.zeros(N_PITCH + 1, np.int64)).to(dev)
        self.cols = torch.from_numpy(cols).to(dev)
        self.fe = get_frontend(self.sr, self.n_mels, self.hop_length, dev)
        if onset_labels == "midi":
            self._upload_note_tables(tables)

    def _upload_note_tables(self, tables) -> None:
        """Note-on point spans of every recording for mt_roll_windows (the layout of spans / pitch_off), and for whole-file items
        the note lists in ticks, cut to each item's frames: notes with on_tick < 320 * t_keep, offsets clipped to it."""
        dev, on_sp, on_po, base = self.device, [], [], 0
        for nt in tables:
            sp, po = onset_spans(nt)
            on_sp.append(sp)
            on_po.append(po + base)
            base += len(sp)
        sp_all = np.concatenate(on_sp) if base else np.zeros((1, 2), np.int32)
        self.onset_spans = torch.from_numpy(np.ascontiguousarray(sp_all, dtype=np.int32)).to(dev)
        self.onset_pitch_off = torch.from_numpy(np.concatenate(on_po) if on_po else np.zeros(N_PITCH + 1, np.int64)).to(dev)
        if self.onset_target == "regress":                  # every note-on in ticks, in the layout of onset_pitch_off
            ticks = np.concatenate([nt.on_tick for nt in tables]) if tables else np.zeros(0, np.int32)
            bases = np.concatenate([[0], np.cumsum([len(nt.on_tick) for nt in tables])]).astype(np.int64)
            t_off = np.concatenate([nt.pitch_off + b for nt, b in zip(tables, bases)]) if tables else np.zeros(N_PITCH + 1, np.int64)
            self.onset_ticks = torch.from_numpy(np.ascontiguousarray(ticks if ticks.size else np.zeros(1), dtype=np.int32)).to(dev)
            self.onset_tick_off = torch.from_numpy(np.ascontiguousarray(t_off, dtype=np.int64)).to(dev)
        if self.chunk_length is not None:
            return
        if self.hop_length * TICKS_PER_SECOND != TICKS_PER_FRAME * self.sr:
            raise ValueError(f"onset_labels='midi': note lists are kept on the grid of {TICKS_PER_FRAME} ticks per frame "
                             f"(sr 16000, hop 512); got sr {self.sr}, hop {self.hop_length}")
        ons, offs, ptrs, self.note_base = [], [], [], [0]
        for nt, t in zip(tables, self.t_keep):
            end = TICKS_PER_FRAME * int(t)
            keep = nt.on_tick < end
            rows = np.repeat(np.arange(N_PITCH), np.diff(nt.pitch_off))[keep]
            ons.append(nt.on_tick[keep])
            offs.append(np.minimum(nt.off_tick[keep], end))
            ptrs.append(np.searchsorted(rows, np.arange(N_PITCH), side="left").astype(np.int64))      # 88 row starts, item-local
            self.note_base.append(self.note_base[-1] + int(keep.sum()))
        cat = lambda xs, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0), dtype=dt)).to(dev)
        self.note_on, self.note_off, self.note_ptr = cat(ons, np.int32), cat(offs, np.int32), cat(ptrs, np.int64)

    def ref_notes(self, indices) -> Dict[str, torch.Tensor]:
        """The reference notes of whole-file items for notes.note_match_list: {"on", "off"} int32 ticks of 100 us and "ptr" int64
        (len(indices) * 88 + 1,), on the device -- row (b, p) owns on/off[ptr[b*88 + p]:ptr[b*88 + p + 1]], sorted by onset;
        notes with on_tick < 320 * t_keep, offsets clipped to 320 * t_keep.  Device slices of the tables uploaded at construction."""
        if self.onset_labels != "midi":
            raise RuntimeError("ref_notes needs a dataset built with onset_labels='midi'")
        if self.chunk_length is not None:
            raise NotImplementedError("ref_notes: note lists are kept for whole recordings only (chunk_length=None; the scripts' "
                                      "--data_source full)")
        idx = [int(i) for i in indices]
        on, off, ptr, acc = [], [], [], 0
        for i in idx:
            lo, hi = self.note_base[i], self.note_base[i + 1]
            on.append(self.note_on[lo:hi])
            off.append(self.note_off[lo:hi])
            ptr.append(self.note_ptr[i * N_PITCH:(i + 1) * N_PITCH] + acc)
            acc += hi - lo
        ptr.append(torch.full((1,), acc, dtype=torch.int64, device=self.device))
        return {"on": torch.cat(on) if on else self.note_on[:0], "off": torch.cat(off) if off else self.note_off[:0], "ptr": torch.cat(ptr)}

    def __len__(self):
        return len(self.rec)

    @property
    def num_frames(self) -> np.ndarray:
        """Frames of every item (the T of its mel and roll)."""
        return self.t_keep

    def get_batch(self, indices):
        """collate_fn([self[i] for i in indices]) with mel (B, 1, n_mels, T) and roll (B, 88, T) on the device and lengths
        (int64) on the host, as the loss reads them.  Window tables go up in one pinned copy each; nothing comes back."""
        if _in_worker():
            raise RuntimeError("MaestroDataset builds batches on the GPU and cannot run in a DataLoader worker process: "
                               "use DeviceBatchLoader, or a DataLoader with num_workers=0")
        idx = np.asarray(list(indices), dtype=np.int64)
        B = len(idx)
        if B == 0:
            raise ValueError("get_batch: empty batch")
        if self.augment is not None:
            return self._get_batch_augmented(idx)
        recs = self.rec[idx]
        offs = self.store.offsets(recs.tolist())
        n_rec = np.array(self.store.n, dtype=np.int64)
        t_keep = self.t_keep[idx]
        T_out = int(t_keep.max())
        h64 = torch.empty((2, B), dtype=torch.int64, pin_memory=True)
        h64[0] = torch.from_numpy(np.array([offs[int(r)] for r in recs], dtype=np.int64) + self.start[idx])
        h64[1] = torch.from_numpy(self.col_off[idx])
        h32 = torch.empty((6, B), dtype=torch.int32, pin_memory=True)
        h32.copy_(torch.from_numpy(np.stack([self.win_len[idx], n_rec[recs] - self.start[idx], t_keep, recs, self.ncols[idx],
                                             self.start[idx]])))
        dev = self.device
        with torch.cuda.device(dev):
            d64, d32 = h64.to(dev, non_blocking=True), h32.to(dev, non_blocking=True)
            mel = torch.empty(B, 1, self.n_mels, T_out, dtype=torch.float32, device=dev)
            cmax = torch.empty(B, dtype=torch.float32, device=dev)
            roll = torch.empty(B, N_PITCH, T_out, dtype=torch.float32, device=dev)
            st = _lib.stream_ptr()
            check(lib.mt_mel_db_windows_f32(ptr(self.fe.plan), self.fe.desc, ptr(self.store.buf), ptr(d64[0]), ptr(d32[0]), ptr(d32[1]), B,
                                            int(self.win_len[idx].max()), T_out, ptr(d32[2]), ptr(mel), ptr(cmax), st), "mt_mel_db_windows_f32")
            check(lib.mt_roll_windows(ptr(self.spans), ptr(self.pitch_off), ptr(self.cols), ptr(d32[3]), ptr(d64[1]), ptr(d32[4]), ptr(d32[2]),
                                      B, T_out, ptr(roll), st), "mt_roll_windows")
            if self.onset_target == "regress":              # triangles around the note-ons, measured from the mel's frame centres
                return mel, {"frame": roll, "onset": self._onset_regress(d32[3], d32[5], None, d32[2], B, T_out, st)}, \
                    torch.from_numpy(t_keep.copy())
            if self.onset_labels == "midi":                 # the note-ons on the same columns: point spans through the same kernel
                onset_roll = torch.empty_like(roll)
                check(lib.mt_roll_windows(ptr(self.onset_spans), ptr(self.onset_pitch_off), ptr(self.cols), ptr(d32[3]), ptr(d64[1]),
                                          ptr(d32[4]), ptr(d32[2]), B, T_out, ptr(onset_roll), st), "mt_roll_windows")
                return mel, {"frame": roll, "onset": onset_roll}, torch.from_numpy(t_keep.copy())
        return mel, roll, torch.from_numpy(t_keep.copy())

    def _get_batch_augmented(self, idx):
        """get_batch with self.augment: mt_augment_windows writes the batch's windows, speed-changed and noised, into a dense
        (B, L_max) buffer; mt_mel_db_windows_f32 reads that buffer as its store; the labels go through a column table built
        for this batch's speeds (augmented_cols).  t_keep and T_out are those of the plain batch.  The draws stay in
        self.last_augment = {"rate_q32" uint64 (B,), "snr_db" float64 (B,) (NaN: no noise), "seed" uint32 ()}."""
        B, aug, dev = len(idx), self.augment, self.device
        rate, snr, seed = aug.draw(B)
        rate = np.ascontiguousarray(rate, dtype=np.uint64)
        snr = np.ascontiguousarray(snr, dtype=np.float64)
        if rate.shape != (B,) or snr.shape != (B,) or abs(int(rate.min()) - _ONE_Q32) > int(AUG_MAX_DEV * _ONE_Q32) \
                or abs(int(rate.max()) - _ONE_Q32) > int(AUG_MAX_DEV * _ONE_Q32):
            raise ValueError(f"Augment.draw: {B} speeds within 1 +- {AUG_MAX_DEV} expected")
        self.last_augment = {"rate_q32": rate.copy(), "snr_db": snr.copy(), "seed": np.array(seed, dtype=np.uint32)}
        noisy = bool(np.isfinite(snr).any())
        recs = self.rec[idx]
        offs = self.store.offsets(recs.tolist())
        n_rec = np.array(self.store.n, dtype=np.int64)
        t_keep, win_len = self.t_keep[idx], self.win_len[idx]
        T_out = int(t_keep.max())
        L_max = -(-int(win_len.max()) // 4) * 4
        fs = self.sr / self.hop_length
        grids = [augmented_cols(self.chunk_t0[i], self.chunk_t1[i], fs, int(r)) for i, r in zip(idx, rate)]
        ncols = np.array([len(g) for g in grids], dtype=np.int64)
        cols = np.concatenate(grids).astype(np.int32) if ncols.sum() else np.zeros(1, np.int32)
        h64 = torch.empty((4, B), dtype=torch.int64, pin_memory=True)
        h64.copy_(torch.from_numpy(np.stack([np.array([offs[int(r)] for r in recs], dtype=np.int64) + self.start[idx],
                                             np.concatenate([[0], np.cumsum(ncols)[:-1]]).astype(np.int64),
                                             np.arange(B, dtype=np.int64) * L_max, rate.view(np.int64)])))
        noise_rel = np.where(np.isfinite(snr), 10.0 ** (-np.nan_to_num(snr) / 20.0), 0.0).astype(np.float32)
        h32 = torch.empty((7, B), dtype=torch.int32, pin_memory=True)
        h32.copy_(torch.from_numpy(np.stack([win_len, n_rec[recs] - self.start[idx], t_keep, recs, ncols, self.start[idx],
                                             noise_rel.view(np.int32).astype(np.int64)])))
        hcols = torch.from_numpy(cols).pin_memory()
        if self._aug_tab is None:
            self._aug_tab = torch.from_numpy(augment_table().astype(np.float32)).to(dev)
        with torch.cuda.device(dev):
            d64, d32, dcols = h64.to(dev, non_blocking=True), h32.to(dev, non_blocking=True), hcols.to(dev, non_blocking=True)
            wave = torch.empty(B * L_max, dtype=torch.float32, device=dev)
            ws_bytes = int(lib.mt_augment_ws_bytes(B, L_max)) if noisy else 0
            ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev) if noisy else None
            mel = torch.empty(B, 1, self.n_mels, T_out, dtype=torch.float32, device=dev)
            cmax = torch.empty(B, dtype=torch.float32, device=dev)
            roll = torch.empty(B, N_PITCH, T_out, dtype=torch.float32, device=dev)
            st = _lib.stream_ptr()
            check(lib.mt_augment_windows(ptr(self.store.buf), ptr(d64[0]), ptr(d32[0]), ptr(d32[5]), ptr(d32[1]), ptr(d64[3]), int(rate.min()),
                                         int(rate.max()), ptr(d32[6]) if noisy else None, seed, ptr(self._aug_tab), B, L_max, ptr(wave), ptr(ws),
                                         ws_bytes, st), "mt_augment_windows")
            check(lib.mt_mel_db_windows_f32(ptr(self.fe.plan), self.fe.desc, ptr(wave), ptr(d64[2]), ptr(d32[0]), ptr(d32[0]), B,
                                            int(win_len.max()), T_out, ptr(d32[2]), ptr(mel), ptr(cmax), st), "mt_mel_db_windows_f32")
            check(lib.mt_roll_windows(ptr(self.spans), ptr(self.pitch_off), ptr(dcols), ptr(d32[3]), ptr(d64[1]), ptr(d32[4]), ptr(d32[2]),
                                      B, T_out, ptr(roll), st), "mt_roll_windows")
            if self.onset_target == "regress":              # frame centres in source time: the batch's own speeds
                return mel, {"frame": roll, "onset": self._onset_regress(d32[3], d32[5], d64[3], d32[2], B, T_out, st)}, \
                    torch.from_numpy(t_keep.copy())
            if self.onset_labels == "midi":
                onset_roll = torch.empty_like(roll)
                check(lib.mt_roll_windows(ptr(self.onset_spans), ptr(self.onset_pitch_off), ptr(dcols), ptr(d32[3]), ptr(d64[1]),
                                          ptr(d32[4]), ptr(d32[2]), B, T_out, ptr(onset_roll), st), "mt_roll_windows")
                return mel, {"frame": roll, "onset": onset_roll}, torch.from_numpy(t_keep.copy())
        return mel, roll, torch.from_numpy(t_keep.copy())

    def _onset_regress(self, win_rec, start, rate_q32, t_keep, B, T_out, st) -> torch.Tensor:
        """mt_onset_regress_windows on the batch's device tables (start: each window's first sample inside its recording)."""
        y = torch.empty(B, N_PITCH, T_out, dtype=torch.float32, device=self.device)
        check(lib.mt_onset_regress_windows(ptr(self.onset_ticks), ptr(self.onset_tick_off), ptr(win_rec), ptr(start), ptr(rate_q32), ptr(t_keep),
                                           B, T_out, self.onset_width, ptr(y), st), "mt_onset_regress_windows")
        return y

    def __getitem__(self, idx):
        if _in_worker():
            raise RuntimeError("MaestroDataset items are built on the GPU and cannot be read in a DataLoader worker process "
                               "(the reference's loaders use 8): use DeviceBatchLoader, or a DataLoader with num_workers=0")
        mel, roll, _ = self.get_batch([idx])
        if isinstance(roll, dict):                          # items keep the reference's (mel, roll) shape; the onset roll is a batch label
            roll = roll["frame"]
        return mel[0].cpu(), roll[0].cpu()


class HybridMaestroDataset(Dataset):
    """data/cached_dataset.py:91-141: the cache when its metadata's chunk_length and overlap equal the request, else MaestroDataset.
    A request with `augment` never uses the cache: its records hold features, and augmentation works on the waveform.  Nor does
    one with onset_target="regress": the cache holds rolls, and the regression target is built from the MIDI note-ons."""

    def __init__(self, root_dir, cache_dir="cached_dataset", split="train", chunk_length=None, overlap=0.0, augment=None,
                 onset_target="point", onset_width=2, **kwargs):
        from .data import CachedMaestroDataset
        self.use_cache = False
        if augment is not None:
            kwargs["augment"] = augment
        if onset_target != "point":
            kwargs["onset_target"], kwargs["onset_width"] = onset_target, onset_width
        try:
            metadata_path = os.path.join(cache_dir, f"{split}_metadata.pkl")
            if augment is None and onset_target == "point" and os.path.exists(metadata_path):
                with open(metadata_path, "rb") as f:
                    metadata = pickle.load(f)
                if metadata.get("chunk_length") == chunk_length and metadata.get("overlap") == overlap:
                    self.cached_dataset = CachedMaestroDataset(cache_dir, split)
                    self.use_cache = True
                    print("✓ Using cached dataset (fast mode!)")
                    return
        except Exception:
            pass
        self.dataset = MaestroDataset(root_dir=root_dir, split=split, chunk_length=chunk_length, overlap=overlap, **kwargs)
        print("⚠ Using raw dataset (slow mode). Run preprocess_dataset.py for 10-50x speedup!")

    def __len__(self):
        return len(self.cached_dataset) if self.use_cache else len(self.dataset)

    def __getitem__(self, idx):
        return self.cached_dataset[idx] if self.use_cache else self.dataset[idx]

    def get_batch(self, indices):
        if self.use_cache:
            from .data import collate_fn
            return collate_fn([self.cached_dataset[i] for i in indices])
        return self.dataset.get_batch(indices)


class DeviceBatchLoader:
    """DataLoader(dataset, batch_size, shuffle, sampler, drop_last, generator, collate_fn=collate_fn) for a dataset with
    get_batch: the same index batches in the same order (the iterator draws the DataLoader's base seed first, so the global
    RNG advances as it would), each built by one get_batch call in this process.  Works with DistributedSampler."""

    def __init__(self, dataset, batch_size=1, shuffle=False, sampler=None, drop_last=False, generator=None):
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        self.dataset, self.batch_size, self.drop_last, self.generator = dataset, batch_size, drop_last, generator
        if sampler is None:
            sampler = RandomSampler(dataset, generator=generator) if shuffle else SequentialSampler(dataset)
        self.sampler = sampler
        self.batch_sampler = BatchSampler(sampler, batch_size, drop_last)

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)      # DataLoader's _base_seed draw
        for indices in self.batch_sampler:
            yield self.dataset.get_batch(indices)
