"""Offline transcription of a whole corpus on ONE rank's shard (BASELINE.json configs[4]).

The reference transcribes a recording as a Python loop over its 30 s chunks, batch 1 (main.py:229-362).  Chunks keep no
cross-chunk state (main.py:258-266), so here they are batched ACROSS recordings: the shard's chunks are streamed in slabs of
`batch` chunks -- a slab is assembled as soon as enough recordings have been decoded, never the whole shard first -- and slab f
runs mel + forward on stream f % streams.  Per recording the device then turns its logits into notes (threshold + chunk
concatenation + per-pitch run-length: mt_roll_to_notes, main.py:153-226), so what crosses PCIe per recording is its note list
(two ints per note), not its piano roll; framewise F1 against a reference roll, when one is given, is computed on the device too.

`transcribe_shard_windows` is the same job on the window grid of windows.py: whole recordings in overlapping 30 s
windows on one frame grid, grouped so that a group's stitched logits are one padded batch with lengths; notes and scores of a
group leave the device together (notes.notes_batch_device), not recording by recording.
"""
from __future__ import annotations

import time
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import transcribe as tr
from . import windows as W
from .frontend import get_frontend
from .notes import check_cleanup, check_smoothing, heads_to_notes_device, note_match_counts, note_prf, notes_batch_device
from .ops import f1_counts, f1_from_counts, framewise_f1, predict_from_logits

SR, CH, HOP = 16000, 480000, 512


def _check_corpus_decoder(decoder: str) -> None:
    """The corpus paths decode with the frame or the onset-gated decoder only: say so for the offset-gated one, instead of falling
    back to the frame decoder without a word."""
    if decoder == "onset_offset":
        raise ValueError("decoder='onset_offset' is not available in corpus transcription (its batched note extractor reads two heads): "
                         "use 'frame' or 'onset' here, or transcribe.transcribe_audio for the offset-gated decoder")


@torch.no_grad()
def transcribe_shard(model, rec_ids: Sequence[int], chunks_of: Callable[[int], torch.Tensor], *, n_mels: int, device,
                     batch: int = 128, streams: int = 3, threshold: float = 0.5, want_notes: bool = True,
                     reference_roll_of: Optional[Callable[[int, int], Optional[torch.Tensor]]] = None,
                     midi_path_of: Optional[Callable[[int], Optional[str]]] = None, warm: bool = True, decoder: str = "frame",
                     onset_threshold: float = 0.5, note_metrics: bool = False, min_note_frames: int = 1,
                     bridge_frames: int = 0, smooth_on: float = 0.0, smooth_off: float = 0.0, onset_detect: str = "edge",
                     peak_reach: int = 1) -> Dict[str, object]:
    """rec_ids: the recordings of this rank; chunks_of(i) -> (n_i, 480000) float32 CUDA tensor (decode + resample + split for
    real audio: part of the measured time; a view of resident synthetic audio otherwise).  Returns {"wall_s", "chunks",
    "notes": {i: [(pitch, start, end)]}, "f1": {i: float}, "n_notes", "finite"}; wall_s covers slab assembly, every forward,
    the note extraction and the F1 counts (one device synchronisation at the end).  decoder="onset": notes from the onset-gated
    decoder (notes.heads_to_notes_device; cnn_rnn_large with heads only).  note_metrics=True with reference rolls: "note_f1" =
    {i: (onset F1, onset+offset F1)} against the runs of the reference roll, estimated notes from the same decoder.
    min_note_frames / bridge_frames: note cleanup in the decoder (DESIGN.md 6c "Note cleanup"), for the notes and for note_f1 alike.
    smooth_on / smooth_off: frame smoothing before the decoder (DESIGN.md 6c "Frame smoothing"), over the recording's chunks
    concatenated in time, for the notes and for note_f1 alike; the framewise "f1" stays the raw threshold's.  (0, 0): none.
    onset_detect="peak" (decoder="onset"): notes open at the peaks of the onset logits over peak_reach frames (DESIGN.md 6c "Peak-picked
    onsets"), for the notes and for note_f1 alike."""
    _check_corpus_decoder(decoder)
    tr.check_decoder(decoder, model=model)
    tr.check_detect_decoder(onset_detect, decoder, peak_reach)
    clean = dict(zip(("min_note_frames", "bridge_frames"), check_cleanup(min_note_frames, bridge_frames)))
    clean.update(zip(("smooth_on", "smooth_off"), check_smoothing(smooth_on, smooth_off)))
    heads = decoder == "onset"
    if heads:                                    # (the frame decoder's calls have no onset head and take neither)
        clean.update(onset_detect=onset_detect, peak_reach=int(peak_reach))
    dev = torch.device(device)
    net = model.model
    fe = get_frontend(SR, n_mels, HOP, str(dev))
    NS = max(1, streams)
    side = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    main = torch.cuda.current_stream(dev)
    if warm:                                     # weight packing, code objects, every stream's workspace: not part of wall_s
        w0 = torch.zeros(batch, CH, device=dev)
        torch.cuda.synchronize(dev)
        for st in side:
            with torch.cuda.stream(st):
                m0, c0 = fe(w0, clamp=False)
                net(m0, chunk_max_power=c0)
        torch.cuda.synchronize(dev)
        del w0
    spans_n: Dict[int, int] = {}
    t0 = time.perf_counter()
    pending: List[torch.Tensor] = []             # decoded chunks not yet in a slab
    n_pending, n_slabs = 0, 0
    # Logits are held PER SLAB and only until every recording with chunks in the slab has been turned into notes: a slab's entry
    # is [logits (batch, 88, T), event behind its forward, recordings still to read it, onset logits or None].
    slabs: List[list] = []
    segs: Dict[int, List[tuple]] = {}            # recording -> [(slab, first row, rows)] in chunk order
    open_recs: List[tuple] = []                  # (recording, first chunk of the shard, n chunks): chunks not yet all in launched slabs
    order: List[int] = []                        # recordings whose chunks are all in launched slabs, oldest first
    res: Dict[str, object] = {"chunks": 0, "notes": {}, "f1": {}, "n_notes": 0, "finite": True}
    if note_metrics:
        res["note_f1"] = {}
    finite_flags: List[torch.Tensor] = []
    fs = SR / HOP
    pos, cut = 0, 0                              # chunks decoded / chunks in launched slabs

    def launch(slab: torch.Tensor):
        nonlocal n_slabs, cut
        st = side[n_slabs % NS]
        st.wait_stream(main)                     # the slab was assembled on the main stream
        with torch.cuda.stream(st):
            mel, cmax = fe(slab, clamp=False)
            if heads:
                out = net(mel, chunk_max_power=cmax, return_all_heads=True)
                lg, on = out["frame"], out["onset"]
            else:
                lg, on = net(mel, chunk_max_power=cmax), None
            slab.record_stream(st)
            ev = torch.cuda.Event()
            ev.record(st)
        k, n = n_slabs, int(slab.shape[0])
        slabs.append([lg, ev, 0, on])
        # which recordings' chunks are rows [0, n) of this slab
        a = cut
        for rec in list(open_recs):
            i, first, cnt = rec
            lo, hi = max(first, a), min(first + cnt, a + n)
            if hi > lo:
                segs.setdefault(i, []).append((k, lo - a, hi - lo))
                slabs[k][2] += 1
            if first + cnt <= a + n:             # complete
                open_recs.remove(rec)
                order.append(i)
        cut += n
        n_slabs += 1

    f1_dev: Dict[int, torch.Tensor] = {}
    note_dev: Dict[int, torch.Tensor] = {}

    def finish(i):
        """Recording i's logits (its rows of the slabs it spans) -> notes / F1 on the device; the slabs are released behind it."""
        mine = segs.pop(i, [])
        if not mine:
            return
        parts, parts_on = [], []
        for k, a, n in mine:
            main.wait_event(slabs[k][1])
            parts.append(slabs[k][0][a:a + n])
            if heads:
                parts_on.append(slabs[k][3][a:a + n])
        lg = parts[0] if len(parts) == 1 else torch.cat(parts)
        on = (parts_on[0] if len(parts_on) == 1 else torch.cat(parts_on)) if heads else None
        finite_flags.append(torch.isfinite(lg).all())
        if want_notes:
            notes = (heads_to_notes_device(lg, on, threshold, onset_threshold, fs, **clean) if heads else
                     tr.notes_from_logits_device(lg, threshold, fs, **clean))
            res["notes"][i] = notes
            res["n_notes"] += len(notes)
            path = midi_path_of(i) if midi_path_of else None
            if path:
                tr.write_midi(notes, path)
        if reference_roll_of is not None:
            ref = reference_roll_of(i, int(lg.shape[0]) * int(lg.shape[2]))
            if ref is not None:
                roll = predict_from_logits(lg, threshold).permute(1, 0, 2).reshape(88, -1)
                L = min(int(ref.shape[1]), int(roll.shape[1]))
                f1_dev[i] = framewise_f1(roll[None, :, :L].contiguous(), ref[None, :, :L].contiguous().float())
                if note_metrics:
                    rows = lambda x: x.permute(1, 0, 2).reshape(88, -1)[:, :L].contiguous()
                    note_dev[i] = note_match_counts(rows(lg), ref[:, :L].contiguous().float(), threshold,
                                                    rows(on) if heads else None, onset_threshold, **clean)
        del parts, parts_on, lg, on
        for k, _, _ in mine:
            slabs[k][2] -= 1
            if slabs[k][2] == 0:
                slabs[k][0] = slabs[k][3] = None               # (the caching allocator reuses the block for a later slab's logits)

    def drain(keep_in_flight: int):
        """Finish the recordings whose last slab has at least `keep_in_flight` younger slabs queued behind it (the host blocks on
        that slab's notes while the GPU still has the younger slabs to run)."""
        while order:
            i = order[0]
            last = max(k for k, _, _ in segs[i])
            if last > n_slabs - 1 - keep_in_flight:
                break
            order.pop(0)
            finish(i)

    for i in rec_ids:
        c = chunks_of(i)
        n_i = int(c.shape[0])
        spans_n[i] = n_i
        if n_i:
            open_recs.append((i, pos, n_i))
            pos += n_i
            pending.append(c)
            n_pending += n_i
        while n_pending >= batch:                # cut slabs off the front of the pending pool
            pool = pending[0] if len(pending) == 1 else torch.cat(pending)
            launch(pool[:batch])
            rest = pool[batch:]
            pending, n_pending = ([rest] if rest.shape[0] else []), int(rest.shape[0])
            drain(NS)
    if n_pending:
        launch(pending[0] if len(pending) == 1 else torch.cat(pending))
    drain(0)
    for st in side:
        main.wait_stream(st)
    res["chunks"] = pos
    res["f1"] = {i: float(v[0]) for i, v in f1_dev.items()}
    if note_metrics:
        res["note_f1"] = {i: (m["onset"][2], m["onset_offset"][2]) for i, v in note_dev.items() for m in note_prf(v)}
    if finite_flags:
        res["finite"] = bool(torch.stack(finite_flags).all())
    torch.cuda.synchronize(dev)
    net.raise_on_handoff_timeout(sync=False)     # a timed-out recurrence leaves NaN logits = all-zero rolls: fail loudly
    res["wall_s"] = time.perf_counter() - t0
    res["slabs"] = n_slabs
    res["chunks_per_recording"] = {i: spans_n[i] for i in rec_ids}
    return res


class _Grouper:
    """plan_groups' rule, one recording at a time: add() returns the groups that the recording closes."""

    def __init__(self, group_windows: int, group_bytes: int, heads: int = 1):
        if group_windows < 1 or group_bytes < 1 or heads < 1:
            raise ValueError(f"group_windows, group_bytes and heads must be positive, got {group_windows}, {group_bytes}, {heads}")
        self.gw, self.gb, self.heads = int(group_windows), int(group_bytes), int(heads)
        self.cur: List[int] = []
        self.windows, self.t_max, self.n = 0, 0, 0

    def _bytes(self, R: int, t_max: int) -> int:
        return self.heads * R * 88 * t_max * 4

    def add(self, n_windows: int, n_frames: int) -> List[List[int]]:
        closed = []
        if self.cur and self._bytes(len(self.cur) + 1, max(self.t_max, int(n_frames))) > self.gb:
            closed += self.flush()
        self.cur.append(self.n)
        self.n += 1
        self.windows += int(n_windows)
        self.t_max = max(self.t_max, int(n_frames))
        if self.windows >= self.gw:
            closed += self.flush()
        return closed

    def flush(self) -> List[List[int]]:
        g, self.cur, self.windows, self.t_max = self.cur, [], 0, 0
        return [g] if g else []


def plan_groups(n_windows: Sequence[int], n_frames: Sequence[int], group_windows: int, group_bytes: int = 1 << 30,
                heads: int = 1) -> List[List[int]]:
    """Consecutive groups of recordings, as positions 0 .. len - 1 in the given order (host integers only).  n_windows[k] / n_frames[k]:
    windows and frames (Tg) of recording k.  A group closes when its windows reach group_windows; it closes before a recording that
    would push its stitched logits, heads * R * 88 * T_max * 4 bytes for R recordings padded to the longest, past group_bytes; a
    recording over that limit on its own is a group of one."""
    if len(n_windows) != len(n_frames):
        raise ValueError(f"{len(n_windows)} window counts for {len(n_frames)} frame counts")
    g = _Grouper(group_windows, group_bytes, heads)
    out: List[List[int]] = []
    for w, t in zip(n_windows, n_frames):
        out += g.add(w, t)
    return out + g.flush()


@torch.no_grad()
def transcribe_shard_windows(model, rec_ids: Sequence[int], audio_of: Callable[[int], torch.Tensor], *, overlap_s: float, n_mels: int, device,
                             batch: int = 128, streams: int = 3, group_windows: Optional[int] = None, group_bytes: int = 1 << 30,
                             threshold: float = 0.5, decoder: str = "frame", onset_threshold: float = 0.5, want_notes: bool = True,
                             reference_roll_of: Optional[Callable[[int, int], Optional[torch.Tensor]]] = None,
                             midi_path_of: Optional[Callable[[int], Optional[str]]] = None, note_metrics: bool = False,
                             warm: bool = True, min_note_frames: int = 1, bridge_frames: int = 0, smooth_on: float = 0.0,
                             smooth_off: float = 0.0, onset_detect: str = "edge", peak_reach: int = 1) -> Dict[str, object]:
    """transcribe_shard on the window grid.  audio_of(i) -> recording i as 1-D float32 at 16 kHz on the device, any length (0 samples
    included).  Recordings are taken in rec_ids order into groups (plan_groups; group_windows defaults to batch * streams).  A group
    runs exactly the slabs of windows.transcribe_windows(model, [its recordings], overlap_s, batch, all_heads) into zero-filled
    (R, 88, T_max) logits per head; slab f, counted over the whole shard, runs on side stream f % streams (at most 3 streams for
    cnn_rnn_large, two recurrence launches per forward: more are clamped to 3).  A group is finished on the main stream with lengths
    = its recordings' frame counts: notes of all its recordings from one notes_batch_device call, F1 counts, note counts and a finite
    flag; the host waits for group g's notes only after group g + 1's slabs are queued.  reference_roll_of(i, frames) -> (88, >= 1)
    roll on the recording's frame grid or None; scored over min(frames, reference frames).  Returns transcribe_shard's keys with
    "windows" for "chunks", and "groups" (lists of recording ids) and "frames" {i: 1 + n_i // 512}.  min_note_frames /
    bridge_frames as in transcribe_shard; smooth_on / smooth_off too, here over each recording's own frames (the lengths the decoder
    and the matcher are given); onset_detect / peak_reach as in transcribe_shard too (mt_notes_batch_peak for the notes)."""
    _check_corpus_decoder(decoder)
    tr.check_decoder(decoder, model=model)
    tr.check_detect_decoder(onset_detect, decoder, peak_reach)
    clean = dict(zip(("min_note_frames", "bridge_frames"), check_cleanup(min_note_frames, bridge_frames)))
    clean.update(zip(("smooth_on", "smooth_off"), check_smoothing(smooth_on, smooth_off)))
    W.overlap_frames(overlap_s)
    heads = decoder == "onset"
    if heads:                                    # (the frame decoder's calls have no onset head and take neither)
        clean.update(onset_detect=onset_detect, peak_reach=int(peak_reach))
    dev = torch.device(device)
    net, n_mels, fe = W._window_setup(model, n_mels, heads, dev)
    from .model import CNNRNNModelLarge
    NS = max(1, int(streams))
    if isinstance(net, CNNRNNModelLarge):
        NS = min(NS, 3)
    gw = int(group_windows) if group_windows is not None else batch * NS
    grouper = _Grouper(gw, group_bytes, 2 if heads else 1)
    side = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    main = torch.cuda.current_stream(dev)
    if warm:                                     # weight packing, code objects, every stream's workspace: not part of wall_s
        w0 = torch.zeros(batch, CH, device=dev)
        torch.cuda.synchronize(dev)
        for st in side:
            with torch.cuda.stream(st):
                m0, c0 = fe(w0, clamp=False)
                net(m0, chunk_max_power=c0, return_all_heads=True) if heads else net(m0, chunk_max_power=c0)
        torch.cuda.synchronize(dev)
        del w0
    ids = list(rec_ids)
    fs = SR / HOP
    res: Dict[str, object] = {"windows": 0, "slabs": 0, "notes": {}, "f1": {}, "n_notes": 0, "finite": True, "groups": [], "frames": {}}
    if note_metrics:
        res["note_f1"] = {}
    held: Dict[int, torch.Tensor] = {}            # position in ids -> recording, until its group runs
    finite_flags: List[torch.Tensor] = []
    f1_dev: List[tuple] = []                      # per group: (ids with a reference, their rows, (R, 3) counts, (R, 4) note counts or None)
    pending: List[tuple] = []                     # the group whose slabs are queued and whose host side is still to do
    t0 = time.perf_counter()

    def queue(group: List[int]):
        """The group's store, zero-filled logits and slabs; the slabs go to the side streams."""
        ys = [held.pop(k) for k in group]
        store, offs, ns = W._store(ys)
        Tg = [1 + n // HOP for n in ns]
        R = len(ys)
        outs = [torch.zeros(R, W.N_PITCH, max(Tg), dtype=torch.float32, device=dev) for _ in range(2 if heads else 1)]
        jobs = W._jobs(ns, range(R), overlap_s)
        events = []
        for s0 in range(0, len(jobs), batch):
            st = side[res["slabs"] % NS]
            st.wait_stream(main)                 # the store and the zero fill were queued on the main stream
            with torch.cuda.stream(st):
                W._run_slab(net, fe, n_mels, jobs[s0:s0 + batch], store, offs, outs, heads, dev)
                for t in [store] + outs:
                    t.record_stream(st)
                ev = torch.cuda.Event()
                ev.record(st)
            events.append(ev)
            res["slabs"] += 1
        res["windows"] += len(jobs)
        rec = [ids[k] for k in group]
        res["groups"].append(rec)
        for i, t in zip(rec, Tg):
            res["frames"][i] = t
        return rec, Tg, outs, events

    def finish(rec, Tg, outs, events):
        """Notes, counts and the finite flag of one group, on the main stream behind the group's slabs."""
        for ev in events:
            main.wait_event(ev)
        frame, onset = outs[0], (outs[1] if heads else None)
        finite_flags.append(torch.isfinite(frame).all())          # (over the zero-filled buffer: padding is finite)
        if want_notes:
            for i, notes in zip(rec, notes_batch_device(frame, onset, threshold, onset_threshold, Tg, fs, **clean)):
                res["notes"][i] = notes
                res["n_notes"] += len(notes)
                path = midi_path_of(i) if midi_path_of else None
                if path:
                    tr.write_midi(notes, path)
        if reference_roll_of is None:
            return
        refs = [reference_roll_of(i, t) for i, t in zip(rec, Tg)]
        if all(r is None for r in refs):
            return
        roll = torch.zeros_like(frame)
        cmp = [0] * len(rec)                      # frames compared per recording; 0 = no reference, its counts are dropped
        for r, ref in enumerate(refs):
            if ref is not None:
                cmp[r] = min(Tg[r], int(ref.shape[1]))
                roll[r, :, :cmp[r]] = ref[:, :cmp[r]]
        ln = torch.tensor(cmp, dtype=torch.int64).to(dev)
        c = f1_counts(predict_from_logits(frame, threshold), roll, ln)
        nc = note_match_counts(frame, roll, threshold, onset, onset_threshold, ln, **clean) if note_metrics else None
        f1_dev.append(([i for i, ref in zip(rec, refs) if ref is not None], [r for r, ref in enumerate(refs) if ref is not None], c, nc))

    def run(group: List[int]):
        queued = queue(group)
        if pending:
            finish(*pending.pop())
        pending.append(queued)

    for k, i in enumerate(ids):
        y = audio_of(i)
        if not torch.is_tensor(y) or y.dim() != 1 or y.dtype != torch.float32 or y.device.type != "cuda":
            raise ValueError(f"audio_of({i}) must return a 1-D float32 CUDA tensor")
        held[k] = y
        p = W.plan_windows(int(y.numel()), overlap_s)
        for group in grouper.add(len(p.start), p.Tg):
            run(group)
    for group in grouper.flush():
        run(group)
    if pending:
        finish(*pending.pop())
    for st in side:
        main.wait_stream(st)
    for rec, rows, c, nc in f1_dev:
        f1 = f1_from_counts(c)
        for i, r in zip(rec, rows):
            res["f1"][i] = float(f1[r])
        if nc is not None:
            prf = note_prf(nc)
            for i, r in zip(rec, rows):
                res["note_f1"][i] = (prf[r]["onset"][2], prf[r]["onset_offset"][2])
    if finite_flags:
        res["finite"] = bool(torch.stack(finite_flags).all())
    torch.cuda.synchronize(dev)
    net.raise_on_handoff_timeout(sync=False)     # a timed-out recurrence leaves NaN logits = all-zero rolls: fail loudly
    res["wall_s"] = time.perf_counter() - t0
    return res


class PcmSource:
    """chunks_of for transcribe_shard when the recordings are PCM frames in (pinned) HOST memory, as a WAV file holds them:
    (frames, channels) int16 / int32 / float32 at `rate`.  Recording order is known up front, so the H2D copy of recording
    k + `ahead` is queued on a copy stream while recording k is resampled (mt_resample_polyphase: channel mean + PCM scaling +
    polyphase filter in one kernel) and cut into zero-padded 30 s chunks (main.py:60-100) -- librosa.load(sr=16000, mono=True) +
    split_audio_into_chunks of the reference, on the device."""

    def __init__(self, pcm_of: Callable[[int], torch.Tensor], rate_of: Callable[[int], int], rec_ids: Sequence[int], device, ahead: int = 2):
        self.pcm_of, self.rate_of, self.ids, self.dev, self.ahead = pcm_of, rate_of, list(rec_ids), torch.device(device), max(0, ahead)
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.index = {i: k for k, i in enumerate(self.ids)}
        self.inflight: Dict[int, tuple] = {}
        self.cursor = 0
        self.bytes_h2d = 0

    def _prefetch(self, upto: int):
        while self.cursor < min(upto + 1, len(self.ids)):
            i = self.ids[self.cursor]
            host = self.pcm_of(i)
            with torch.cuda.stream(self.copy_stream):
                d = host.to(self.dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            self.bytes_h2d += host.numel() * host.element_size()
            self.inflight[i] = (d, ev)
            self.cursor += 1

    def recording(self, i: int) -> torch.Tensor:
        """Recording i as 1-D float32 at 16 kHz on the device (audio_of for transcribe_shard_windows)."""
        self._prefetch(self.index[i] + self.ahead)
        d, ev = self.inflight.pop(i)
        main = torch.cuda.current_stream(self.dev)
        main.wait_event(ev)
        d.record_stream(main)
        return tr.resample_pcm_device(d, self.rate_of(i), SR)

    def __call__(self, i: int) -> torch.Tensor:
        return tr.split_into_chunks_device(self.recording(i))[0]


def synthetic_corpus(n_recordings: int, hours: float, seed: int = 0):
    """Durations (s) of a MAESTRO-test-like corpus: gamma(2.5)-distributed lengths scaled to `hours` in total."""
    import numpy as np
    rng = np.random.default_rng(seed)
    raw = rng.gamma(2.5, 1.0, size=n_recordings)
    return list(raw / raw.sum() * hours * 3600.0)


def synth_recording(i: int, seconds: float, device, seed: int = 0) -> torch.Tensor:
    """Noise + a few decaying partials, generated on the GPU; the last chunk zero-padded in the waveform domain (main.py:93-95)."""
    n = int(seconds * SR)
    g = torch.Generator(device=device).manual_seed(seed * 100003 + i)
    nch = max(1, -(-n // CH))
    t = torch.arange(nch * CH, device=device, dtype=torch.float32) / SR
    y = 0.1 * torch.randn(nch * CH, device=device, generator=g)
    for k in range(4):
        f0 = 27.5 * 2.0 ** (float(torch.randint(0, 88, (1,), device=device, generator=g)) / 12.0)
        y += 0.3 * torch.exp(-((t * (0.5 + k)) % 3.0)) * torch.sin(2 * torch.pi * f0 * t)
    y[n:] = 0.0
    return y.clamp_(-1, 1).view(nch, CH)
