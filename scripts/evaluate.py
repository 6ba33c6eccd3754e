#!/usr/bin/env python3
"""Framewise-F1 evaluation of a checkpoint over a cached split: the evaluation half of the reference's scripts/evaluate.py
(:335-379 headless loop, :524-618 threshold tuning; same flag names and defaults for what is kept).

    python scripts/evaluate.py --model outputs/.../checkpoints/model_best.pth --cache_dir cached_dataset_mels320 --headless
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/evaluate.py --model ... --headless

`--headless` prints exactly one line, `EVAL_MEAN_F1=<%.6f>` (what the reference's example.sh greps for).  The metric is the
reference's: per-sample binary F1 over the valid frames of the flattened (88, L) roll with zero_division = 0, unweighted mean
over the samples.  On the device: the model runs once per sample (samples of equal length batched -- no padding arises, so each
sample's logits are what batch 1 gives), thresholding and the TP / FP / FN counts are one integer pass (mt_f1_sweep_counts);
with `--tune_threshold` every candidate threshold of the reference's coarse-to-fine schedule is another counts pass over the SAME
logits instead of another run of the model.  With more than one rank the samples are sharded contiguously (no data-path
collective) and the per-sample values gathered by one small all-reduce.  `--data_source full` (and `auto` without a cache)
evaluates whole recordings under --root_dir, one sample per recording (MaestroDataset with chunk_length=None, featurised on
the GPU); a recording longer than the inference recurrence takes (T * hidden_size < 2^24 frames) ends the run with an error
naming it.  `--window_overlap SECONDS` instead runs every recording in overlapping 30 s windows stitched on its own frame grid
(windows.py), which has no such limit.  `--note_metrics --note_reference midi` (whole recordings only) scores the decoded notes
against the MIDI note list of each recording, in which a re-struck key is a note of its own, instead of the runs of the label roll.
`--note_metrics --tune_note_thresholds` first chooses the note decoder's thresholds for the best mean note F1 (one model run, one
sweep pass over the logits per group and round: evaluate.tune_note_thresholds) and reports the note metrics at those.
`--note_metrics --tune_note_decoder [--tune_min_note_ms 0 64 ...] [--tune_bridge_gap_ms 0 32 ...]` chooses every parameter of the
decoder together, with any --decoder: its thresholds (frame; onset; offset) and the note cleanup out of the product of the two lists
(evaluate.tune_note_decoder: one model run, one grid pass per group and round), and reports the note metrics at that configuration.
`--note_metrics --smooth_on X --smooth_off Y` smooths the frame head with a two-state HMM per pitch before the notes are decoded
(notes.smooth_frame_logits); the framewise F1 stays that of the raw threshold, and no tuner takes a fixed smoothing.
`--tune_note_decoder --tune_smooth_on 0 1 2 --tune_smooth_off 0 1 2` tunes the two penalties with everything else: every pair of the
two lists is one more candidate of each round's grid (one packed-path launch per group and tile of 16 frame candidates), and the
note metrics are reported at the chosen pair.
`--note_metrics --decoder onset|onset_offset --onset_detect peak [--peak_reach N]` opens the notes at the local maxima of the onset
logits, not at the rising edges of the thresholded onset head (DESIGN.md 6c "Peak-picked onsets"); with cleanup, smoothing,
--window_overlap and --refine_onsets as before, not with the tuners.
`--tune_note_decoder --decoder onset|onset_offset --tune_peak_reach 0 1 2` tunes that detector with everything else: every reach of the
list, 0 = the edge rule, is one more candidate of each round's grid (DESIGN.md 6c "Peak picking in the decoder grid"), and the note
metrics are reported at the chosen reach.
`--note_metrics --note_reference midi --decoder onset|onset_offset --refine_onsets [--refine_reach N]` gives every decoded note a
sub-frame onset (mt_refine_onsets) and scores the note lists on the device in ticks of 100 us (notes.notes_ticks_tables_device,
notes.note_match_ticks_device: a maximum matching per pitch row; only the counts reach the host); the same EVAL_NOTE_* lines as the host
matcher notes.note_match_ticks gives.  Cleanup and smoothing flags stay allowed; the tuners are refused here (from Python,
evaluate.tune_note_decoder(refine_onsets=True) tunes the decoder on that figure; DESIGN.md 6c "Decoder grid in ticks").
MIDI / plot outputs, background mode and the results browser are out of scope.
"""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


def main():
    ap = argparse.ArgumentParser(description="Evaluate a transcription checkpoint (framewise F1) on a cached split")
    ap.add_argument("--model", type=str, required=True, help="Path to model checkpoint (.pth file)")
    ap.add_argument("--split", type=str, default="test", choices=["train", "validation", "test"])
    ap.add_argument("--threshold", type=float, default=0.5, help="Sigmoid threshold for binary prediction (default: 0.5)")
    ap.add_argument("--subset", type=int, default=None, help="Limit number of samples (for quick eval)")
    ap.add_argument("--batch_size", type=int, default=1, help="accepted for compatibility: samples of equal length are batched on the device")
    ap.add_argument("--data_source", type=str, default="auto", choices=["auto", "cache", "full"])
    ap.add_argument("--cache_dir", type=str, default="cached_dataset_mels320")
    ap.add_argument("--root_dir", type=str, default="maestro-v3.0.0", help="Path to MAESTRO dataset (for full files, default: maestro-v3.0.0)")
    ap.add_argument("--year", type=str, default=None, help="Year filter (full files only, e.g., 2017)")
    ap.add_argument("--n_mels", type=int, default=None, help="Number of mel bins (auto-detected from cache if not specified)")
    ap.add_argument("--model_type", type=str, default="cnn_rnn_large")
    ap.add_argument("--hidden_size", type=int, default=512)
    ap.add_argument("--num_layers", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--out_dir", type=str, default="eval_outputs", help="results.json is written here unless --headless")
    ap.add_argument("--headless", action="store_true", help="Headless mode: only print EVAL_MEAN_F1=<value>")
    ap.add_argument("--note_metrics", action="store_true",
                    help="also report note-level precision / recall / F1 (onset within 50 ms; onset + offset within max(50 ms, 20%% of the "
                         "note), mir_eval's criteria on the 32 ms frame grid) against the runs of the label roll; headless prints "
                         "EVAL_NOTE_ONSET_F1= and EVAL_NOTE_ONSET_OFFSET_F1= after EVAL_MEAN_F1=")
    ap.add_argument("--note_reference", choices=["roll", "midi"], default="roll",
                    help="reference notes of --note_metrics: roll = the runs of the label roll (default; pedalled and gapless re-strikes are "
                         "one note); midi = the recording's MIDI note list in 100 us ticks, pedal-extended and cut at the pitch's next onset "
                         "(needs --data_source full)")
    ap.add_argument("--decoder", choices=["frame", "onset", "onset_offset"], default="frame",
                    help="note decoder for --note_metrics: frame = runs of active frames (default); onset = notes start at rising edges "
                         "of the onset head; onset_offset = those notes, ended on the frame where the offset head fires (cnn_rnn_large "
                         "trained with --train_all_heads; untrained heads make both meaningless)")
    ap.add_argument("--onset_threshold", type=float, default=0.5,
                    help="threshold of the onset head for --decoder onset / onset_offset (default: 0.5)")
    ap.add_argument("--offset_threshold", type=float, default=0.5, help="threshold of the offset head for --decoder onset_offset (default: 0.5)")
    ap.add_argument("--min_note_ms", type=float, default=0.0,
                    help="with --note_metrics: note cleanup in the decoder, drop every estimated note shorter than this many milliseconds "
                         "(32 ms frames; at most 2048; default 0 = keep all).  Not with --tune_note_thresholds: the sweeps do not clean")
    ap.add_argument("--bridge_gap_ms", type=float, default=0.0,
                    help="with --note_metrics: note cleanup in the decoder, a dropout of the activity no longer than this many "
                         "milliseconds does not end the note (below 2048; default 0 = none)")
    ap.add_argument("--smooth_on", type=float, default=0.0,
                    help="with --note_metrics: frame smoothing before the note decoder, the cost in logits of switching a pitch on in the "
                         "two-state HMM that replaces the frame head by its best path (0 to 64; default 0).  The framewise F1 printed "
                         "beside the note F1 stays that of the raw threshold.  Not with --tune_threshold, --tune_note_thresholds or "
                         "--tune_note_decoder: the tuners do not smooth")
    ap.add_argument("--smooth_off", type=float, default=0.0,
                    help="with --note_metrics: frame smoothing, the cost in logits of switching a pitch off (0 to 64; default 0 = with "
                         "--smooth_on 0, no smoothing)")
    ap.add_argument("--refine_onsets", action="store_true",
                    help="with --note_metrics --note_reference midi --decoder onset / onset_offset: give every decoded note a sub-frame onset "
                         "from the onset head's values around its peak (a head trained with train_cnn.py --onset_target regress) and score "
                         "the note lists on the device in 100 us ticks (mt_note_match_ticks); prints the same EVAL_NOTE_* lines.  Not with the "
                         "three tuners")
    ap.add_argument("--refine_reach", type=int, default=2,
                    help="--refine_onsets: frames the peak search may walk from a note's first frame (0..8; default 2 = the default "
                         "--onset_width of training)")
    ap.add_argument("--onset_detect", choices=["edge", "peak"], default="edge",
                    help="with --note_metrics --decoder onset / onset_offset: where a note opens.  edge (default): at every rising edge of "
                         "the thresholded onset head; peak: at every local maximum of the onset logits within --peak_reach frames that "
                         "passes the onset threshold (for a head trained with train_cnn.py --onset_target regress, whose triangles the "
                         "edge rule merges when a key is re-struck within --onset_width frames).  Not with the three tuners: the sweep "
                         "kernels have no peak mode, and --tune_note_decoder tunes the detector through --tune_peak_reach")
    ap.add_argument("--peak_reach", type=int, default=1,
                    help="--onset_detect peak: a peak must be the largest logit of this many frames on either side (1..8; default 1); "
                         "peaks are then more than this many frames apart")
    ap.add_argument("--window_overlap", type=float, default=None,
                    help="full files only: run every recording in overlapping 30 s windows (this many seconds of overlap, 0.256 to 15) "
                         "stitched on its own frame grid, instead of one recurrence over the whole file; lifts the T * hidden_size < 2^24 "
                         "length limit")
    ap.add_argument("--tune_threshold", action="store_true")
    ap.add_argument("--tune_rounds", type=int, default=6)
    ap.add_argument("--tune_range", type=float, nargs=2, default=[0.05, 0.95])
    ap.add_argument("--tune_step", type=float, default=0.1)
    ap.add_argument("--tune_min_step", type=float, default=0.01)
    ap.add_argument("--tune_note_thresholds", action="store_true",
                    help="with --note_metrics: choose the note decoder's thresholds (--decoder frame: the frame threshold; onset: the "
                         "frame and the onset threshold together) for the best mean note F1 by the coarse-to-fine schedule of "
                         "--tune_threshold (--tune_rounds / --tune_range / --tune_step / --tune_min_step), one model run, and report the "
                         "note metrics there; headless adds EVAL_NOTE_THRESHOLD= (and EVAL_NOTE_ONSET_THRESHOLD=).  Framewise F1 keeps "
                         "--threshold / --tune_threshold")
    ap.add_argument("--tune_note_objective", choices=["onset", "onset_offset"], default="onset",
                    help="the note F1 that --tune_note_thresholds maximises (default: onset)")
    ap.add_argument("--tune_note_decoder", action="store_true",
                    help="with --note_metrics: choose every parameter of the note decoder together for the best mean note F1 "
                         "(--tune_note_objective), with any --decoder: the thresholds of the heads it reads (frame; onset; offset) and the "
                         "note cleanup out of --tune_min_note_ms x --tune_bridge_gap_ms, by the schedule of --tune_threshold, one model run; "
                         "headless adds EVAL_NOTE_THRESHOLD= (EVAL_NOTE_ONSET_THRESHOLD=, EVAL_NOTE_OFFSET_THRESHOLD=), "
                         "EVAL_NOTE_MIN_NOTE_MS= and EVAL_NOTE_BRIDGE_GAP_MS=.  Not with --tune_note_thresholds, --min_note_ms or "
                         "--bridge_gap_ms")
    ap.add_argument("--tune_min_note_ms", type=float, nargs="+", default=[0.0],
                    help="--tune_note_decoder: the candidates for --min_note_ms (default: 0)")
    ap.add_argument("--tune_bridge_gap_ms", type=float, nargs="+", default=[0.0],
                    help="--tune_note_decoder: the candidates for --bridge_gap_ms (default: 0); every pair of the two lists is tried")
    ap.add_argument("--tune_smooth_on", type=float, nargs="+", default=[0.0],
                    help="--tune_note_decoder: the candidates for --smooth_on, in logits (default: 0); headless adds EVAL_NOTE_SMOOTH_ON= "
                         "and EVAL_NOTE_SMOOTH_OFF= when either list is given")
    ap.add_argument("--tune_smooth_off", type=float, nargs="+", default=[0.0],
                    help="--tune_note_decoder: the candidates for --smooth_off (default: 0); every pair of the two lists is tried, with "
                         "every cleanup pair, in every round")
    ap.add_argument("--tune_peak_reach", type=int, nargs="+", default=None, metavar="R",
                    help="--tune_note_decoder with --decoder onset or onset_offset: the candidate reaches of the peak-picking onset "
                         "detector (--onset_detect peak --peak_reach R), integers in 0..8, 0 = the edge rule; every reach is tried with "
                         "every cleanup and smoothing pair, in every round, and the note metrics are those at the chosen one; headless "
                         "adds EVAL_NOTE_PEAK_REACH= (0: the edge rule won).  Default: absent, the edge rule alone")
    args = ap.parse_args()
    tune_cleanups = tune_smoothings = None
    if args.tune_peak_reach is not None:
        if not args.tune_note_decoder:
            ap.error("--tune_peak_reach lists the candidate reaches of --tune_note_decoder and needs that flag")
        if args.decoder not in ("onset", "onset_offset"):
            ap.error("--tune_peak_reach picks peaks on the onset head and needs --decoder onset or onset_offset")
        if not all(0 <= r <= 8 for r in args.tune_peak_reach):
            ap.error("--tune_peak_reach: a reach must lie in 0..8 frames (0 = the edge rule)")
    if args.tune_note_decoder:
        if args.tune_note_thresholds:
            ap.error("--tune_note_decoder cannot be combined with --tune_note_thresholds: it tunes the thresholds itself")
        if args.min_note_ms or args.bridge_gap_ms:
            ap.error("--tune_note_decoder cannot be combined with --min_note_ms / --bridge_gap_ms: it chooses the cleanup itself, out of "
                     "--tune_min_note_ms x --tune_bridge_gap_ms")
        try:
            from music_transcription_amd.notes import cleanup_frames
            tune_cleanups = [(m, g, cleanup_frames(m, g)) for m in args.tune_min_note_ms for g in args.tune_bridge_gap_ms]     # min-note-major
            if args.tune_smooth_on != [0.0] or args.tune_smooth_off != [0.0]:
                from music_transcription_amd.notes import check_smoothing
                tune_smoothings = [check_smoothing(a, b) for a in args.tune_smooth_on for b in args.tune_smooth_off]             # on-major
        except ValueError as e:
            ap.error(str(e))
    elif args.tune_min_note_ms != [0.0] or args.tune_bridge_gap_ms != [0.0]:
        ap.error("--tune_min_note_ms / --tune_bridge_gap_ms are the cleanup candidates of --tune_note_decoder and need that flag")
    elif args.tune_smooth_on != [0.0] or args.tune_smooth_off != [0.0]:
        ap.error("--tune_smooth_on / --tune_smooth_off are the smoothing candidates of --tune_note_decoder and need that flag")
    if args.tune_note_thresholds and args.decoder == "onset_offset":
        ap.error("--tune_note_thresholds does not cover --decoder onset_offset (the threshold sweeps do not read the offset head): tune with "
                 "--decoder onset and pass the thresholds it reports")
    min_note_frames, bridge_frames = 1, 0
    if args.min_note_ms or args.bridge_gap_ms:
        if not args.note_metrics:
            ap.error("--min_note_ms / --bridge_gap_ms clean the notes of --note_metrics and need that flag")
        if args.tune_note_thresholds:
            ap.error("--min_note_ms / --bridge_gap_ms cannot be combined with --tune_note_thresholds: the threshold sweeps do not clean "
                     "notes; tune without cleanup, then evaluate with it at the thresholds reported")
        try:
            from music_transcription_amd.notes import cleanup_frames
            min_note_frames, bridge_frames = cleanup_frames(args.min_note_ms, args.bridge_gap_ms)
        except ValueError as e:
            ap.error(str(e))
    smooth_on = smooth_off = 0.0
    if args.smooth_on or args.smooth_off:
        if not args.note_metrics:
            ap.error("--smooth_on / --smooth_off smooth the frame head for the notes of --note_metrics and need that flag")
        for flag in ("tune_threshold", "tune_note_thresholds", "tune_note_decoder"):
            if getattr(args, flag):
                ap.error(f"--smooth_on / --smooth_off cannot be combined with --{flag}: the tuners do not smooth; tune without smoothing, "
                         "then evaluate with it at the values reported")
        try:
            from music_transcription_amd.notes import check_smoothing
            smooth_on, smooth_off = check_smoothing(args.smooth_on, args.smooth_off)
        except ValueError as e:
            ap.error(str(e))
    if args.refine_onsets:
        if not args.note_metrics or args.note_reference != "midi":
            ap.error("--refine_onsets refines the notes of --note_metrics and scores them against the MIDI note list in ticks: it needs "
                     "--note_metrics --note_reference midi")
        if args.decoder not in ("onset", "onset_offset"):
            ap.error("--refine_onsets reads the onset head and needs --decoder onset or onset_offset")
        for flag in ("tune_threshold", "tune_note_thresholds", "tune_note_decoder"):
            if getattr(args, flag):
                ap.error(f"--refine_onsets cannot be combined with --{flag}: this script's tuners count on the frame grid; tune "
                         "without it, then evaluate with it at the values reported"
                         + (" (from Python, evaluate.tune_note_decoder(refine_onsets=True) tunes on refined onsets, scored in ticks)"
                            if flag == "tune_note_decoder" else ""))
        if not 0 <= args.refine_reach <= 8:
            ap.error("--refine_reach must lie in 0..8 frames")
    if args.onset_detect != "edge" or args.peak_reach != 1:
        if not args.note_metrics:
            ap.error("--onset_detect / --peak_reach choose where the notes of --note_metrics open and need that flag")
        if args.decoder not in ("onset", "onset_offset"):
            ap.error("--onset_detect / --peak_reach read the onset head and need --decoder onset or onset_offset")
        for flag in ("tune_threshold", "tune_note_thresholds", "tune_note_decoder"):
            if getattr(args, flag):
                ap.error(f"--onset_detect / --peak_reach cannot be combined with --{flag}: peak detection inside the sweep and grid "
                         "kernels is out of scope; tune with the edge rule, then evaluate with peaks at the values reported"
                         + (" -- or let it tune the detector itself: --tune_peak_reach 0 1 2" if flag == "tune_note_decoder" else ""))
        if not 1 <= args.peak_reach <= 8:
            ap.error("--peak_reach must lie in 1..8 frames (--onset_detect peak)")
    say = (lambda *a, **k: None) if args.headless else print

    if args.note_reference == "midi" and args.data_source != "full":
        print("Error: --note_reference midi scores against the MIDI note list of whole recordings and needs --data_source full "
              "(cache records hold rolls of chunks, not notes)")
        return 1
    if args.tune_note_thresholds and not args.note_metrics:
        print("Error: --tune_note_thresholds tunes the thresholds of --note_metrics and needs that flag")
        return 1
    if args.tune_note_decoder and not args.note_metrics:
        print("Error: --tune_note_decoder tunes the decoder of --note_metrics and needs that flag")
        return 1
    if not os.path.exists(args.model):
        print(f"Error: Model checkpoint not found: {args.model}")
        return 1
    heads = args.decoder in ("onset", "onset_offset")
    if args.note_metrics and heads and args.model_type not in ("cnn_rnn_large", "large"):
        print(f"Error: --decoder {args.decoder} needs the onset head of cnn_rnn_large (model_type {args.model_type} has none)")
        return 1
    meta_path = os.path.join(args.cache_dir, f"{args.split}_metadata.pkl")
    full = args.data_source == "full" or (args.data_source == "auto" and not os.path.exists(meta_path))
    if full and not os.path.exists(args.root_dir):
        print(f"Error: neither cache ({meta_path}) nor dataset ({args.root_dir}) found")
        return 1
    if not full and not os.path.exists(meta_path):
        print(f"Error: no cached split at {meta_path} (run scripts/preprocess_dataset.py, or use --data_source full --root_dir ...)")
        return 1
    if args.window_overlap is not None:
        if not full:
            print(f"Error: --window_overlap evaluates whole recordings and needs --data_source full (the cache at {meta_path} holds chunks)")
            return 1
        try:
            from music_transcription_amd.windows import overlap_frames
            overlap_frames(args.window_overlap)
        except ValueError as e:
            print(f"Error: --window_overlap: {e}")
            return 1
    n_mels = args.n_mels
    if full:
        n_mels = n_mels or 320
    elif n_mels is None:                                # evaluate.py:151-156: n_mels from the cache metadata
        with open(meta_path, "rb") as f:
            n_mels = pickle.load(f).get("n_mels", 320)
        say(f"Auto-detected n_mels={n_mels} from cache metadata")

    import torch
    import torch.distributed as dist
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    backend = os.environ.get("MT_BENCH_BACKEND", "nccl")
    if not torch.cuda.is_available():
        print("Error: music_transcription_amd evaluates on the GPU only")
        return 1
    dev_index = local if backend == "nccl" else local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    dev = f"cuda:{dev_index}"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    import music_transcription_amd as mta
    from music_transcription_amd import evaluate as E

    say(f"Using device: {dev}")
    if full:                                           # recordings first: one past the recurrence's limit ends the run before the model loads
        say(f"Loading full-file dataset from: {args.root_dir}")
        ds = mta.MaestroDataset(args.root_dir, split=args.split, year=args.year, n_mels=n_mels, subset_size=args.subset, chunk_length=None,
                                device=dev, onset_labels="midi" if args.note_reference == "midi" else "roll")
        t_max = ((1 << 24) - 1) // args.hidden_size        # lstm.hip: the inference recurrence takes T * H < 2^24
        for row, t in zip(ds.rows, ds.num_frames):
            if int(t) > t_max and args.window_overlap is None:          # (in windows every forward is 938 frames)
                print(f"Error: recording {row['audio_filename']} has T={int(t)} frames; the inference recurrence takes at most "
                      f"{t_max} at hidden_size={args.hidden_size} (T * hidden_size < 2^24)")
                return 1
    model = mta.TranscriptionModel(model_type=args.model_type, device=dev, n_mels=n_mels, hidden_size=args.hidden_size,
                                   num_layers=args.num_layers, dropout=args.dropout)
    model.load_state_dict(torch.load(args.model, map_location=dev))
    model.eval()
    if not full:
        say(f"Loading cached dataset from: {args.cache_dir}")
        ds = mta.CachedMaestroDataset(args.cache_dir, args.split)
    threshold = args.threshold
    if args.tune_threshold:
        threshold, tuned_f1 = E.tune_threshold(model, ds, dev, subset=args.subset, tune_range=tuple(args.tune_range), tune_step=args.tune_step,
                                               tune_min_step=args.tune_min_step, tune_rounds=args.tune_rounds, rank=rank, world=world,
                                               log=say if rank == 0 else None, window_overlap=args.window_overlap)
        say(f"Best threshold: {threshold:.4f} (mean F1 {tuned_f1:.6f})")
    mean_f1, per_sample = E.evaluate_dataset(model, ds, threshold, dev, subset=args.subset, rank=rank, world=world,
                                             window_overlap=args.window_overlap)
    notes = None
    note_threshold, note_onset_threshold = threshold, (args.onset_threshold if heads else None)
    note_offset_threshold = args.offset_threshold if args.decoder == "onset_offset" else None
    if args.tune_note_thresholds:
        note_threshold, note_onset_threshold, tuned_note_f1 = E.tune_note_thresholds(
            model, ds, dev, subset=args.subset, decoder=args.decoder, note_reference=args.note_reference, objective=args.tune_note_objective,
            tune_range=tuple(args.tune_range), tune_step=args.tune_step, tune_min_step=args.tune_min_step, tune_rounds=args.tune_rounds,
            rank=rank, world=world, log=say if rank == 0 else None, window_overlap=args.window_overlap)
        say(f"Best note thresholds: frame {note_threshold:.4f}" + ("" if note_onset_threshold is None else f", onset {note_onset_threshold:.4f}")
            + f" (mean {args.tune_note_objective} note F1 {tuned_note_f1:.6f})")
    note_min_ms = note_gap_ms = None
    note_peak_reach = args.peak_reach if args.onset_detect == "peak" else 0
    if args.tune_note_decoder:
        tuned = E.tune_note_decoder(
            model, ds, dev, subset=args.subset, decoder=args.decoder, note_reference=args.note_reference, objective=args.tune_note_objective,
            cleanups=[c for _, _, c in tune_cleanups], tune_range=tuple(args.tune_range), tune_step=args.tune_step,
            tune_min_step=args.tune_min_step, tune_rounds=args.tune_rounds, rank=rank, world=world, log=say if rank == 0 else None,
            window_overlap=args.window_overlap, smoothings=tune_smoothings, peak_reaches=args.tune_peak_reach)
        note_threshold, note_onset_threshold, note_offset_threshold, tuned_clean = tuned[:4]
        tuned_note_f1 = tuned[-1]
        if tune_smoothings is not None:                    # the note metrics below are those at the chosen penalties
            smooth_on, smooth_off = tuned[4]
        # (the first candidate with the chosen frames: different milliseconds can round to one pair, and the search keeps the first)
        note_min_ms, note_gap_ms = next((m, g) for m, g, c in tune_cleanups if c == tuned_clean)
        min_note_frames, bridge_frames = tuned_clean
        if args.tune_peak_reach is not None:               # ... and at the chosen detector: ("edge", 0) or ("peak", R)
            note_peak_reach = tuned[-2][1]
        say(f"Best note decoder: frame {note_threshold:.4f}" + ("" if note_onset_threshold is None else f", onset {note_onset_threshold:.4f}")
            + ("" if note_offset_threshold is None else f", offset {note_offset_threshold:.4f}")
            + f", min note {note_min_ms:g} ms, bridged gap {note_gap_ms:g} ms"
            + ("" if tune_smoothings is None else f", smoothing on {smooth_on:g} / off {smooth_off:g} logits")
            + ("" if args.tune_peak_reach is None else f", onsets at peaks over {note_peak_reach} frames" if note_peak_reach else ", onsets at edges")
            + f" (mean {args.tune_note_objective} note F1 {tuned_note_f1:.6f})")
    if args.note_metrics:
        notes = E.note_metrics_dataset(model, ds, note_threshold, note_onset_threshold, dev,
                                       subset=args.subset, rank=rank, world=world, window_overlap=args.window_overlap,
                                       note_reference=args.note_reference, offset_threshold=note_offset_threshold,
                                       min_note_frames=min_note_frames, bridge_frames=bridge_frames, smooth_on=smooth_on,
                                       smooth_off=smooth_off, **(dict(refine_onsets=True, refine_reach=args.refine_reach)
                                                                 if args.refine_onsets else {}),
                                       **(dict(onset_detect="peak", peak_reach=note_peak_reach) if note_peak_reach else {}))
    if rank == 0:
        if args.headless:
            print(f"EVAL_MEAN_F1={mean_f1:.6f}")
            if notes is not None:
                print(f"EVAL_NOTE_ONSET_F1={notes['mean']['onset_f1']:.6f}")
                print(f"EVAL_NOTE_ONSET_OFFSET_F1={notes['mean']['onset_offset_f1']:.6f}")
                if args.tune_note_thresholds or args.tune_note_decoder:
                    print(f"EVAL_NOTE_THRESHOLD={note_threshold:.4f}")
                    if note_onset_threshold is not None:
                        print(f"EVAL_NOTE_ONSET_THRESHOLD={note_onset_threshold:.4f}")
                if args.tune_note_decoder:
                    if note_offset_threshold is not None:
                        print(f"EVAL_NOTE_OFFSET_THRESHOLD={note_offset_threshold:.4f}")
                    print(f"EVAL_NOTE_MIN_NOTE_MS={note_min_ms:g}")
                    print(f"EVAL_NOTE_BRIDGE_GAP_MS={note_gap_ms:g}")
                    if tune_smoothings is not None:
                        print(f"EVAL_NOTE_SMOOTH_ON={smooth_on:g}")
                        print(f"EVAL_NOTE_SMOOTH_OFF={smooth_off:g}")
                    if args.tune_peak_reach is not None:
                        print(f"EVAL_NOTE_PEAK_REACH={note_peak_reach}")
        else:
            print(f"\nMean framewise F1 over {len(per_sample)} samples at threshold {threshold:.4f}: {mean_f1:.6f}")
            results = {"mean_f1": mean_f1, "threshold": threshold, "per_sample_f1": per_sample, "split": args.split,
                       "num_samples": len(per_sample), "model": args.model, "model_type": args.model_type}
            if notes is not None:
                m = notes["mean"]
                print(f"Mean note F1 ({args.decoder} decoder, {args.note_reference} reference): onset {m['onset_f1']:.6f}, onset+offset {m['onset_offset_f1']:.6f}")
                results["note_metrics"] = {"decoder": args.decoder, "note_reference": args.note_reference,
                                           "onset_threshold": note_onset_threshold,
                                           **notes}
                if note_offset_threshold is not None:
                    results["note_metrics"]["offset_threshold"] = note_offset_threshold
                if args.tune_note_thresholds or args.tune_note_decoder:
                    results["note_metrics"].update(threshold=note_threshold, tuned_objective=args.tune_note_objective)
                if args.tune_note_decoder:
                    results["note_metrics"].update(min_note_ms=note_min_ms, bridge_gap_ms=note_gap_ms)
                    if tune_smoothings is not None:
                        results["note_metrics"].update(smooth_on=smooth_on, smooth_off=smooth_off)
                    if args.tune_peak_reach is not None:
                        results["note_metrics"].update(tuned_peak_reach=note_peak_reach)
            os.makedirs(args.out_dir, exist_ok=True)
            with open(os.path.join(args.out_dir, "results.json"), "w") as f:
                json.dump(results, f)
            print(f"Results written to {os.path.join(args.out_dir, 'results.json')}")
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
