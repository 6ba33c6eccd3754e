#!/usr/bin/env python3
"""Inference CLI with the reference's interface (main.py:290-362):

    python main.py audio_file model_file [-o OUT.mid] [-d {cpu,cuda}] [-t THRESHOLD] [--decoder {frame,onset,onset_offset}] [--overlap SECONDS]
                   [--min-note-ms MS] [--bridge-gap-ms MS] [--smooth-on LOGITS] [--smooth-off LOGITS] [--refine-onsets] [--refine-reach N]

Exit code 1 with a message when a file is missing or transcription fails.  The checkpoint must be a
CNNRNNModelLarge(320, 512, 3) state_dict as in the reference (main.py:16-20); --model-type/--n-mels/
--hidden-size/--num-layers are additive overrides.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description="Transcribe audio files to MIDI using trained music transcription model")
    ap.add_argument("audio_file", type=str, help="Path to input audio file (wav)")
    ap.add_argument("model_file", type=str, help="Path to model checkpoint file (.pth)")
    ap.add_argument("-o", "--output", type=str, default=None, help="Path to output MIDI file (default: <audio_name>_transcription.mid)")
    ap.add_argument("-d", "--device", type=str, choices=["cpu", "cuda"], default=None, help="Device to use for inference (default: auto-detect)")
    ap.add_argument("-t", "--threshold", type=float, default=0.5, help="Threshold for note predictions (default: 0.5)")
    ap.add_argument("--decoder", choices=["frame", "onset", "onset_offset"], default="frame",
                    help="frame: notes are runs of active frames (default); onset: notes start at rising edges of the onset head and "
                         "last while frame or onset is active; onset_offset: the onset decoder's notes, ended on the frame where the "
                         "offset head fires (both need a cnn_rnn_large checkpoint trained with --train_all_heads)")
    ap.add_argument("--onset-threshold", type=float, default=0.5,
                    help="threshold of the onset head for --decoder onset / onset_offset (default: 0.5)")
    ap.add_argument("--offset-threshold", type=float, default=0.5, help="threshold of the offset head for --decoder onset_offset (default: 0.5)")
    ap.add_argument("--overlap", type=float, default=0.0,
                    help="seconds of overlap between 30 s windows (0.256 to 15; default 0 = the reference's chunk concatenation, which "
                         "places chunk k's notes 16 ms x k late because a 480000-sample chunk spans 937.5 hops but yields 938 frames). "
                         "With an overlap the windows start on the 512-sample hop and their centres are stitched on the recording's "
                         "own frame grid: no drift, and no cold network start at the chunk boundaries")
    ap.add_argument("--min-note-ms", type=float, default=0.0,
                    help="note cleanup in the decoder: drop every note shorter than this many milliseconds (32 ms frames; at most 2048; "
                         "default 0 = keep all)")
    ap.add_argument("--bridge-gap-ms", type=float, default=0.0,
                    help="note cleanup in the decoder: a dropout of the activity no longer than this many milliseconds, with activity "
                         "directly before and after it, does not end the note (below 2048; default 0 = none).  Gaps are bridged first, "
                         "then short notes dropped")
    ap.add_argument("--smooth-on", type=float, default=0.0,
                    help="frame smoothing before the decoder: per pitch, the frame head is replaced by the best path of a two-state "
                         "(off / on) HMM whose evidence is logit - logit(threshold) per frame; switching a pitch on costs this many "
                         "logits (0 to 64; default 0).  A blip survives only if its evidence pays for switching on and off again")
    ap.add_argument("--smooth-off", type=float, default=0.0,
                    help="frame smoothing: the cost in logits of switching a pitch off (0 to 64; default 0).  A dropout is bridged only "
                         "if its counter-evidence is smaller than --smooth-on + --smooth-off.  Both 0 = no smoothing.  Chunks and "
                         "--overlap alike; the onset and offset heads are not smoothed; note cleanup then sees the smoothed activity")
    ap.add_argument("--refine-onsets", action="store_true",
                    help="--decoder onset / onset_offset: give every note a sub-frame start time from the onset head's values around "
                         "its peak (a head trained with train_cnn.py --onset_target regress).  Chunks and --overlap alike, but on "
                         "concatenated chunks the frame grid itself drifts 16 ms per chunk: --overlap is where sub-frame times mean something")
    ap.add_argument("--refine-reach", type=int, default=2,
                    help="--refine-onsets: frames the peak search may walk from a note's first frame (0..8; default 2)")
    ap.add_argument("--onset-detect", choices=["edge", "peak"], default="edge",
                    help="--decoder onset / onset_offset: where a note opens.  edge (default): at every rising edge of the thresholded "
                         "onset head; peak: at every local maximum of the onset logits within --peak-reach frames that passes "
                         "--onset-threshold (a head trained with train_cnn.py --onset_target regress: the edge rule merges a key "
                         "re-struck within --onset_width frames into one note and stamps notes early)")
    ap.add_argument("--peak-reach", type=int, default=1,
                    help="--onset-detect peak: a peak must be the largest logit of this many frames on either side (1..8; default 1)")
    ap.add_argument("--model-type", default="cnn_rnn_large")
    ap.add_argument("--n-mels", type=int, default=320)
    ap.add_argument("--hidden-size", type=int, default=512)
    ap.add_argument("--num-layers", type=int, default=3)
    args = ap.parse_args()
    try:
        from music_transcription_amd.notes import check_smoothing, cleanup_frames
        min_note_frames, bridge_frames = cleanup_frames(args.min_note_ms, args.bridge_gap_ms)
        smooth_on, smooth_off = check_smoothing(args.smooth_on, args.smooth_off)
        if args.refine_onsets:
            from music_transcription_amd.transcribe import check_refine_decoder
            check_refine_decoder(True, args.decoder, args.refine_reach)
        if args.onset_detect != "edge" or args.peak_reach != 1:
            from music_transcription_amd.transcribe import check_detect_decoder
            check_detect_decoder("peak", args.decoder, args.peak_reach)
    except ValueError as e:
        ap.error(str(e))
    if not os.path.exists(args.audio_file):
        print(f"Error: Audio file not found: {args.audio_file}")
        sys.exit(1)
    if not os.path.exists(args.model_file):
        print(f"Error: Model file not found: {args.model_file}")
        sys.exit(1)
    print("=" * 60 + "\nMusic Transcription Pipeline\n" + "=" * 60)
    try:
        from music_transcription_amd.transcribe import transcribe_audio
        out = transcribe_audio(args.audio_file, args.model_file, args.output, args.device, args.threshold,
                               decoder=args.decoder, onset_threshold=args.onset_threshold, overlap=args.overlap,
                               offset_threshold=args.offset_threshold, min_note_frames=min_note_frames, bridge_frames=bridge_frames,
                               smooth_on=smooth_on, smooth_off=smooth_off, refine_onsets=args.refine_onsets, refine_reach=args.refine_reach,
                               onset_detect=args.onset_detect, peak_reach=args.peak_reach,
                               model_type=args.model_type, n_mels=args.n_mels, hidden_size=args.hidden_size,
                               num_layers=args.num_layers)
        print("=" * 60 + f"\nTranscription completed successfully!\nOutput: {out}\n" + "=" * 60)
    except Exception as e:
        print(f"Error during transcription: {e}")
        import traceback
        traceback.print_exc()
        sys.exit(1)


if __name__ == "__main__":
    main()
