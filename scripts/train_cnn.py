#!/usr/bin/env python3
"""BASELINE.json configs[3]: chunked training of the CNN-RNN transcriber from a preprocessed cache, data-parallel
over the GPUs of one node (the training half of the reference's scripts/train_cnn.py:86-372, same flag names).

    python scripts/train_cnn.py --cached_dir cached_dataset --batch_size 16 --epochs 25
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/train_cnn.py ...
    python scripts/train_cnn.py --root_dir maestro-v3.0.0 --chunk_length 30 --chunk_overlap 0.25    # no cache needed

Data source: the cache under --cached_dir when it exists and its metadata's chunk_length / overlap equal the request (a
chunk flag left out takes the cache's value, so invocations without them train from the cache as before); otherwise the
recordings under --root_dir, decoded onto the GPU once and featurised per step (MaestroDataset + DeviceBatchLoader,
music_transcription_amd/rawdata.py), where --subset_size counts recordings as in the reference.  Full-file training
(no --chunk_length and no usable cache) is refused before the first step.  `--train_all_heads --onset_labels midi` trains the
onset head against the MIDI note-ons (a key struck again under the pedal or without a gap gets its onset) instead of the rising
edges of the label roll; cache records hold no note list, so it always reads the recordings under --root_dir.
`--onset_target regress [--onset_width J]` (with the two flags above) trains the onset head against a triangle of J frames around each
note-on's true time instead of one hot cell, so that `--refine-onsets` can recover sub-frame onsets at decode time (DESIGN.md 6c
"Sub-frame onsets"); the training set only, the validation loss keeps the point target.
`--augment_pitch_cents X` and `--augment_snr_db LO HI` (either or both) augment the training set on the GPU: each chunk is played at
a speed within +-X cents and gets white noise at a signal-to-noise ratio drawn from [LO, HI] dB, the labels moving with the audio
(rawdata.Augment).  They work on the waveform, so they too read the recordings under --root_dir; validation is never augmented.
`--pos_weight`, `--focal_gamma` and `--head_weights` (FRAME ONSET OFFSET each, or one value) train with the class-weighted / focal loss of
ops.heads_loss in one fused kernel and add the per-head training losses to the epoch line; the validation loss stays plain BCE.
`--ema_decay D` keeps an exponential moving average of the weights as one more stream of the fused optimizer pass, validates it too
(`val_loss_ema`) and writes `model_best_ema.pth`, `model_ema_epoch_N.pth` and `model_final_ema.pth` beside the live checkpoints, in the
same format.  `--warmup_steps N`, `--lr_decay cosine` and `--min_lr X` schedule the learning rate over epochs x steps per epoch.  Beside
every numbered and final checkpoint rank 0 writes `train_state.pth` (optimizer moments and step count, the average, best losses,
history, RNG state); `--resume_state PATH` continues from it at the next epoch, where `--resume` restores the weights only.

One process per GPU.  Every step is the HIP training step (train-mode forward, backward, fused clip + Adam); with more
than one rank each rank draws its own shard of the shuffled chunk indices (DistributedSampler) and the flat gradient
is all-reduced (mean) over RCCL before the clip, so all ranks hold identical weights.  Checkpoints are plain
`state_dict` files that the reference's TranscriptionModel loads unchanged, under the reference's names
(scripts/train_cnn.py:345-358): `checkpoints/model_epoch_N.pth` every --save_every epochs and after the last one,
`checkpoints/model_best.pth` whenever the validation loss improves, `checkpoints/model_final.pth` at the end.  Background
re-execution, run-directory bookkeeping and loss plots of the reference script are out of scope.
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# The training step overlaps its weight-gradient work on two side streams; streams that share a hardware queue run one after the other.  With 32
# queues (the runtime's default is 4) no two of a training process's streams share one (profiles/r04_train_large_stream_mapping.txt).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cached_dir", default="cached_dataset")
    ap.add_argument("--root_dir", default="maestro-v3.0.0", help="MAESTRO root, used when the cache is missing or does not match")
    ap.add_argument("--year", default=None, help="year filter of the raw recordings (e.g. 2017)")
    ap.add_argument("--chunk_length", type=float, default=None, help="chunk length in seconds (default: the cache's)")
    ap.add_argument("--chunk_overlap", type=float, default=None, help="overlap ratio between training chunks (default: the cache's, else 0.0)")
    ap.add_argument("--subset_size", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=8, help="per GPU")
    ap.add_argument("--epochs", type=int, default=25)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--save_every", type=int, default=10)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--start_epoch", type=int, default=1)
    ap.add_argument("--model", default="cnn_rnn")
    ap.add_argument("--n_mels", type=int, default=320)
    ap.add_argument("--hidden_size", type=int, default=512)
    ap.add_argument("--num_layers", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--use_attention", action="store_true", default=True, help="attention block (cnn_rnn_large only)")
    ap.add_argument("--no_attention", action="store_false", dest="use_attention")
    ap.add_argument("--use_onset_offset_heads", action="store_true", default=True, help="onset / offset heads (cnn_rnn_large only)")
    ap.add_argument("--no_onset_offset_heads", action="store_false", dest="use_onset_offset_heads")
    ap.add_argument("--train_all_heads", action="store_true",
                    help="train the onset and offset heads too: loss 0.5 frame + 0.25 onset + 0.25 offset (cnn_rnn_large with heads "
                         "only).  Default off = the reference's frame-only loss, which leaves the onset head untrained, so "
                         "--decoder onset is meaningless on such a checkpoint")
    ap.add_argument("--onset_labels", choices=["roll", "midi"], default="roll",
                    help="onset targets of --train_all_heads: roll = rising edges of the label roll (default); midi = the MIDI note-ons, "
                         "re-struck keys included.  midi reads the recordings under --root_dir even where a cache matches (cache records "
                         "hold no note list)")
    ap.add_argument("--onset_target", choices=["point", "regress"], default="point",
                    help="training set only, with --train_all_heads --onset_labels midi: point = one hot cell per note-on (default); regress = "
                         "a triangle of --onset_width frames around the true onset time, from which --refine-onsets / --refine_onsets "
                         "recover sub-frame onsets at decode time.  The validation loss keeps the point target")
    ap.add_argument("--onset_width", type=int, default=2, metavar="J", help="half-width of the --onset_target regress triangle in frames (2..8)")
    ap.add_argument("--augment_pitch_cents", type=float, default=None, metavar="X",
                    help="training set only: play each chunk at a speed drawn from +-X cents (0..50; pitch and tempo move together, "
                         "labels follow).  Reads the recordings under --root_dir even where a cache matches")
    ap.add_argument("--augment_snr_db", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="training set only: add white noise at a signal-to-noise ratio drawn from [LO, HI] dB per chunk.  Reads the "
                         "recordings under --root_dir even where a cache matches")
    heads3 = ("FRAME", "ONSET", "OFFSET")
    ap.add_argument("--pos_weight", type=float, nargs="+", default=None, metavar="W",
                    help="training loss: weight of the positive class per head, FRAME ONSET OFFSET (torch's pos_weight; > 0, default 1 1 1).  "
                         "One value for --model cnn_rnn or without --train_all_heads")
    ap.add_argument("--focal_gamma", type=float, nargs="+", default=None, metavar="G",
                    help="training loss: focal-loss exponent per head, FRAME ONSET OFFSET (0..8, default 0 0 0 = no focusing).  One value "
                         "for --model cnn_rnn or without --train_all_heads")
    ap.add_argument("--head_weights", type=float, nargs="+", default=None, metavar="H",
                    help="training loss: weight of each head's term, FRAME ONSET OFFSET (>= 0, default 0.5 0.25 0.25; --train_all_heads only)")
    ap.add_argument("--ema_decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the weights (0 <= D < 1, e.g. 0.999) inside the fused optimizer pass; adds "
                         "val_loss_ema to the epoch line and writes model_best_ema.pth, model_ema_epoch_N.pth and model_final_ema.pth")
    ap.add_argument("--warmup_steps", type=int, default=0, metavar="N", help="linear learning-rate warm-up over the first N optimizer steps")
    ap.add_argument("--lr_decay", choices=["none", "cosine"], default="none",
                    help="cosine: after the warm-up the learning rate falls along a half cosine to --min_lr at the run's last step "
                         "(epochs x steps per epoch)")
    ap.add_argument("--min_lr", type=float, default=0.0, metavar="X", help="where --lr_decay cosine ends (default 0)")
    ap.add_argument("--resume_state", default=None, metavar="PATH",
                    help="continue a run from its train_state.pth: optimizer moments and step count, weight average, best validation "
                         "losses, history and RNG state, with the weights of model_epoch_N.pth beside it (N = the state's epoch).  "
                         "--resume alone restores weights only")
    ap.add_argument("--run_dir", default="outputs/train_cnn")
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    # the weighted / focal training loss (music_transcription_amd.LossConfig); the validation loss stays plain BCE
    loss_kw = {}
    for flag, field, ok, rng in (("--pos_weight", "pos_weight", lambda v: v > 0, "> 0"), ("--focal_gamma", "focal_gamma", lambda v: 0 <= v <= 8, "within 0..8"),
                                 ("--head_weights", "head_weights", lambda v: v >= 0, ">= 0")):
        vals = getattr(args, field)
        if vals is None:
            continue
        if len(vals) == 3 and not args.train_all_heads:
            ap.error(f"{flag} {' '.join(heads3)} sets the three heads and needs --train_all_heads (one value without it)")
        if field == "head_weights" and not args.train_all_heads:
            ap.error("--head_weights weighs the three heads against each other and needs --train_all_heads")
        if len(vals) not in (1, 3):
            ap.error(f"{flag} takes one value or three ({' '.join(heads3)}), got {len(vals)}")
        if not all(v == v and abs(v) != float("inf") and ok(v) for v in vals):
            ap.error(f"{flag}: every value must be finite and {rng}")
        loss_kw[field] = tuple(vals) if len(vals) == 3 else vals[0]
    if args.train_all_heads and (args.model not in ("cnn_rnn_large", "large") or not args.use_onset_offset_heads):
        print("Error: --train_all_heads needs --model cnn_rnn_large with its onset / offset heads (not --no_onset_offset_heads)",
              file=sys.stderr)
        return 2
    midi_onsets = args.onset_labels == "midi"
    if midi_onsets and not args.train_all_heads:
        print("Error: --onset_labels midi sets the onset head's targets and needs --train_all_heads", file=sys.stderr)
        return 2
    if args.onset_target == "regress":
        if not (midi_onsets and args.train_all_heads):
            print("Error: --onset_target regress builds the onset head's targets from the MIDI note-on times and needs "
                  "--train_all_heads --onset_labels midi", file=sys.stderr)
            return 2
        if not 2 <= args.onset_width <= 8:
            print("Error: --onset_width must lie in 2..8 frames", file=sys.stderr)
            return 2

    if args.resume and args.resume_state:
        print("Error: --resume (weights only) and --resume_state (the whole training state) cannot be combined", file=sys.stderr)
        return 2
    if args.ema_decay is not None and not 0.0 <= args.ema_decay < 1.0:
        print("Error: --ema_decay must lie in [0, 1)", file=sys.stderr)
        return 2
    scheduled = args.warmup_steps > 0 or args.lr_decay == "cosine"
    if args.warmup_steps < 0 or not 0.0 <= args.min_lr <= args.lr or (args.min_lr > 0.0 and args.lr_decay != "cosine"):
        print("Error: --warmup_steps must be >= 0 and --min_lr within [0, --lr]; --min_lr needs --lr_decay cosine", file=sys.stderr)
        return 2
    if args.resume_state and not os.path.exists(args.resume_state):
        print(f"Error: --resume_state {args.resume_state} not found", file=sys.stderr)
        return 2
    extended = args.ema_decay is not None or scheduled or args.resume_state is not None      # the epoch line gains lr and opt_step

    augmenting = args.augment_pitch_cents is not None or args.augment_snr_db is not None
    if augmenting:
        if not 0.0 <= (args.augment_pitch_cents or 0.0) <= 50.0:
            print("Error: --augment_pitch_cents must be within 0..50 (the labels' pitches never change)", file=sys.stderr)
            return 2
        if args.augment_snr_db is not None and not 0.0 <= args.augment_snr_db[0] <= args.augment_snr_db[1]:
            print("Error: --augment_snr_db needs 0 <= LO <= HI", file=sys.stderr)
            return 2

    import pickle
    meta_path = os.path.join(args.cached_dir, "train_metadata.pkl")
    meta = None
    if os.path.exists(meta_path):
        with open(meta_path, "rb") as f:
            meta = pickle.load(f)
    if meta is not None:
        chunk_length = args.chunk_length if args.chunk_length is not None else meta.get("chunk_length")
        overlap = args.chunk_overlap if args.chunk_overlap is not None else meta.get("overlap")
        use_cache = meta.get("chunk_length") == chunk_length and meta.get("overlap") == overlap
    else:
        chunk_length, overlap, use_cache = args.chunk_length, args.chunk_overlap or 0.0, False
    cache_matches = use_cache
    if midi_onsets or augmenting:
        use_cache = False
    if not use_cache and chunk_length is None:
        print("Error: full-file training is not supported (the training recurrence takes chunk-length sequences): "
              "pass --chunk_length (e.g. 30.0) or a matching --cached_dir", file=sys.stderr)
        return 2
    if midi_onsets or augmenting:
        needs = "--onset_labels midi reads the MIDI note lists" if midi_onsets else "--augment_* reads the waveforms"
        from music_transcription_amd.preprocess import read_maestro_csv
        try:
            n_rec = len(read_maestro_csv(args.root_dir, "train", args.year, args.subset_size, None))
        except (OSError, ValueError) as e:
            n_rec, why_none = 0, str(e)
        else:
            why_none = "its csv lists no train recordings"
        if n_rec == 0:
            print(f"Error: {needs} of the recordings under --root_dir, and {args.root_dir} "
                  f"has none ({why_none})", file=sys.stderr)
            return 2

    import torch
    import torch.distributed as dist
    from torch.utils.data import DataLoader, Subset
    from torch.utils.data.distributed import DistributedSampler
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    backend = os.environ.get("MT_BENCH_BACKEND", "nccl")
    dev_index = local if backend == "nccl" else local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    import music_transcription_amd as mta
    from music_transcription_amd import train as T

    if args.model not in ("cnn_rnn", "cnn+rnn", "cnn_rnn_large", "large"):
        raise SystemExit(f"model={args.model}: the HIP training step exists for cnn_rnn and cnn_rnn_large")
    torch.manual_seed(args.seed)                       # same initial weights on every rank
    if use_cache:
        if rank == 0:
            print(f"Data source: cache {args.cached_dir} (chunk_length={chunk_length}, overlap={overlap})", flush=True)
        train_ds = mta.CachedMaestroDataset(args.cached_dir, "train")
        val_ds = mta.CachedMaestroDataset(args.cached_dir, "validation")
        if args.subset_size:
            train_ds = Subset(train_ds, range(min(args.subset_size, len(train_ds))))
            val_ds = Subset(val_ds, range(min(max(1, args.subset_size // 4), len(val_ds))))
    else:
        if rank == 0:
            why = "no cache" if meta is None else f"cache has chunk_length={meta.get('chunk_length')}, overlap={meta.get('overlap')}"
            if midi_onsets and cache_matches:
                why = "the cache matches, but --onset_labels midi needs the MIDI note lists and cache records hold none"
            elif augmenting and cache_matches:
                why = "the cache matches, but --augment_* works on the waveforms and cache records hold features only"
            print(f"Data source: raw recordings {args.root_dir} on the GPU (chunk_length={chunk_length}, overlap={overlap}; {why})", flush=True)
        kw_raw = dict(year=args.year, n_mels=args.n_mels, subset_size=args.subset_size, chunk_length=chunk_length, device=dev,
                      onset_labels=args.onset_labels)
        augment = None
        if augmenting:                                 # the training set only; each rank draws its own speeds and noise
            augment = mta.Augment(pitch_cents=args.augment_pitch_cents or 0.0, snr_db=args.augment_snr_db,
                                  generator=torch.Generator().manual_seed(args.seed + rank))
            if rank == 0:
                print(f"Augmentation (training set): pitch +-{augment.pitch_cents} cents, snr_db {augment.snr_db}", flush=True)
        kw_train = {}
        if args.onset_target == "regress":             # the training set only: the validation loss keeps the point target
            kw_train = dict(onset_target="regress", onset_width=args.onset_width)
            if rank == 0:
                print(f"Onset target (training set): regression triangles of {args.onset_width} frames", flush=True)
        train_ds = mta.MaestroDataset(args.root_dir, split="train", overlap=overlap, augment=augment, **kw_raw, **kw_train)
        val_ds = mta.MaestroDataset(args.root_dir, split="validation", overlap=0.0, **kw_raw)
    sampler = DistributedSampler(train_ds, num_replicas=world, rank=rank, shuffle=True, seed=args.seed, drop_last=True) if world > 1 else None
    if use_cache:
        kw = dict(collate_fn=mta.collate_fn, num_workers=args.num_workers, pin_memory=True)
        train_loader = DataLoader(train_ds, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler, drop_last=world > 1, **kw)
        val_loader = DataLoader(val_ds, batch_size=args.batch_size, shuffle=False, **kw)
    else:                                              # batches are built on the GPU in this process: no workers
        train_loader = mta.DeviceBatchLoader(train_ds, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler, drop_last=world > 1)
        val_loader = mta.DeviceBatchLoader(val_ds, batch_size=args.batch_size, shuffle=False)

    model = mta.TranscriptionModel(model_type=args.model, n_mels=args.n_mels, hidden_size=args.hidden_size, num_layers=args.num_layers,
                                   dropout=args.dropout, device=str(dev), use_attention=args.use_attention,
                                   use_onset_offset_heads=args.use_onset_offset_heads)
    start_epoch = args.start_epoch
    if args.resume:
        model.load_state_dict(torch.load(args.resume, map_location=dev))
        m = re.search(r"epoch_(\d+)", os.path.basename(args.resume))
        if m and args.start_epoch == 1:
            start_epoch = int(m.group(1)) + 1
    state = None
    if args.resume_state:                              # every rank: the weights of the state's own epoch, then (below) the optimizer's
        state = torch.load(args.resume_state, map_location="cpu")
        weights = os.path.join(os.path.dirname(os.path.abspath(args.resume_state)), f"model_epoch_{state['epoch']}.pth")
        if not os.path.exists(weights):
            raise SystemExit(f"Error: --resume_state holds the state after epoch {state['epoch']} and needs that epoch's weights, {weights}")
        model.load_state_dict(torch.load(weights, map_location=dev))
        start_epoch = state["epoch"] + 1
    schedule = None
    if scheduled:                                      # the run's length in optimizer steps: epochs x this rank's steps per epoch
        try:
            schedule = mta.LRSchedule(args.lr, warmup_steps=args.warmup_steps, min_lr=args.min_lr,
                                      total_steps=args.epochs * len(train_loader) if args.lr_decay == "cosine" else None)
        except ValueError as e:
            raise SystemExit(f"Error: {e} (epochs x steps per epoch = {args.epochs * len(train_loader)})")
    if args.ema_decay is None and schedule is None:
        opt = mta.make_optimizer(model, lr=args.lr, eps=1e-8, weight_decay=1e-5)
    else:
        opt = mta.make_optimizer(model, lr=args.lr, eps=1e-8, weight_decay=1e-5, ema_decay=args.ema_decay, schedule=schedule)
        if rank == 0:
            print(f"Optimizer: ema_decay {args.ema_decay}, schedule {schedule.params() if schedule else None}", flush=True)
    loss_cfg = mta.LossConfig(**loss_kw) if loss_kw else None
    if loss_cfg is not None and rank == 0:
        print(f"Training loss: head_weights {loss_cfg.head_weights}, pos_weight {loss_cfg.pos_weight}, focal_gamma {loss_cfg.focal_gamma} "
              f"(validation loss: plain BCE)", flush=True)
    ckpt_dir = os.path.join(args.run_dir, "checkpoints")
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    history = []
    best_val_loss = best_val_loss_ema = float("inf")
    if state is not None:
        opt.load_state_dict(state["optimizer"])
        history, best_val_loss, best_val_loss_ema = list(state["history"]), state["best_val_loss"], state["best_val_loss_ema"]
        torch.set_rng_state(state["rng_state"])
        if rank == 0:
            print(f"Resumed from {args.resume_state}: epoch {state['epoch']} done, optimizer step {opt.t}, best val loss {best_val_loss:.4f}",
                  flush=True)

    def save(name):                                    # plain state_dict with the reference's keys (rank 0 only)
        path = os.path.join(ckpt_dir, name)
        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, path)
        return path

    def save_ema(name):                                # the same, with the averaged weights under the model while it is written
        with opt.averaged_weights():
            return save(name)
    state_epoch = [None]

    def save_state(epoch):                             # what --resume_state continues from; one file, overwritten (rank 0 only)
        if state_epoch[0] != epoch:
            torch.save({"epoch": epoch, "optimizer": opt.state_dict(), "best_val_loss": best_val_loss, "best_val_loss_ema": best_val_loss_ema,
                        "history": history, "rng_state": torch.get_rng_state()}, os.path.join(ckpt_dir, "train_state.pth"))
            state_epoch[0] = epoch
    for epoch in range(start_epoch, args.epochs + 1):
        if sampler is not None:
            sampler.set_epoch(epoch)
        t0 = time.perf_counter()
        head_sums = {}

        def log_parts(step, step_loss, norm, parts=None):          # called with parts only under a LossConfig
            for k, v in (parts or {}).items():
                head_sums[k] = head_sums.get(k, 0.0) + v
        train_loss, step_losses = T.train_one_epoch(model, train_loader, opt, dev, max_grad_norm=1.0, all_heads=args.train_all_heads,
                                                    loss=loss_cfg, log=log_parts if loss_cfg is not None else None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        val_loss = T.evaluate(model, val_loader, dev, all_heads=args.train_all_heads) if rank == 0 else float("nan")
        if rank == 0:
            rec = {"epoch": epoch, "train_loss": train_loss, "val_loss": val_loss, "steps": len(step_losses),
                   "chunks_per_s": round(len(step_losses) * args.batch_size * world / max(dt, 1e-9), 2)}
            if args.ema_decay is not None:             # the same validation loop on the averaged weights
                rec["val_loss_ema"] = T.evaluate(model, val_loader, dev, all_heads=args.train_all_heads, optimizer=opt, averaged=True)
            if extended:
                rec.update({"lr": opt.last_lr, "opt_step": opt.t})
            if loss_cfg is not None:                   # mean per-head training loss over the epoch's steps (each times its head weight)
                heads = ("frame", "onset", "offset") if args.train_all_heads else ("frame",)
                rec.update({f"train_{k}_loss": head_sums.get(k, 0.0) / max(len(step_losses), 1) for k in heads})
            history.append(rec)
            print(json.dumps(rec), flush=True)
            numbered = epoch % args.save_every == 0 or epoch == args.epochs
            if numbered:
                print(f"Checkpoint saved to {save(f'model_epoch_{epoch}.pth')}", flush=True)
                if args.ema_decay is not None:
                    save_ema(f"model_ema_epoch_{epoch}.pth")
            if val_loss < best_val_loss:               # best model = lowest validation loss (reference scripts/train_cnn.py:349-354)
                best_val_loss = val_loss
                save("model_best.pth")
                print(f"New best model saved! Val loss: {val_loss:.4f}", flush=True)
            if args.ema_decay is not None and rec["val_loss_ema"] < best_val_loss_ema:
                best_val_loss_ema = rec["val_loss_ema"]
                save_ema("model_best_ema.pth")
                print(f"New best averaged model saved! Val loss: {best_val_loss_ema:.4f}", flush=True)
            if numbered:
                save_state(epoch)
        if world > 1:
            dist.barrier()
    if rank == 0:
        print(f"Final model saved to {save('model_final.pth')}", flush=True)       # reference scripts/train_cnn.py:180,:357
        if args.ema_decay is not None:
            save_ema("model_final_ema.pth")
        if history:
            save_state(history[-1]["epoch"])
        with open(os.path.join(args.run_dir, "history.json"), "w") as f:
            json.dump(history, f)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
