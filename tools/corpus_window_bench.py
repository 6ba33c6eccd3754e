"""The corpus path in chunks against the corpus path in windows (DESIGN.md 6d "The corpus in windows"): corpus.transcribe_shard and
corpus.transcribe_shard_windows in ONE process, on the same synthetic corpus (corpus.synthetic_corpus / synth_recording) and the
same model (cnn_rnn_large 320 / 512 / 3, seeded random weights), alternating, with random reference rolls so that F1 is counted:

  * wall_s of each path per round (the functions' own figure: one device synchronisation at the end), median and spread;
  * windows per chunk;
  * blocking device-to-host copies of each path: calls of torch.Tensor.cpu on a device tensor inside the pass, counted.

    python tools/corpus_window_bench.py [--recordings 177 --hours 20] [--overlap 2] [--rounds 3] [--decoder frame] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=177)
    ap.add_argument("--hours", type=float, default=20.0)
    ap.add_argument("--overlap", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--decoder", choices=["frame", "onset"], default="frame")
    ap.add_argument("--n-mels", type=int, default=320)
    ap.add_argument("--hidden-size", type=int, default=512)
    ap.add_argument("--num-layers", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import music_transcription_amd as mta
    from music_transcription_amd import corpus
    if not torch.cuda.is_available():
        raise SystemExit("corpus_window_bench measures on the GPU only")
    dev = "cuda"
    torch.manual_seed(1234)
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=args.n_mels, hidden_size=args.hidden_size, num_layers=args.num_layers, device=dev)
    for p in model.parameters():
        if p.dim() > 1:
            torch.nn.init.uniform_(p, -0.05, 0.05)
    model.eval()
    durations = corpus.synthetic_corpus(args.recordings, args.hours)
    ids = list(range(args.recordings))
    chunks = {i: corpus.synth_recording(i, durations[i], dev) for i in ids}                 # resident, as scripts/transcribe_corpus.py
    audio = {i: chunks[i].view(-1)[:int(durations[i] * SR)] for i in ids}

    def roll_of(i, frames):
        return (torch.rand(88, frames, device=dev, generator=torch.Generator(device=dev).manual_seed(i)) < 0.04).float()

    common = dict(n_mels=args.n_mels, device=dev, batch=args.batch, streams=args.streams, decoder=args.decoder, reference_roll_of=roll_of,
                  note_metrics=True)
    paths = {"chunks": lambda warm: corpus.transcribe_shard(model, ids, lambda i: chunks[i], warm=warm, **common),
             "windows": lambda warm: corpus.transcribe_shard_windows(model, ids, lambda i: audio[i], overlap_s=args.overlap, warm=warm, **common)}

    copies = {"n": 0}
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        copies["n"] += bool(self.is_cuda)
        return real_cpu(self, *a, **k)

    res = {"recordings": args.recordings, "audio_hours": round(sum(durations) / 3600.0, 2), "overlap_s": args.overlap, "decoder": args.decoder,
           "batch": args.batch, "streams": args.streams, "rounds": args.rounds}
    walls = {k: [] for k in paths}
    for k, fn in paths.items():                              # warm-up: workspaces of every stream, code objects, allocator pools
        fn(True)
    for _ in range(args.rounds):
        for k, fn in paths.items():                          # alternating: drift of the machine hits both alike
            copies["n"] = 0
            torch.Tensor.cpu = counting_cpu
            try:
                r = fn(False)
            finally:
                torch.Tensor.cpu = real_cpu
            walls[k].append(r["wall_s"])
            res[k] = r[k]
            res[k + "_slabs"] = r["slabs"]
            res[k + "_notes"] = r["n_notes"]
            res[k + "_blocking_d2h_copies"] = copies["n"]
            if k == "windows":
                res["groups"] = len(r["groups"])
    for k in paths:
        res[k + "_wall_s"] = [round(w, 4) for w in walls[k]]
        res[k + "_wall_s_median"] = round(float(np.median(walls[k])), 4)
    res["windows_per_chunk"] = round(res["windows"] / res["chunks"], 4)
    res["windows_over_chunks_wall"] = round(res["windows_wall_s_median"] / res["chunks_wall_s_median"], 4)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
