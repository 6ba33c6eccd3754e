"""Cache-free data path measurements (profiles/rawdata_*): store build time and bytes, the GPU time of one training
batch's featurisation (MaestroDataset.get_batch: mel + labels of B chunks), and train_cnn.py's epoch chunks/s from the raw
recordings against the preprocessed cache of the same synthetic MAESTRO tree.

    python tools/rawdata_bench.py --out rawdata.json                             # everything
    python tools/rawdata_bench.py --featurise_only --iters 50                     # under rocprofv3 --kernel-trace --stats

With --augment the featurisation is also timed with rawdata.Augment (10 cents, 20..40 dB), the augmentation launches are timed
on their own beside mt_mel_db_windows_f32 over the same batch, and train_cnn.py runs once more with --augment_* .
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_tree(root, n_rec, seconds, rate=22050):
    from scipy.io import wavfile
    from music_transcription_amd import transcribe as TR
    os.makedirs(os.path.join(root, "2004"), exist_ok=True)
    rng = np.random.default_rng(0)
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for i in range(n_rec + 2):
        name, split = (f"r{i}", "train") if i < n_rec else (f"v{i}", "validation")
        n = int(seconds * rate)
        t = np.arange(n) / rate
        sig = 0.3 * np.sin(2 * np.pi * (110.0 + 7 * i) * t) + 0.02 * rng.standard_normal(n)
        wavfile.write(os.path.join(root, "2004", f"{name}.wav"), rate, (sig * 32767).astype(np.int16))
        notes = [(30 + (k * 5) % 60, s, s + 0.7) for k, s in enumerate(np.arange(0.0, seconds - 1.0, 0.25))]
        TR.write_midi(notes, os.path.join(root, "2004", f"{name}.midi"))
        rows.append(f"X,Y,{split},2004,2004/{name}.midi,2004/{name}.wav,{seconds}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


def featurise(root, n_mels, batch, iters, augment=False):
    import torch
    import music_transcription_amd as mta
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = mta.MaestroDataset(root, split="train", n_mels=n_mels, chunk_length=30.0)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    idx = [list(range(k, k + batch)) for k in range(0, len(ds) - batch + 1, batch)]
    for b in idx[:3]:
        ds.get_batch(b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        ds.get_batch(idx[k % len(idx)])
    e1.record()
    torch.cuda.synchronize()
    res = {"recordings": len(ds.rows), "chunks": len(ds), "store_build_s": round(build_s, 3),
           "store_bytes": int(ds.store.resident_bytes), "store_capacity_bytes": int(ds.store.capacity * 4),
           "batch": batch, "n_mels": n_mels, "get_batch_ms_stream": round(e0.elapsed_time(e1) / iters, 4)}
    if augment:
        res["augment"] = augment_times(root, n_mels, batch, iters, idx)
    return res


def _timed(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def augment_times(root, n_mels, batch, iters, idx):
    """Stream time of an augmented get_batch, and of its launches one by one on one batch: mt_augment_windows without and with
    noise, and mt_mel_db_windows_f32 over the augmented buffer (the launch it feeds)."""
    import torch
    import music_transcription_amd as mta
    from music_transcription_amd import _lib, rawdata as RD
    lib, ptr = _lib.lib, _lib.ptr
    ds = mta.MaestroDataset(root, split="train", n_mels=n_mels, chunk_length=30.0,
                            augment=mta.Augment(pitch_cents=10.0, snr_db=(20.0, 40.0), generator=torch.Generator().manual_seed(0)))
    k = [0]

    def batch_fn():
        ds.get_batch(idx[k[0] % len(idx)])
        k[0] += 1
    out = {"pitch_cents": 10.0, "snr_db": [20.0, 40.0], "get_batch_ms_stream": _timed(batch_fn, iters)}
    b = np.asarray(idx[0], dtype=np.int64)
    B, dev = len(b), ds.device
    rate, snr, seed = ds.augment.draw(B)
    recs = ds.rec[b]
    offs = ds.store.offsets(recs.tolist())
    win_len = ds.win_len[b]
    L_max = -(-int(win_len.max()) // 4) * 4
    d64 = torch.from_numpy(np.stack([np.array([offs[int(r)] for r in recs], dtype=np.int64) + ds.start[b], rate.view(np.int64),
                                     np.arange(B, dtype=np.int64) * L_max])).to(dev)
    d32 = torch.from_numpy(np.stack([win_len, ds.start[b], np.array(ds.store.n, dtype=np.int64)[recs] - ds.start[b],
                                     ds.t_keep[b]]).astype(np.int32)).to(dev)
    nrel = torch.from_numpy((10.0 ** (-snr / 20.0)).astype(np.float32)).to(dev)
    tab = torch.from_numpy(RD.augment_table().astype(np.float32)).to(dev)
    wave = torch.empty(B * L_max, device=dev)
    ws_bytes = int(lib.mt_augment_ws_bytes(B, L_max))
    ws = torch.empty(ws_bytes // 4, device=dev)
    T_out = int(ds.t_keep[b].max())
    mel = torch.empty(B, 1, n_mels, T_out, device=dev)
    cmax = torch.empty(B, device=dev)
    st = _lib.stream_ptr()

    def aug(noise):
        _lib.check(lib.mt_augment_windows(ptr(ds.store.buf), ptr(d64[0]), ptr(d32[0]), ptr(d32[1]), ptr(d32[2]), ptr(d64[1]), int(rate.min()),
                                          int(rate.max()), ptr(nrel) if noise else None, seed, ptr(tab), B, L_max, ptr(wave),
                                          ptr(ws) if noise else None, ws_bytes if noise else 0, st), "mt_augment_windows")

    def mel_fn():
        _lib.check(lib.mt_mel_db_windows_f32(ptr(ds.fe.plan), ds.fe.desc, ptr(wave), ptr(d64[2]), ptr(d32[0]), ptr(d32[0]), B,
                                             int(win_len.max()), T_out, ptr(d32[3]), ptr(mel), ptr(cmax), st), "mt_mel_db_windows_f32")
    out["launch_ms"] = {"augment_resample": _timed(lambda: aug(False), iters), "augment_resample_and_noise": _timed(lambda: aug(True), iters),
                        "mel_db_windows_over_augmented": _timed(mel_fn, iters)}
    out["samples_per_batch"] = int(win_len.sum())
    return out


def train_rate(root, cache, n_mels, batch, hidden, epochs, model, augment=False):
    out = {}
    common = [sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--epochs", str(epochs), "--batch_size", str(batch),
              "--n_mels", str(n_mels), "--hidden_size", str(hidden), "--num_layers", "3", "--model", model, "--seed", "0",
              "--save_every", "1000"]
    raw = ["--cached_dir", cache + "_absent", "--root_dir", root, "--chunk_length", "30"]
    runs = [("cache", ["--cached_dir", cache]), ("raw", raw)]
    if augment:
        runs.append(("raw_augmented", raw + ["--augment_pitch_cents", "10", "--augment_snr_db", "20", "40"]))
    for tag, extra in runs:
        run_dir = tempfile.mkdtemp()
        try:
            r = subprocess.run(common + extra + ["--run_dir", run_dir], capture_output=True, text=True, timeout=1800)
        finally:
            shutil.rmtree(run_dir, ignore_errors=True)
        if r.returncode != 0:
            raise SystemExit(f"train_cnn.py ({tag}) failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        out[tag] = {"chunks_per_s_by_epoch": [x["chunks_per_s"] for x in recs], "train_loss": [x["train_loss"] for x in recs]}
    c = np.median(out["cache"]["chunks_per_s_by_epoch"][1:])
    r_ = np.median(out["raw"]["chunks_per_s_by_epoch"][1:])
    out["median_after_first_epoch"] = {"cache": float(c), "raw": float(r_), "raw_over_cache": round(float(r_ / c), 4)}
    if augment:
        a = float(np.median(out["raw_augmented"]["chunks_per_s_by_epoch"][1:]))
        out["median_after_first_epoch"].update({"raw_augmented": a, "raw_augmented_over_raw": round(a / float(r_), 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=125.0)
    ap.add_argument("--n_mels", type=int, default=320)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--model", default="cnn_rnn")
    ap.add_argument("--featurise_only", action="store_true")
    ap.add_argument("--augment", action="store_true", help="also measure the augmented data path (rawdata.Augment)")
    args = ap.parse_args()
    import music_transcription_amd  # noqa: F401  (sets GPU_MAX_HW_QUEUES before the runtime starts)
    work = tempfile.mkdtemp()
    try:
        run(args, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def run(args, work):
    root = os.path.join(work, "maestro")
    n_rec = args.recordings if not args.featurise_only else 8
    make_tree(root, n_rec, args.seconds)
    res = {"tree": {"recordings": n_rec, "seconds": args.seconds, "wav_rate": 22050}}
    res["featurise"] = featurise(root, args.n_mels, args.batch, args.iters, args.augment)
    if not args.featurise_only:
        from music_transcription_amd import preprocess as P
        cache = os.path.join(work, "cache")
        t0 = time.perf_counter()
        for split in ("train", "validation"):
            P.preprocess_and_cache(root, cache, 30.0, 0.0, args.n_mels, 16000, 512, split)
        res["cache_build_s"] = round(time.perf_counter() - t0, 3)
        res["train"] = train_rate(root, cache, args.n_mels, args.batch, args.hidden, args.epochs, args.model, args.augment)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
