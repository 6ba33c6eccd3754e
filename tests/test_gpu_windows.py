"""GPU tests of whole recordings in overlapping windows (windows.py, csrc/stitch.hip): mt_stitch_windows against numpy, the stitched
grid against one mel over the whole recording, transcribe_windows against the chunk path run on the same windows, and the two CLIs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rawdata_cpu import cc64, note, smf  # noqa: E402

pytestmark = pytest.mark.gpu
SR, HOP, W, TW = 16000, 512, 480000, 938


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _stitch(src, dst, rows, f0, lo, hi):
    from music_transcription_amd import _lib
    dev = src.device
    d_rows = torch.tensor(rows, dtype=torch.int32, device=dev)
    d_f0 = torch.tensor(f0, dtype=torch.int64, device=dev)
    d_lo = torch.tensor(lo, dtype=torch.int32, device=dev)
    d_hi = torch.tensor(hi, dtype=torch.int32, device=dev)
    Bw, P, Tw = src.shape
    R, _, T_dst = dst.shape
    _lib.check(_lib.lib.mt_stitch_windows(_lib.ptr(src), Bw, P, Tw, _lib.ptr(d_rows), _lib.ptr(d_f0), _lib.ptr(d_lo), _lib.ptr(d_hi),
                                          _lib.ptr(dst), R, T_dst, _lib.stream_ptr()), "mt_stitch_windows")


def _plans(ns, overlap):
    from music_transcription_amd.windows import plan_windows
    rows, f0, lo, hi, starts = [], [], [], [], []
    for r, n in enumerate(ns):
        p = plan_windows(n, overlap)
        for a, l, h in zip(p.start, p.lo, p.hi):
            rows.append(r)
            f0.append(int(a))
            lo.append(int(l))
            hi.append(int(h))
            starts.append((r, int(a)))
    return rows, f0, lo, hi, starts


# ------------------------------------------------------------------ 1. the kernel against numpy
def test_stitch_equals_numpy(mta):
    from music_transcription_amd import _lib
    rng = np.random.default_rng(3)
    ns = [2_300_123, 480_000, 1_000_001]
    rows, f0, lo, hi, _ = _plans(ns, 2.0)
    order = rng.permutation(len(rows))                       # windows of the 3 recordings interleaved in the batch
    rows, f0, lo, hi = [[x[i] for i in order] for x in (rows, f0, lo, hi)]
    Bw, P = len(rows), 88
    src = torch.from_numpy(rng.standard_normal((Bw, P, TW)).astype(np.float32)).cuda()
    T_dst = 1 + max(ns) // HOP + 5
    dst = torch.full((3, P, T_dst), float("nan"), device="cuda")
    _stitch(src, dst, rows, f0, lo, hi)
    want = np.full((3, P, T_dst), np.nan, np.float32)
    s = src.cpu().numpy()
    for b in range(Bw):
        want[rows[b], :, f0[b] + lo[b]:f0[b] + hi[b]] = s[b, :, lo[b]:hi[b]]
    got = dst.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    for r, n in enumerate(ns):                               # every frame of each recording's grid written, none past it
        assert not np.isnan(got[r, :, :1 + n // HOP]).any() and np.isnan(got[r, :, 1 + n // HOP:]).all()

    # bad dimensions and null pointers are refused
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    t64 = torch.zeros(4, dtype=torch.int64, device="cuda")
    f = _lib.lib.mt_stitch_windows
    p = _lib.ptr
    st = _lib.stream_ptr()
    good = [p(src), 1, P, TW, p(t), p(t64), p(t), p(t), p(dst), 3, T_dst, st]
    assert f(*good) == 0
    for k, bad in [(1, -1), (1, 65536), (2, 0), (3, 0), (9, 0), (10, 0), (10, -5)] + [(k, None) for k in (0, 4, 5, 6, 7, 8)]:
        args = list(good)
        args[k] = bad
        assert f(*args) != 0, (k, bad)
        assert "mt_stitch_windows" in _lib.last_error()
    torch.cuda.synchronize()


def test_stitch_past_2g_floats(mta):
    """A destination of 3 x 1 x (2^30 + 2^20) floats: row 2 starts past 2^31 floats (64-bit indexing)."""
    T_dst = (1 << 30) + (1 << 20)
    dst = torch.full((3, 1, T_dst), float("nan"), device="cuda")
    src = torch.arange(2 * TW, dtype=torch.float32, device="cuda").view(2, 1, TW)
    f0 = [T_dst - TW, 123]
    _stitch(src, dst, [2, 1], f0, [5, 0], [TW, 17])
    tail = dst[2, 0, T_dst - 2 * TW:].cpu().numpy()
    assert np.isnan(tail[:TW + 5]).all() and np.array_equal(tail[TW + 5:], np.arange(5, TW, dtype=np.float32))
    head = dst[1, 0, :200].cpu().numpy()
    assert np.isnan(head[:123]).all() and np.array_equal(head[123:140], np.arange(TW, TW + 17, dtype=np.float32))
    assert np.isnan(head[140:]).all()
    assert torch.isnan(dst[0]).all() and torch.isnan(dst[2, 0, :T_dst - 2 * TW]).all()
    del dst
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 2. the grid, model-free
def _audio(seconds, seed):
    """Noise plus decaying tones: every mel bin of every frame within 80 dB of the recording's loudest, so no clamp floor bites."""
    n = int(seconds * SR)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = 0.05 * rng.standard_normal(n)
    for k, f in enumerate((110.0, 440.0 * (seed + 1), 1760.0, 3520.0)):
        y += 0.2 * np.sin(2 * np.pi * f * t + k) * np.exp(-0.7 * (t % (1.3 + 0.4 * k)))
    return torch.from_numpy(y.astype(np.float32)).cuda()


def _window_mel(mta, ys, overlap, n_mels):
    """Every window of every recording featurised in one mt_mel_db_windows_f32 launch, as windows.transcribe_windows does."""
    from music_transcription_amd import _lib
    ns = [int(y.numel()) for y in ys]
    offs, pos = [], 0
    for n in ns:
        offs.append(pos)
        pos += -(-n // 64) * 64
    store = torch.zeros(pos + 64, device="cuda")
    for y, o in zip(ys, offs):
        store[o:o + y.numel()] = y
    rows, f0, lo, hi, starts = _plans(ns, overlap)
    B = len(rows)
    fe = mta.get_frontend(SR, n_mels, HOP, "cuda")
    d64 = torch.tensor([offs[r] + HOP * a for r, a in starts], dtype=torch.int64, device="cuda")
    d32 = torch.tensor([[W] * B, [ns[r] - HOP * a for r, a in starts], [TW] * B], dtype=torch.int32, device="cuda")
    mel = torch.empty(B, 1, n_mels, TW, device="cuda")
    cmax = torch.empty(B, device="cuda")
    _lib.check(_lib.lib.mt_mel_db_windows_f32(_lib.ptr(fe.plan), fe.desc, _lib.ptr(store), _lib.ptr(d64), _lib.ptr(d32[0]), _lib.ptr(d32[1]),
                                              B, W, TW, _lib.ptr(d32[2]), _lib.ptr(mel), _lib.ptr(cmax), _lib.stream_ptr()))
    return mel, (rows, f0, lo, hi)


@pytest.mark.parametrize("overlap", [0.5, 2.0, 15.0])
def test_stitched_window_mel_is_the_whole_recording_mel(mta, overlap):
    n_mels = 64
    ys = [_audio(100.0, 0), _audio(47.0, 1)]
    fe = mta.get_frontend(SR, n_mels, HOP, "cuda")
    mel, (rows, f0, lo, hi) = _window_mel(mta, ys, overlap, n_mels)
    Tg = [1 + y.numel() // HOP for y in ys]
    dst = torch.full((2, n_mels, max(Tg)), float("nan"), device="cuda")
    _stitch(mel[:, 0].contiguous(), dst, rows, f0, lo, hi)
    for r, y in enumerate(ys):
        whole, _ = fe(y[None], clamp=False)
        whole = whole[0, 0]
        assert whole.shape[-1] == Tg[r]
        assert (whole.max() - whole.min()).item() < 79.0                 # the premise: no -80 dB floor anywhere
        assert torch.equal(dst[r, :, :Tg[r]], whole), (r, (dst[r, :, :Tg[r]] != whole).nonzero()[:5].tolist())
        assert torch.isnan(dst[r, :, Tg[r]:]).all()


# ------------------------------------------------------------------ 3./4. logits against the chunk path on the same windows
def _cnn_rnn(mta, seed=4, nm=64, H=32, L=2):
    from oracle import model_ref as R
    m = mta.TranscriptionModel("cnn_rnn", n_mels=nm, hidden_size=H, num_layers=L, device="cuda")
    m.load_state_dict(R.make_state_dict("cnn_rnn", nm, H, L, seed=seed), strict=True)
    return m.eval()


def _large(mta, seed=5, nm=32, H=16, L=2):
    from oracle import model_ref as R
    m = mta.TranscriptionModel("cnn_rnn_large", n_mels=nm, hidden_size=H, num_layers=L, dropout=0.0, device="cuda")
    m.load_state_dict(R.make_state_dict("cnn_rnn_large", nm, H, L, seed), strict=True)
    return m.eval()


def _chunk_path_stitched(model, ys, overlap, n_mels, all_heads=False):
    """The windows sliced and zero-padded by hand, through the chunk path (mel with clamp=False + forward with chunk_max_power, as
    transcribe_chunks_to_notes runs it) in one batch, stitched in numpy."""
    from music_transcription_amd.frontend import get_frontend
    rows, f0, lo, hi, starts = _plans([int(y.numel()) for y in ys], overlap)
    chunks = torch.zeros(len(rows), W, device="cuda")
    for b, (r, a) in enumerate(starts):
        seg = ys[r][HOP * a:HOP * a + W]
        chunks[b, :seg.numel()] = seg
    mel, cmax = get_frontend(SR, n_mels, HOP, "cuda")(chunks, clamp=False)
    with torch.no_grad():
        if all_heads:
            h = model.model(mel, chunk_max_power=cmax, return_all_heads=True)
            heads = [h["frame"].cpu().numpy(), h["onset"].cpu().numpy()]
        else:
            heads = [model.model(mel, chunk_max_power=cmax).cpu().numpy()]
    out = []
    for r, y in enumerate(ys):
        Tg = 1 + y.numel() // HOP
        per = []
        for lg in heads:
            roll = np.full((88, Tg), np.nan, np.float32)
            for b in range(len(rows)):
                if rows[b] == r:
                    roll[:, f0[b] + lo[b]:f0[b] + hi[b]] = lg[b, :, lo[b]:hi[b]]
            assert not np.isnan(roll).any()
            per.append(roll)
        out.append(per)
    return out


def test_transcribe_windows_equals_chunk_path_on_the_windows(mta):
    model = _cnn_rnn(mta)
    ys = [_audio(75.0, 2), _audio(20.0, 3)]
    got = mta.transcribe_windows(model, ys, 2.0)
    want = _chunk_path_stitched(model, ys, 2.0, 64)
    for r, y in enumerate(ys):
        assert got[r].shape == (88, 1 + y.numel() // HOP) and got[r].is_cuda
        assert np.array_equal(got[r].cpu().numpy(), want[r][0]), r
    # a slab boundary inside a recording: same stitched roll from slabs of 2 windows as from one slab, up to the batch
    # composition of the forward (tile shapes differ)
    small = mta.transcribe_windows(model, ys, 2.0, batch=2)
    for a, b in zip(small, got):
        assert (a - b).abs().max().item() < 1e-5


def test_transcribe_windows_all_heads(mta):
    model = _large(mta)
    ys = [_audio(75.0, 4), _audio(20.0, 5)]
    got = mta.transcribe_windows(model, ys, 2.0, all_heads=True)
    want = _chunk_path_stitched(model, ys, 2.0, 32, all_heads=True)
    for r in range(2):
        assert np.array_equal(got[r][0].cpu().numpy(), want[r][0]) and np.array_equal(got[r][1].cpu().numpy(), want[r][1]), r
    with pytest.raises(ValueError, match="onset head"):
        mta.transcribe_windows(_cnn_rnn(mta), ys, 2.0, all_heads=True)
    with pytest.raises(ValueError, match="between"):
        mta.transcribe_windows(model, ys, 0.1)


@pytest.mark.parametrize("seconds", [3.3, 29.99, 30.0])
def test_single_window_equals_chunk_path(mta, seconds):
    from music_transcription_amd import transcribe as TR
    model = _cnn_rnn(mta, seed=6)
    y = _audio(seconds, 6)
    n = y.numel()
    chunks, _ = TR.split_into_chunks_device(y)
    assert len(chunks) == 1
    mel, cmax = mta.get_frontend(SR, 64, HOP, "cuda")(chunks, clamp=False)
    with torch.no_grad():
        want = model.model(mel, chunk_max_power=cmax)[0, :, :1 + n // HOP]
    got = mta.transcribe_windows(model, [y], 2.0)[0]
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 5. main.py --overlap
def _run(args, timeout=900, ok=True):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if ok:
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def _mid_threshold(logits):
    return float(np.clip(torch.sigmoid(logits.float().median()).item(), 0.05, 0.95))


@pytest.mark.parametrize("kind", ["cnn_rnn", "cnn_rnn_large"])
def test_main_overlap_writes_the_stitched_notes(mta, tmp_path, kind):
    from scipy.io import wavfile
    from oracle import model_ref as R
    from music_transcription_amd import transcribe as TR
    from music_transcription_amd.notes import heads_to_notes_device
    nm, H, L = (64, 32, 2) if kind == "cnn_rnn" else (32, 16, 2)
    sd = R.make_state_dict(kind, nm, H, L, seed=8)
    ckpt = str(tmp_path / "m.pth")
    torch.save(sd, ckpt)
    y = _audio(70.0, 7)
    wav = str(tmp_path / "x.wav")
    wavfile.write(wav, SR, y.cpu().numpy())
    model = TR.load_model(ckpt, "cuda", model_type=kind, n_mels=nm, hidden_size=H, num_layers=L)
    yd = TR.load_audio_device(wav, SR, "cuda")
    fs = SR / HOP
    dims = ["--model-type", kind, "--n-mels", str(nm), "--hidden-size", str(H), "--num-layers", str(L)]
    if kind == "cnn_rnn":
        frame = mta.transcribe_windows(model, [yd], 2.0)[0]
        thr = _mid_threshold(frame)
        want = TR.notes_from_logits_device(frame[None], thr, fs)
        extra = []
    else:
        frame, onset = mta.transcribe_windows(model, [yd], 2.0, all_heads=True)[0]
        thr, othr = _mid_threshold(frame), _mid_threshold(onset)
        want = heads_to_notes_device(frame[None], onset[None], thr, othr, fs)
        extra = ["--decoder", "onset", "--onset-threshold", repr(othr)]
    assert len(want) > 10
    TR.write_midi(want, str(tmp_path / "want.mid"))
    out = str(tmp_path / "got.mid")
    r = _run([os.path.join(ROOT, "main.py"), wav, ckpt, "-o", out, "-t", repr(thr), "--overlap", "2"] + dims + extra)
    assert "windows of 30.0s" in r.stdout
    assert open(out, "rb").read() == open(tmp_path / "want.mid", "rb").read()
    # --overlap 0 is the chunk concatenation, byte for byte
    base = [os.path.join(ROOT, "main.py"), wav, ckpt, "-t", repr(thr)] + dims + extra
    _run(base + ["-o", str(tmp_path / "plain.mid")])
    _run(base + ["-o", str(tmp_path / "zero.mid"), "--overlap", "0"])
    plain = open(tmp_path / "plain.mid", "rb").read()
    assert plain == open(tmp_path / "zero.mid", "rb").read() and plain != open(out, "rb").read()
    bad = _run(base + ["-o", str(tmp_path / "bad.mid"), "--overlap", "0.1"], ok=False)
    assert bad.returncode != 0 and "between 0.256 s and 15.008 s" in bad.stdout


# ------------------------------------------------------------------ 6./7. scripts/evaluate.py --window_overlap
DURS = {"a": 47.3, "b": 31.5, "c": 64.05, "v": 33.3}


def _tree(root, durs=DURS, rate=44100, channels=2):
    """tests/test_gpu_rawdata.py's synthetic MAESTRO tree, with the WAV rate and channel count as parameters."""
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "2004"), exist_ok=True)
    rng = np.random.default_rng(0)
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for i, (name, d) in enumerate(durs.items()):
        n = int(d * rate)
        t = np.arange(n) / float(rate)
        f = 220.0 * (i + 1)
        sig = 0.3 * np.sin(2 * np.pi * f * t) * np.exp(-0.5 * (t % 1.7)) + 0.02 * rng.standard_normal(n)
        pcm = np.stack([sig, 0.6 * sig], 1) if channels == 2 else sig
        wavfile.write(os.path.join(root, "2004", f"{name}.wav"), rate, (pcm * 32767).astype(np.int16))
        ev = []
        for k, s in enumerate(np.arange(0.0, d - 1.0, 0.9)):
            ev += note(0, 40 + (k * 7) % 50, int(s * 2000), int((s + 0.5 + 0.3 * (k % 3)) * 2000))   # 2000 ticks per second
        for k in range(int(d // 5)):
            ev += cc64(0, 10000 * k + 2000, 100) + cc64(0, 10000 * k + 7000, 0)
        with open(os.path.join(root, "2004", f"{name}.midi"), "wb") as fh:
            fh.write(smf([[], ev, note(9, 38, 0, 900)]))
        split = "validation" if name == "v" else "train"
        rows.append(f"X,Y,{split},2004,2004/{name}.midi,2004/{name}.wav,{d}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")


def _value(out, key):
    line = [x for x in out.splitlines() if x.startswith(key + "=")]
    assert len(line) == 1, out
    return float(line[0].split("=")[1])


def test_evaluate_window_overlap(mta, tmp_path):
    from oracle import model_ref as R
    from music_transcription_amd import evaluate as E
    root = str(tmp_path / "tree")
    _tree(root)
    nm, H, L = 64, 32, 2
    sd = R.make_state_dict("cnn_rnn", nm, H, L, seed=4)
    ckpt = str(tmp_path / "m.pth")
    torch.save(sd, ckpt)
    model = _cnn_rnn(mta, seed=4, nm=nm, H=H, L=L)
    ds = mta.MaestroDataset(root, split="train", n_mels=nm)
    lr = mta.collect_logits_windows(model, ds, range(len(ds)), 2.0)
    assert [x[0] for x in lr] == list(range(len(ds)))
    for i, lg, roll in lr:
        t = int(ds.t_keep[i])
        _, want_roll = ds[i]
        assert lg.shape == roll.shape == (88, t) and torch.equal(roll.cpu(), want_roll)
    want_f1 = float(np.mean(E.f1_at_thresholds(lr, [0.5])[:, 0]))
    want_notes = E.note_metrics_dataset(model, ds, 0.5, window_overlap=2.0)["mean"]
    out = _run([os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--data_source", "full", "--root_dir", root, "--split", "train",
                "--model_type", "cnn_rnn", "--n_mels", str(nm), "--hidden_size", str(H), "--num_layers", str(L), "--headless",
                "--cache_dir", str(tmp_path / "none"), "--window_overlap", "2", "--note_metrics"]).stdout
    assert abs(_value(out, "EVAL_MEAN_F1") - want_f1) < 1e-6, (out, want_f1)
    assert abs(_value(out, "EVAL_NOTE_ONSET_F1") - want_notes["onset_f1"]) < 1e-6, out
    assert abs(_value(out, "EVAL_NOTE_ONSET_OFFSET_F1") - want_notes["onset_offset_f1"]) < 1e-6, out
    assert [l.split("=")[0] for l in out.strip().splitlines()] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1"]


def test_evaluate_window_overlap_past_the_recurrence_limit(mta, tmp_path):
    """18 min of 16 kHz mono: T = 33 751 frames > 32 767, what the whole-file recurrence takes at hidden_size 512."""
    from oracle import model_ref as R
    root = str(tmp_path / "long")
    _tree(root, {"long": 1080.0}, rate=SR, channels=1)
    nm, H, L = 64, 512, 1
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn", nm, H, L, seed=9), ckpt)
    base = [os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--data_source", "full", "--root_dir", root, "--split", "train",
            "--model_type", "cnn_rnn", "--n_mels", str(nm), "--hidden_size", str(H), "--num_layers", str(L), "--headless",
            "--cache_dir", str(tmp_path / "none")]
    refused = _run(base, ok=False)
    assert refused.returncode != 0 and "2004/long.wav has T=" in refused.stdout and "at most 32767" in refused.stdout, refused.stdout
    out = _run(base + ["--window_overlap", "2"]).stdout
    f1 = _value(out, "EVAL_MEAN_F1")
    assert 0.0 <= f1 <= 1.0
    model = _cnn_rnn(mta, seed=9, nm=nm, H=H, L=L)
    ds = mta.MaestroDataset(root, split="train", n_mels=nm)
    (_, lg, roll), = mta.collect_logits_windows(model, ds, [0], 2.0)
    assert lg.shape[-1] == int(ds.t_keep[0]) > 32767 and torch.isfinite(lg).all()
    from music_transcription_amd import evaluate as E
    assert abs(float(E.f1_at_thresholds([(0, lg, roll)], [0.5])[0, 0]) - f1) < 1e-6
