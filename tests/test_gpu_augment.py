"""GPU tests of the training augmentation: mt_augment_windows against the float64 reference (tests/augment_ref.py), and
MaestroDataset(augment=...) against its own kernels, its labels and the training script.

One store and one set of windows serve the kernel tests: a window at a recording's first sample, one at an odd offset, one of
odd length, one running past its recording's end, one with nothing of its recording left, and one a sample longer than a tile
of 2048 outputs (rows of four tiles, so more than one workgroup per row and the zero padding of every row are covered)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as AR  # noqa: E402
from test_rawdata_cpu import cc64, note, smf  # noqa: E402

pytestmark = pytest.mark.gpu
SR, HOP, TILE = 16000, 512, 2048
ONE = 1 << 32
R_MAX, R_MIN = AR.rate_of_cents(50.0), AR.rate_of_cents(-50.0)
# (win_off, win_len, before, after)
WINS = [(0, 5000, 0, 60000), (70001, 6000, 10001, 50000), (130000, 4003, 500, 20000), (150000, 8000, 100, 5000),
        (170000, 3000, 200, -5), (180000, TILE + 1, 7, 15000)]
L_MAX = 8000


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


@pytest.fixture(scope="module")
def store():
    g = torch.Generator().manual_seed(5)
    host = (torch.randn(200_003, generator=g) * 0.2).numpy()
    return host, torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def tab32(mta):
    from music_transcription_amd import rawdata as RD
    t = RD.augment_table().astype(np.float32)
    return t.astype(np.float64), torch.from_numpy(t).cuda()


def _augment(store_dev, tab_dev, wins, rates, noise_rel=None, seed=0, l_max=L_MAX):
    """One mt_augment_windows launch: (out (B, l_max), the workspace of per-tile partial sums of squares or None)."""
    from music_transcription_amd import _lib
    B, dev = len(wins), store_dev.device
    d64 = torch.tensor([[w[0] for w in wins], [int(np.uint64(r).view(np.int64)) for r in rates]], dtype=torch.int64, device=dev)
    d32 = torch.tensor([[w[1] for w in wins], [w[2] for w in wins], [w[3] for w in wins]], dtype=torch.int32, device=dev)
    out = torch.full((B, l_max), float("nan"), device=dev)
    ws, nrel = None, None
    if noise_rel is not None:
        nrel = torch.tensor(noise_rel, dtype=torch.float32, device=dev)
        ws = torch.full((int(_lib.lib.mt_augment_ws_bytes(B, l_max)) // 4,), float("nan"), device=dev)
        assert ws.numel() == B * -(-l_max // TILE)
    _lib.check(_lib.lib.mt_augment_windows(_lib.ptr(store_dev), _lib.ptr(d64[0]), _lib.ptr(d32[0]), _lib.ptr(d32[1]), _lib.ptr(d32[2]),
                                           _lib.ptr(d64[1]), int(min(rates)), int(max(rates)), _lib.ptr(nrel), seed, _lib.ptr(tab_dev), B,
                                           l_max, _lib.ptr(out), _lib.ptr(ws), 0 if ws is None else ws.numel() * 4, _lib.stream_ptr()),
               "mt_augment_windows")
    return out, ws


def _reference(store_host, tab, win, rate):
    off, n, before, after = win
    return AR.resample(AR.window_reader(store_host, off, before, after), n, rate, tab)


def test_identity_copies_the_windows(mta, store, tab32):
    host, dev = store
    out, _ = _augment(dev, tab32[1], WINS, [ONE] * len(WINS))
    for b, (off, n, before, after) in enumerate(WINS):
        want = torch.zeros(L_MAX, device=dev.device)
        k = max(0, min(after, n))
        want[:k] = dev[off:off + k]
        assert torch.equal(out[b], want), b


def test_bad_arguments_are_refused(mta, store, tab32):
    from music_transcription_amd import _lib
    host, dev = store
    with pytest.raises(_lib.MtError, match="0.03"):
        _augment(dev, tab32[1], WINS[:1], [int(1.031 * ONE)])
    with pytest.raises(_lib.MtError, match="multiple of 4"):
        _augment(dev, tab32[1], WINS[:1], [ONE], l_max=5002)


# |out - ref| <= 2e-5 * max|x|: 32 f32 products and sums with sum|c| <= 2 give about 4e-6 * max|x|, a margin of 5
@pytest.mark.parametrize("rate", [ONE + 1, R_MAX, R_MIN, ONE - 1], ids=["one_plus_ulp", "plus50c", "minus50c", "phase255_mu1"])
def test_resampling_against_float64(mta, store, tab32, rate):
    host, dev = store
    if rate == ONE - 1:                                          # output 1 sits at frac = 2^32 - 1: ph = 255, mu = 1 - 2^-24
        k, ph, mu = AR.positions(4, rate)
        assert ph[1] == 255 and mu[1] == 1.0 - 2.0 ** -24
    out, _ = _augment(dev, tab32[1], WINS, [rate] * len(WINS))
    got = out.cpu().numpy().astype(np.float64)
    bound = 2e-5 * float(np.abs(host).max())
    for b, w in enumerate(WINS):
        ref = _reference(host, tab32[0], w, rate)
        err = float(np.abs(got[b, :w[1]] - ref).max())
        print(f"rate {rate / ONE:.9f} window {b}: max|out - ref| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (b, err)
        assert np.all(got[b, w[1]:] == 0.0), b                   # the padding past win_len is exactly 0


def test_noise(mta, store, tab32):
    host, dev = store
    # the shared windows and a silent one: its recording ends 100 samples before it, out of the taps' reach (the shared window
    # with after = -5 still hears the recording's last samples through the filter's leading taps, so it is quiet, not silent)
    wins = WINS + [(175000, 2500, 50, -100)]
    rates = [R_MAX, R_MIN, ONE, ONE + 12345678, R_MAX, R_MIN, R_MAX]
    # SNRs of 10..20 dB: sigma >= 0.1 * rms keeps the f32 rounding of y + noise (half an ulp of |out| < 2) under 1e-5 sigma
    nrel = [10.0 ** (-10.0 / 20), 10.0 ** (-20.0 / 20), 0.0, 10.0 ** (-15.0 / 20), 10.0 ** (-10.0 / 20), 10.0 ** (-12.0 / 20), 10.0 ** (-10.0 / 20)]
    clean, _ = _augment(dev, tab32[1], wins, rates)
    noisy, ws = _augment(dev, tab32[1], wins, rates, nrel, seed=1234567)
    again, _ = _augment(dev, tab32[1], wins, rates, nrel, seed=1234567)
    other, _ = _augment(dev, tab32[1], wins, rates, nrel, seed=1234568)
    assert torch.equal(noisy, again)
    assert not torch.equal(noisy, other)
    tiles = -(-L_MAX // TILE)
    part = ws.cpu().numpy().astype(np.float64).reshape(len(wins), tiles)
    c, nz = clean.cpu().numpy().astype(np.float64), noisy.cpu().numpy().astype(np.float64)
    silent = 0
    for b, w in enumerate(wins):
        n = w[1]
        ref = _reference(host, tab32[0], w, rates[b])
        ms_ref = AR.mean_square(ref)
        ms = part[b, :-(-n // TILE)].sum() / n
        assert np.all(nz[b, n:] == 0.0)
        if ms_ref == 0.0:                                        # nothing of the recording left: a silent window stays silent
            assert ms == 0.0 and np.all(nz[b] == 0.0), b
            silent += 1
            continue
        assert abs(ms - ms_ref) <= 1e-5 * ms_ref, (b, ms, ms_ref)
        if nrel[b] == 0.0:
            assert np.array_equal(nz[b], c[b]), b
            continue
        sigma = np.sqrt(ms_ref) * nrel[b]
        g = (nz[b, :n] - c[b, :n]) / sigma
        err = float(np.abs(g - AR.gauss(1234567, b, n)).max())
        print(f"window {b}: mean square {ms:.9e} (ref {ms_ref:.9e}), max|g - g_ref| = {err:.3e}")
        assert err <= 1e-4, (b, err)
    assert silent == 1
    allg = AR.gauss(1234567, 1, 6000)
    assert abs(allg.mean()) < 0.05 and abs(allg.std() - 1.0) < 0.05   # the reference's g is a unit normal


# ------------------------------------------------------------------ through the dataset
def _write_tree(root, recs):
    """recs: name -> (split, seconds, signal(t) -> float array, MIDI events): 44.1 kHz stereo wav + MIDI + csv."""
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "2004"), exist_ok=True)
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for name, (split, d, sig, ev) in recs.items():
        t = np.arange(int(d * 44100)) / 44100.0
        s = sig(t)
        wavfile.write(os.path.join(root, "2004", f"{name}.wav"), 44100, (np.stack([s, s], 1) * 32767).astype(np.int16))
        with open(os.path.join(root, "2004", f"{name}.midi"), "wb") as fh:
            fh.write(smf([[], ev]))
        rows.append(f"X,Y,{split},2004,2004/{name}.midi,2004/{name}.wav,{d}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("maestro_aug"))
    rng = np.random.default_rng(0)
    recs = {}
    for i, (name, split, d) in enumerate((("a", "train", 9.3), ("b", "train", 6.1), ("v", "validation", 4.5))):
        ev = []
        for k, s in enumerate(np.arange(0.0, d - 0.6, 0.35)):    # 2000 ticks per second
            ev += note(0, 40 + (k * 7) % 50, int(s * 2000), int((s + 0.3 + 0.2 * (k % 3)) * 2000))
        ev += cc64(0, 3000, 100) + cc64(0, 7000, 0)
        noise = 0.02 * rng.standard_normal(int(d * 44100))
        recs[name] = (split, d, lambda t, f=220.0 * (i + 1), nz=noise: 0.3 * np.sin(2 * np.pi * f * t) * np.exp(-0.5 * (t % 1.7)) + nz, ev)
    _write_tree(root, recs)
    return root


CHUNK = 4.0                                                      # a: 2 chunks (1.3 s dropped), b: 4 s + 2.1 s, v: 1 chunk


@pytest.fixture(scope="module")
def plain(mta, tree):
    return mta.MaestroDataset(tree, split="train", n_mels=64, chunk_length=CHUNK)


def test_dataset_identity_equals_plain_batches(mta, tree, plain):
    aug = mta.MaestroDataset(tree, split="train", n_mels=64, chunk_length=CHUNK, augment=mta.Augment(pitch_cents=0.0, snr_db=None))
    assert len(plain) == len(aug) == 4
    for idx in ([3, 0, 2, 1], [2], [1, 3]):
        a, p = aug.get_batch(idx), plain.get_batch(idx)
        assert torch.equal(a[0], p[0]) and torch.equal(a[1], p[1]) and torch.equal(a[2], p[2]), idx
        assert np.all(aug.last_augment["rate_q32"] == ONE) and np.all(np.isnan(aug.last_augment["snr_db"]))
    assert plain.last_augment is None


@pytest.mark.parametrize("onset_labels", ["roll", "midi"])
def test_batch_is_the_composition_of_the_kernels(mta, tree, tab32, onset_labels):
    from music_transcription_amd import _lib
    ds = mta.MaestroDataset(tree, split="train", n_mels=64, chunk_length=CHUNK, onset_labels=onset_labels,
                            augment=mta.Augment(pitch_cents=50.0, snr_db=(10.0, 30.0), generator=torch.Generator().manual_seed(9)))
    idx = [3, 0, 2, 1]
    mel, labels, lengths = ds.get_batch(idx)
    la = ds.last_augment
    assert set(la) == {"rate_q32", "snr_db", "seed"} and la["rate_q32"].dtype == np.uint64 and len(set(la["rate_q32"].tolist())) == 4
    assert np.all((la["snr_db"] >= 10.0) & (la["snr_db"] <= 30.0)) and 0 <= int(la["seed"]) < 1 << 31
    dev, B = ds.device, len(idx)
    wins = [(ds.store.loc[int(ds.rec[i])] + int(ds.start[i]), int(ds.win_len[i]), int(ds.start[i]),
             ds.store.n[int(ds.rec[i])] - int(ds.start[i])) for i in idx]
    l_max = -(-max(w[1] for w in wins) // 4) * 4
    wave, _ = _augment(ds.store.buf, tab32[1], wins, la["rate_q32"].tolist(), (10.0 ** (-la["snr_db"] / 20.0)).astype(np.float32).tolist(),
                       seed=int(la["seed"]), l_max=l_max)
    t_keep = [int(ds.t_keep[i]) for i in idx]
    T_out = max(t_keep)
    assert lengths.tolist() == t_keep
    d64 = torch.arange(B, dtype=torch.int64, device=dev) * l_max
    d32 = torch.tensor([[w[1] for w in wins], t_keep], dtype=torch.int32, device=dev)
    want = torch.full((B, 1, 64, T_out), float("nan"), device=dev)
    cmax = torch.empty(B, device=dev)
    _lib.check(_lib.lib.mt_mel_db_windows_f32(_lib.ptr(ds.fe.plan), ds.fe.desc, _lib.ptr(wave.reshape(-1)), _lib.ptr(d64), _lib.ptr(d32[0]),
                                              _lib.ptr(d32[0]), B, max(w[1] for w in wins), T_out, _lib.ptr(d32[1]), _lib.ptr(want),
                                              _lib.ptr(cmax), _lib.stream_ptr()))
    assert torch.equal(mel, want)
    fs = SR / HOP
    grids = [AR.cols_aug(ds.chunks[i]["start_time"], ds.chunks[i]["end_time"], fs, int(r)) for i, r in zip(idx, la["rate_q32"])]
    ncols = [len(g) for g in grids]
    dcols = torch.from_numpy(np.concatenate(grids).astype(np.int32)).to(dev)
    dco = torch.tensor(np.concatenate([[0], np.cumsum(ncols)[:-1]]), dtype=torch.int64, device=dev)
    drec = torch.tensor([[int(ds.rec[i]) for i in idx], ncols], dtype=torch.int32, device=dev)
    tables = [("frame", ds.spans, ds.pitch_off)] + ([("onset", ds.onset_spans, ds.onset_pitch_off)] if onset_labels == "midi" else [])
    for key, spans, poff in tables:
        roll = torch.full((B, 88, T_out), float("nan"), device=dev)
        _lib.check(_lib.lib.mt_roll_windows(_lib.ptr(spans), _lib.ptr(poff), _lib.ptr(dcols), _lib.ptr(drec[0]), _lib.ptr(dco), _lib.ptr(drec[1]),
                                            _lib.ptr(d32[1]), B, T_out, _lib.ptr(roll), _lib.stream_ptr()))
        got = labels[key] if onset_labels == "midi" else labels
        assert torch.equal(got, roll) and float(roll.sum()) > 0, key


def _fixed_rate(mta, rate):
    """The fixed-draw hook: an Augment whose draw() returns one given speed and no noise."""
    class Fixed(mta.Augment):
        def draw(self, n):
            return np.full(n, rate, np.uint64), np.full(n, np.nan), 5
    return Fixed(pitch_cents=50.0)


def _edges(row):
    on = np.flatnonzero(row > 0)
    assert len(on) and np.all(np.diff(on) == 1), on               # one run
    return int(on[0]), int(on[-1]) + 1


def test_audio_and_labels_move_together(mta, tmp_path):
    """One recording, silent but for two tones, 1.0-2.0 s (chunk 0) and 4.2-5.1 s (chunk 1, 1.2-2.1 s into it), each with its
    MIDI note.  At the highest speed both edges of label and audio come earlier than at the lowest, and the mel's rise stays
    within a frame of the label's: r against 1 / r, or a column rule anchored at 0 instead of the window start, fails.

    The mel's rise is its first frame within 14 dB of the loudest.  A frame is centred on sample 512 n and a label column is on
    from the frame that holds the onset, so the threshold sits where a frame centred half a frame before the onset would be:
    on the float64 reference with the oracle's mel, the first frame counted lies 4.6 to 9.2 dB under the peak and the one
    before it 19.7 to 37.4 dB under, in all six cases.  An edge at 1 s moves by 0.9 frames at 50 cents, so against the plain
    batch the rise may stay on its frame; the fall (1.8 frames) and the two extremes against each other may not."""
    from music_transcription_amd import midi as MD, rawdata as RD
    root = str(tmp_path / "tone")
    tones = ((1.0, 2.0, 69, 440.0), (4.2, 5.1, 76, 659.26))
    sig = lambda t: sum(0.5 * np.sin(2 * np.pi * f * t) * ((t >= a) & (t < b)) for a, b, _, f in tones)
    ev = sum((note(0, p, int(a * 2000), int(b * 2000)) for a, b, p, _ in tones), [])
    _write_tree(root, {"tone": ("train", 6.0, sig, ev)})
    fs = SR / HOP
    spans, poff, _, _ = RD.label_spans(MD.MidiFile(os.path.join(root, "2004", "tone.midi")), fs)
    seen = {}
    for rate in (ONE, R_MAX, R_MIN):
        ds = mta.MaestroDataset(root, split="train", n_mels=64, chunk_length=3.0, augment=None if rate == ONE else _fixed_rate(mta, rate))
        assert len(ds) == 2
        mel, roll, lengths = ds.get_batch([0, 1])
        if rate != ONE:
            assert np.all(ds.last_augment["rate_q32"] == rate)
        mel, roll = mel.cpu().numpy(), roll.cpu().numpy()
        for b, (_, _, pitch, _) in enumerate(tones):
            t = int(lengths[b])
            cols = AR.cols_aug(ds.chunks[b]["start_time"], ds.chunks[b]["end_time"], fs, rate)
            want = RD.roll_from_spans(spans, poff, t, cols)
            assert np.array_equal(roll[b, :, :t], want), (rate, b)
            rise, fall = _edges(roll[b, pitch - 21, :t])
            assert (rise, fall) == _edges(want[pitch - 21])
            energy = mel[b, 0, :, :t].max(axis=0)                # dB; silence sits at the clamp, 80 dB under the tone
            loud = np.flatnonzero(energy >= energy.max() - 14.0)
            print(f"rate {rate / ONE:.6f} chunk {b}: label [{rise}, {fall}), mel within 14 dB of its peak [{loud[0]}, {loud[-1] + 1})")
            assert abs(int(loud[0]) - rise) <= 1, (rate, b, int(loud[0]), rise)
            seen[rate, b] = (rise, fall)
    for b in range(2):
        assert seen[R_MAX, b][0] <= seen[ONE, b][0] <= seen[R_MIN, b][0] and seen[R_MAX, b][0] < seen[R_MIN, b][0], seen
        assert seen[R_MAX, b][1] < seen[ONE, b][1] < seen[R_MIN, b][1], seen


def test_train_script_with_augmentation(mta, tree, tmp_path):
    from music_transcription_amd import preprocess as P
    cache = str(tmp_path / "cache")
    for split in ("train", "validation"):
        P.preprocess_and_cache(tree, cache, CHUNK, 0.0, 64, SR, HOP, split)
    common = [sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--epochs", "1", "--batch_size", "2", "--n_mels", "64",
              "--model", "cnn_rnn", "--hidden_size", "32", "--num_layers", "2", "--seed", "3", "--num_workers", "0", "--save_every", "1",
              "--root_dir", tree, "--augment_pitch_cents", "10", "--augment_snr_db", "20", "40"]
    for tag, extra in (("none", ["--cached_dir", str(tmp_path / "none"), "--chunk_length", str(CHUNK)]), ("cache", ["--cached_dir", cache])):
        run_dir = tmp_path / f"run_{tag}"
        r = subprocess.run(common + extra + ["--run_dir", str(run_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        assert "Data source: raw recordings" in r.stdout and "Augmentation (training set)" in r.stdout, r.stdout
        if tag == "cache":
            assert "the cache matches" in r.stdout
        hist = json.load(open(run_dir / "history.json"))
        assert len(hist) == 1 and hist[0]["steps"] == 2
        assert np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"]), hist
