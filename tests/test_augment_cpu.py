"""CPU tests of the training augmentation's host side (no GPU): the interpolation table, the resampling rule's quality on the
float64 reference, the column rule that moves the labels with the audio, and the argument checks of Augment, the datasets and
the training script."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as AR  # noqa: E402
from test_rawdata_cpu import CASES, smf  # noqa: E402

SR, HOP = 16000, 512
R_MAX, R_MIN = AR.rate_of_cents(50.0), AR.rate_of_cents(-50.0)


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def test_table(mta):
    from music_transcription_amd import rawdata as RD
    tab = RD.augment_table()
    assert tab.dtype == np.float64 and tab.shape == (257, 32) and RD.AUG_BETA == AR.BETA
    for row, tap in ((0, 15), (256, 16)):
        assert np.array_equal(tab[row], np.eye(32)[tap])
        assert np.array_equal(tab.astype(np.float32)[row], np.eye(32, dtype=np.float32)[tap])
    assert np.abs(tab.sum(axis=1) - 1.0).max() <= 1e-12
    assert np.abs(tab - AR.table()).max() <= 1e-15             # the package's builder against the reference's, written apart
    # the rows meet the impulses: the table is continuous in the phase (what the blend of neighbouring rows relies on)
    assert np.abs(tab[1] - tab[0]).max() < 0.02 and np.abs(tab[256] - tab[255]).max() < 0.02


# SNR of the float64 reference against the analytic sine at r * f, 8192 outputs, table held as float32 (beta = 10):
# 1 kHz 132.0 dB, 6 kHz 100.9 dB at both +50 and -50 cents.  The test asserts that figure minus 6 dB.
MEASURED_SNR_DB = {1000.0: 132.0, 6000.0: 100.9}


@pytest.mark.parametrize("freq", [1000.0, 6000.0])
@pytest.mark.parametrize("rate", [R_MAX, R_MIN])
def test_resampler_quality_on_sines(freq, rate):
    n, tab = 8192, AR.table_f32()
    w = 2.0 * np.pi * freq / SR
    y = AR.resample(lambda idx: np.sin(w * idx), n, rate, tab)
    ref = np.sin(w * (np.arange(n, dtype=np.float64) * rate / 2.0 ** 32))
    snr = 10.0 * np.log10(np.sum(ref ** 2) / np.sum((y - ref) ** 2))
    print(f"freq {freq} rate {rate / 2 ** 32:.6f}: SNR {snr:.2f} dB")
    assert snr >= MEASURED_SNR_DB[freq] - 6.0, snr


def _brute_roll(spans, pitch_off, cols, t_keep):
    """Frame n is on iff a span intersects source frames [cols[n], max(cols[n + 1], cols[n] + 1)); the last column stays 0."""
    out = np.zeros((88, t_keep), np.float32)
    for p in range(88):
        for n in range(min(t_keep, len(cols) - 1)):
            s, e = int(cols[n]), max(int(cols[n + 1]), int(cols[n]) + 1)
            for u, v in spans[pitch_off[p]:pitch_off[p + 1]]:
                if u < e and v > s:
                    out[p, n] = 1.0
                    break
    return out


@pytest.mark.parametrize("rate", [1 << 32, R_MIN, R_MAX])
def test_labels_follow_the_speed(mta, rate):
    from music_transcription_amd import midi as MD, preprocess as P, rawdata as RD
    fs = SR / HOP
    for name in ("pedal_edges", "on_frame_edges", "random"):
        m = MD.MidiFile(smf(CASES[name]))
        spans, poff, _, _ = RD.label_spans(m, fs)
        for c in P.build_chunk_index([m.get_end_time() + 3.0], 2.3, 0.25, SR):
            cols = RD.augmented_cols(c["start_time"], c["end_time"], fs, rate)
            assert np.array_equal(cols, AR.cols_aug(c["start_time"], c["end_time"], fs, rate))
            if rate == 1 << 32:
                assert np.array_equal(cols, RD.column_grid(c["start_time"], c["end_time"], fs))
            else:                                                # columns start where the window starts and run at the speed
                assert cols[0] == RD.column_grid(c["start_time"], c["end_time"], fs)[0]
                span = (c["end_time"] - c["start_time"]) * fs * rate / 2.0 ** 32
                assert abs((cols[-1] - cols[0]) - span) <= 1.0
            t = len(cols)
            assert np.array_equal(RD.roll_from_spans(spans, poff, t, cols), _brute_roll(spans, poff, cols, t)), (name, c)


def test_augment_argument_checks(mta):
    import torch
    a = mta.Augment()
    assert a.pitch_cents == 10.0 and a.snr_db is None and isinstance(a.generator, torch.Generator)
    assert mta.Augment(0.0, (20, 40)).snr_db == (20.0, 40.0) and mta.Augment(50.0).pitch_cents == 50.0
    for bad in (-1.0, 50.5, float("nan")):
        with pytest.raises(ValueError, match="pitch_cents"):
            mta.Augment(pitch_cents=bad)
    for bad in ((-1.0, 10.0), (30.0, 20.0), (float("nan"), 3.0), 20.0, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="snr_db"):
            mta.Augment(snr_db=bad)


def test_augment_draws(mta):
    import torch
    g = torch.Generator().manual_seed(11)
    a = mta.Augment(pitch_cents=50.0, snr_db=(20.0, 40.0), generator=g)
    rate, snr, seed = a.draw(1000)
    assert rate.dtype == np.uint64 and rate.shape == snr.shape == (1000,) and 0 <= seed < 1 << 31
    assert R_MIN <= rate.min() < (1 << 32) - (1 << 26) and (1 << 32) + (1 << 26) < rate.max() <= R_MAX
    assert 20.0 <= snr.min() < 22.0 and 38.0 < snr.max() <= 40.0
    rate2, snr2, seed2 = mta.Augment(50.0, (20.0, 40.0), torch.Generator().manual_seed(11)).draw(1000)
    assert np.array_equal(rate, rate2) and np.array_equal(snr, snr2) and seed == seed2
    rate0, snr0, _ = mta.Augment(pitch_cents=0.0).draw(7)
    assert np.all(rate0 == 1 << 32) and np.all(np.isnan(snr0))


def test_whole_files_refuse_augmentation(mta, tmp_path):
    # refused in the constructor before anything is read: no tree and no GPU needed
    with pytest.raises(ValueError, match="chunk_length"):
        mta.MaestroDataset(str(tmp_path / "absent"), augment=mta.Augment())
    with pytest.raises(TypeError, match="Augment"):
        mta.MaestroDataset(str(tmp_path / "absent"), chunk_length=30.0, augment={"pitch_cents": 10})


def test_hybrid_dataset_never_augments_from_the_cache(mta, tmp_path, monkeypatch, capsys):
    from music_transcription_amd import rawdata as RD
    from test_rawdata_cpu import _write_meta
    made = []

    class Fake:
        def __init__(self, **kw):
            made.append(kw)
    monkeypatch.setattr(RD, "MaestroDataset", Fake)
    cache = str(tmp_path / "cache")
    _write_meta(cache, 30.0, 0.0)
    aug = mta.Augment()
    h = mta.HybridMaestroDataset("root", cache, "train", chunk_length=30.0, overlap=0.0, augment=aug)
    assert not h.use_cache and made[-1]["augment"] is aug and "Using raw dataset" in capsys.readouterr().out
    h = mta.HybridMaestroDataset("root", cache, "train", chunk_length=30.0, overlap=0.0)
    assert h.use_cache and len(made) == 1


def _train(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py")] + args, capture_output=True, text=True, timeout=120)


def test_train_script_flags_and_refusals(tmp_path):
    r = _train(["--help"])
    assert r.returncode == 0 and "--augment_pitch_cents" in r.stdout and "--augment_snr_db" in r.stdout
    none = ["--cached_dir", str(tmp_path / "none"), "--root_dir", str(tmp_path), "--chunk_length", "30"]
    r = _train(none + ["--augment_pitch_cents", "10"])             # no recordings to read: refused before the GPU is touched
    assert r.returncode != 0 and "--augment_*" in r.stderr and "--root_dir" in r.stderr
    r = _train(none + ["--augment_pitch_cents", "60"])
    assert r.returncode != 0 and "--augment_pitch_cents" in r.stderr
    r = _train(none + ["--augment_snr_db", "30", "20"])
    assert r.returncode != 0 and "--augment_snr_db" in r.stderr
    r = _train(["--cached_dir", str(tmp_path / "none"), "--root_dir", str(tmp_path), "--augment_snr_db", "20", "40"])
    assert r.returncode != 0 and "--chunk_length" in r.stderr      # full-file training stays refused
