"""CPU tests of the cache-free data path (music_transcription_amd/rawdata.py): the per-recording label span tables, rendered
by the host copy of mt_roll_windows' rule, equal midi.chunk_roll / the full-file roll exactly; HybridMaestroDataset's
cache-or-raw choice; the new script flags."""
import os
import pickle
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


# ------------------------------------------------------------------ a small SMF writer
def _vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append(0x80 | (n & 0x7F))
        n >>= 7
    return bytes(reversed(out))


def smf(tracks, resolution=1000, tempo_us=500000):
    """tracks: lists of (tick, status, data1, data2); track 0 gets the tempo.  Format 1."""
    chunks = []
    for i, evs in enumerate(tracks):
        body, last = b"", 0
        if i == 0:
            body += _vlq(0) + b"\xff\x51\x03" + tempo_us.to_bytes(3, "big")
        for tick, st, d1, d2 in sorted(evs, key=lambda e: e[0]):
            body += _vlq(tick - last) + bytes([st, d1]) + (bytes([d2]) if d2 is not None else b"")
            last = tick
        body += _vlq(0) + b"\xff\x2f\x00"
        chunks.append(b"MTrk" + struct.pack(">I", len(body)) + body)
    return b"MThd" + struct.pack(">IHHH", 6, 1, len(chunks), resolution) + b"".join(chunks)


def note(ch, pitch, t0, t1, vel=80):
    return [(t0, 0x90 | ch, pitch, vel), (t1, 0x80 | ch, pitch, 0)]


def cc64(ch, tick, value):
    return [(tick, 0xB0 | ch, 64, value)]


def _cases():
    # 120 bpm, 1000 ticks per beat: one tick = 0.5 ms; a frame at 16 kHz / 512 is 32 ms = 64 ticks
    c = {}
    c["overlap_same_pitch"] = [[]] + [note(0, 60, 100, 3000) + note(0, 60, 1500, 5000) + note(0, 62, 2000, 2000 + 64 * 7)]
    ped = note(0, 64, 200, 900) + note(0, 67, 5000, 5200) + note(0, 69, 12000, 12100) + note(0, 71, 13000, 14000)
    ped += cc64(0, 100, 63) + cc64(0, 300, 64) + cc64(0, 2000, 127) + cc64(0, 4000, 20) + cc64(0, 4900, 127) + cc64(0, 8000, 0)
    ped += cc64(0, 11000, 100)                                       # pedal still down at the end of the file
    c["pedal_edges"] = [[], ped]
    t1 = note(0, 50, 0, 640) + note(0, 52, 3000, 3300) + cc64(0, 500, 90) + cc64(0, 6000, 10)
    t2 = note(1, 50, 1000, 1100) + note(1, 55, 4000, 4100) + cc64(1, 3900, 127) + cc64(1, 9000, 0)
    drums = note(9, 36, 0, 20000) + note(9, 40, 500, 700)
    c["two_tracks_and_drums"] = [[], t1, t2, drums]
    c["outside_range"] = [[], note(0, 10, 0, 2000) + note(0, 120, 100, 3000) + note(0, 21, 200, 400) + note(0, 108, 500, 900)]
    c["zero_length"] = [[], note(0, 60, 640, 640) + note(0, 61, 1000, 1010) + note(0, 62, 2000, 4000) + cc64(0, 600, 127) + cc64(0, 700, 0)]
    c["on_frame_edges"] = [[], sum((note(0, 40 + k, 64 * k, 64 * (k + 3)) for k in range(30)), [])]
    rng = np.random.default_rng(3)
    ev = []
    for _ in range(300):
        p, t0 = int(rng.integers(15, 115)), int(rng.integers(0, 60000))
        ev += note(0, p, t0, t0 + int(rng.integers(0, 3000)), int(rng.integers(1, 128)))
    for k in range(20):
        ev += cc64(0, 3000 * k + int(rng.integers(0, 500)), int(rng.integers(0, 128)))
    c["random"] = [[], ev]
    c["empty"] = [[]]
    return c


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("chunk,overlap", [(2.0, 0.0), (1.3, 0.25), (3.0, 0.25)])
def test_span_tables_reproduce_chunk_roll(mta, name, chunk, overlap):
    from music_transcription_amd import midi as MD, rawdata as RD, preprocess as P
    sr, hop = 16000, 512
    fs = sr / hop
    m = MD.MidiFile(smf(CASES[name]))
    spans, poff, width, has_notes = RD.label_spans(m, fs)
    assert np.all(spans[:, 0] < spans[:, 1]) and poff[0] == 0 and poff[-1] == len(spans)
    for p in range(88):                                          # sorted and disjoint per pitch
        sp = spans[poff[p]:poff[p + 1]]
        assert np.all(sp[1:, 0] > sp[:-1, 1])
    full = m.get_piano_roll(fs=fs)[21:109] > 0
    assert width == full.shape[1]
    assert np.array_equal(RD.roll_from_spans(spans, poff, width, None), full.astype(np.float32))
    # chunks over a duration reaching past the MIDI end
    dur = m.get_end_time() + 7.0
    for c in P.build_chunk_index([dur], chunk, overlap, sr):
        want = MD.chunk_roll(m, c["start_time"], c["end_time"], sr, hop)
        cols = RD.column_grid(c["start_time"], c["end_time"], fs)
        t = len(cols) if has_notes else 0
        assert want.shape == (88, t), (want.shape, t)
        got = RD.roll_from_spans(spans, poff, t, cols)
        assert np.array_equal(got, want), (name, c, np.argwhere(got != want)[:5])


def test_cases_exercise_the_edges(mta):
    from music_transcription_amd import midi as MD, rawdata as RD
    fs = 16000 / 512
    m = MD.MidiFile(smf(CASES["pedal_edges"]))
    spans, poff, _, _ = RD.label_spans(m, fs)
    r = 64 - 21
    assert len(spans[poff[r]:poff[r + 1]]) == 1 and spans[poff[r]][1] > int(m.instruments[0].notes[0].end * fs)   # sustained by CC 64 >= 64
    t = 71 - 21                                                  # pedal down at the end of the file: the last note is not extended
    sp = spans[poff[t]:poff[t + 1]]
    n = [x for x in m.instruments[0].notes if x.pitch == 71][0]
    assert sp.tolist() == [[int(n.start * fs), int(n.end * fs)]]
    m2 = MD.MidiFile(smf(CASES["two_tracks_and_drums"]))
    assert sum(i.is_drum for i in m2.instruments) == 1 and len(m2.instruments) == 3
    s2, p2, w2, _ = RD.label_spans(m2, fs)
    assert w2 == int(fs * m2.get_end_time())                      # the drum track sets the full-file width
    assert p2[36 - 21] == p2[36 - 21 + 1]                         # drums contribute nothing


def _write_meta(path, chunk_length, overlap):
    os.makedirs(os.path.join(path, "train"), exist_ok=True)
    with open(os.path.join(path, "train_metadata.pkl"), "wb") as f:
        pickle.dump({"chunk_length": chunk_length, "overlap": overlap, "num_chunks": 0, "chunks": []}, f)


def test_hybrid_dataset_choice(mta, tmp_path, monkeypatch, capsys):
    from music_transcription_amd import rawdata as RD
    made = []

    class Fake:
        def __init__(self, **kw):
            made.append(kw)

        def __len__(self):
            return 5
    monkeypatch.setattr(RD, "MaestroDataset", Fake)
    cache = str(tmp_path / "cache")
    _write_meta(cache, 30.0, 0.0)
    h = mta.HybridMaestroDataset("root", cache, "train", chunk_length=30.0, overlap=0.0)
    assert h.use_cache and not made and "Using cached dataset" in capsys.readouterr().out
    for cl, ov in ((30.0, 0.25), (20.0, 0.0), (None, 0.0)):
        h = mta.HybridMaestroDataset("root", cache, "train", chunk_length=cl, overlap=ov, n_mels=64)
        assert not h.use_cache and made[-1]["chunk_length"] == cl and made[-1]["overlap"] == ov and made[-1]["n_mels"] == 64
        assert "Using raw dataset" in capsys.readouterr().out and len(h) == 5
    h = mta.HybridMaestroDataset("root", str(tmp_path / "missing"), "train", chunk_length=30.0)
    assert not h.use_cache and len(made) == 4


def test_maestro_dataset_refuses_waveforms_and_workers(mta, monkeypatch):
    from music_transcription_amd import rawdata as RD
    with pytest.raises(NotImplementedError):
        mta.MaestroDataset("root", return_waveform=True)
    ds = RD.MaestroDataset.__new__(RD.MaestroDataset)
    monkeypatch.setattr(RD, "_in_worker", lambda: True)
    with pytest.raises(RuntimeError, match="DeviceBatchLoader"):
        ds[0]
    with pytest.raises(RuntimeError, match="num_workers=0"):
        ds.get_batch([0])


def test_device_batch_loader_matches_dataloader_order(mta):
    import torch
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler

    class Idx(torch.utils.data.Dataset):
        def __len__(self):
            return 23

        def __getitem__(self, i):
            return i

        def get_batch(self, idx):
            return list(idx)
    ds = Idx()
    for kw in (dict(shuffle=True), dict(shuffle=False), dict(shuffle=True, drop_last=True)):
        torch.manual_seed(5)
        a = [b.tolist() for b in DataLoader(ds, batch_size=4, **kw)] + [b.tolist() for b in DataLoader(ds, batch_size=4, **kw)]
        after_a = torch.rand(1)
        torch.manual_seed(5)
        b = list(mta.DeviceBatchLoader(ds, 4, **kw)) + list(mta.DeviceBatchLoader(ds, 4, **kw))
        assert a == b and torch.equal(after_a, torch.rand(1))
    s = DistributedSampler(ds, num_replicas=2, rank=1, shuffle=True, seed=3, drop_last=True)
    s.set_epoch(2)
    assert [b.tolist() for b in DataLoader(ds, batch_size=3, sampler=s)] == list(mta.DeviceBatchLoader(ds, 3, sampler=s))
    assert len(mta.DeviceBatchLoader(ds, 4, drop_last=True)) == 5


@pytest.mark.parametrize("script,flags", [("train_cnn.py", ("--root_dir", "--year", "--chunk_length", "--chunk_overlap")),
                                          ("evaluate.py", ("--root_dir", "--year", "--data_source"))])
def test_script_help_lists_new_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert f in r.stdout


def test_train_refuses_full_file_training_before_starting(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--cached_dir", str(tmp_path / "none"),
                        "--root_dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--chunk_length" in r.stderr
