"""GPU tests of the sub-frame onsets (csrc/onset_regress.hip; DESIGN.md 6c "Sub-frame onsets"): mt_onset_regress_windows bit for bit
against the integer reference, mt_refine_onsets within one tick of the float64 reference, the round trip target -> logit -> decoder ->
refinement on the device, the dataset options and the scripts.  Every test prints the figure it is about to assert (`-s`)."""
import importlib.util
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
import onset_regress_ref as OR  # noqa: E402
from test_onset_regress_cpu import _tables  # noqa: E402
from test_rawdata_cpu import note, smf  # noqa: E402

pytestmark = pytest.mark.gpu
ONE = 1 << 32
RATE_LO, RATE_HI = ONE - int(0.03 * ONE), ONE + int(0.03 * ONE)


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _target(on_tick, tick_off, win_rec, start, t_keep, T_out, J, rate=None):
    from music_transcription_amd import _lib
    B = len(win_rec)
    d = [_dev(on_tick if len(on_tick) else np.zeros(1), np.int32), _dev(tick_off, np.int64), _dev(win_rec, np.int32), _dev(start, np.int32),
         None if rate is None else _dev(np.array(rate, np.uint64).view(np.int64), np.int64), _dev(t_keep, np.int32)]
    out = torch.full((B, 88, T_out), float("nan"), device="cuda")
    _lib.check(_lib.lib.mt_onset_regress_windows(*[_lib.ptr(t) for t in d], B, T_out, J, _lib.ptr(out), _lib.stream_ptr()), "mt_onset_regress_windows")
    return out.cpu().numpy()


# ------------------------------------------------------------------ 1. the target kernel
def _target_case():
    """Two recordings, three windows: window 0 starts at sample 0 of recording 0, windows 1 and 2 inside recordings 1 and 0 at starts
    that are no multiple of 512."""
    notes = {
        # (pitch 0 of recording 0 stays empty)
        (0, 1): [-0 + 5, 320 * 400],                                # far before windows 1 / 2 and past every window's end
        (0, 2): [320 * 5 - 100, 320 * 5 + 100, 320 * 9 + 17],        # two onsets closer than W, equidistant from frame 5 of window 0
        (0, 3): [320 * 60 + 319, 320 * 64, 320 * 64 + 1, 320 * 127 + 160],
        (0, 87): [320 * 3 + 7, 320 * 129 + 300, 320 * 200],
        (1, 2): [100, 1500, 1600, 20000, 41000],
        (1, 40): [12345 // 16 * 10 + 3, 12345 // 16 * 10 + 700],     # near the first frames of window 1 (start 12345 samples = 7715.6 ticks)
    }
    on_tick, tick_off = _tables(notes, n_rec=2)
    return on_tick, tick_off, [0, 1, 0], [0, 12345, 777]


@pytest.mark.parametrize("T_out", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("J", [2, 8])
def test_target_kernel_equals_the_integer_reference(mta, T_out, J):
    on_tick, tick_off, win_rec, start = _target_case()
    t_keep = [T_out, max(T_out - 3, 0), max(T_out // 2, 1)]
    cells = 0
    for rate in (None, [ONE] * 3, [RATE_LO, RATE_HI, ONE + 12345677], [RATE_HI, RATE_LO, RATE_LO]):
        want = OR.regress_target(on_tick, tick_off, win_rec, start, t_keep, T_out, J, rate)
        got = _target(on_tick, tick_off, win_rec, start, t_keep, T_out, J, rate)
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), (T_out, J, rate, np.argwhere(got != want)[:5])
        cells += int((want > 0).sum())
        assert not want[0, 0].any() and not want[1, 2, t_keep[1]:].any()
    plain, one = (_target(on_tick, tick_off, win_rec, start, t_keep, T_out, J, r) for r in (None, [ONE] * 3))
    assert np.array_equal(plain, one)
    print(f"T_out {T_out} J {J}: {cells} non-zero target cells compared")
    if T_out >= 64:
        assert cells > 100
        w0 = OR.regress_target(on_tick, tick_off, win_rec, start, t_keep, T_out, J)[0, 2]
        assert w0[5] == np.float32(2560 * J - 800) / np.float32(2560 * J)       # the equidistant pair: either is the nearest


# ------------------------------------------------------------------ 2. the dataset
def _small_tree(root, durs):
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "2004"), exist_ok=True)
    rng = np.random.default_rng(0)
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for i, (name, (d, split)) in enumerate(durs.items()):
        n = int(d * 16000)
        t = np.arange(n) / 16000.0
        sig = 0.3 * np.sin(2 * np.pi * 220.0 * (i + 1) * t) * np.exp(-0.5 * (t % 1.7)) + 0.02 * rng.standard_normal(n)
        wavfile.write(os.path.join(root, "2004", f"{name}.wav"), 16000, (sig * 32767).astype(np.int16))
        ev = []
        for k, s in enumerate(np.arange(0.3, d - 1.0, 0.37)):                       # 2000 MIDI ticks per second; onsets at every phase
            ev += note(0, 30 + (k * 7) % 50, int(s * 2000) + 3 * k, int((s + 0.3 + 0.1 * (k % 3)) * 2000))
        with open(os.path.join(root, "2004", f"{name}.midi"), "wb") as fh:
            fh.write(smf([[], ev]))
        rows.append(f"X,Y,{split},2004,2004/{name}.midi,2004/{name}.wav,{d}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("maestro_onsets"))
    _small_tree(root, {"a": (12.0, "train"), "b": (9.5, "train"), "v": (7.0, "validation")})
    return root


def _host_tables(mta, tree, ds):
    from music_transcription_amd import midi as MD, rawdata as RD
    tabs = [RD.label_notes(MD.MidiFile(os.path.join(tree, r["midi_filename"])), 16000 / 512) for r in ds.rows]
    ticks = np.concatenate([t.on_tick for t in tabs])
    base = np.concatenate([[0], np.cumsum([len(t.on_tick) for t in tabs])])
    return ticks, np.concatenate([t.pitch_off + b for t, b in zip(tabs, base)])


def test_dataset_regress_targets(mta, tree):
    kw = dict(split="train", n_mels=64, chunk_length=5.0, overlap=0.25)
    ds = mta.MaestroDataset(tree, onset_labels="midi", onset_target="regress", onset_width=3, **kw)
    ticks, off = _host_tables(mta, tree, ds)
    assert np.array_equal(ds.onset_ticks.cpu().numpy(), ticks) and np.array_equal(ds.onset_tick_off.cpu().numpy(), off)
    idx = [len(ds) - 1, 0, 2, 1]
    mel, labels, lengths = ds.get_batch(idx)
    T = int(lengths.max())
    want = OR.regress_target(ticks, off, ds.rec[idx], ds.start[idx], ds.t_keep[idx], T, 3)
    assert torch.equal(labels["onset"].cpu(), torch.from_numpy(want)) and 0 < (want > 0).mean() < 0.2
    assert (ds.start[idx] % 512 != 0).any()
    point = mta.MaestroDataset(tree, onset_labels="midi", onset_target="point", **kw)
    old = mta.MaestroDataset(tree, onset_labels="midi", **kw)
    for a, b in zip(point.get_batch(idx), old.get_batch(idx)):
        if isinstance(a, dict):
            assert torch.equal(a["frame"], b["frame"]) and torch.equal(a["onset"], b["onset"])
            assert torch.equal(a["frame"], labels["frame"]) and not torch.equal(a["onset"], labels["onset"])
        else:
            assert torch.equal(a, b)
    assert torch.equal(mel, old.get_batch(idx)[0])
    aug = mta.MaestroDataset(tree, onset_labels="midi", onset_target="regress", onset_width=2,
                             augment=mta.Augment(pitch_cents=50.0, generator=torch.Generator().manual_seed(4)), **kw)
    _, la, _ = aug.get_batch(idx)
    rate = aug.last_augment["rate_q32"]
    assert len(set(rate.tolist())) == len(idx) and all(int(r) != ONE for r in rate)
    want_a = OR.regress_target(ticks, off, aug.rec[idx], aug.start[idx], aug.t_keep[idx], T, 2, rate)
    assert torch.equal(la["onset"].cpu(), torch.from_numpy(want_a))
    assert not np.array_equal(want_a, OR.regress_target(ticks, off, aug.rec[idx], aug.start[idx], aug.t_keep[idx], T, 2))
    whole = mta.MaestroDataset(tree, split="train", n_mels=64, onset_labels="midi", onset_target="regress", onset_width=2)
    _, lw, ln = whole.get_batch([1, 0])
    want_w = OR.regress_target(ticks, off, [1, 0], [0, 0], whole.t_keep[[1, 0]], int(ln.max()), 2)
    assert torch.equal(lw["onset"].cpu(), torch.from_numpy(want_w))
    hy = mta.HybridMaestroDataset(tree, cache_dir=os.path.join(tree, "no_cache"), n_mels=64, onset_labels="midi", onset_target="regress",
                                  chunk_length=5.0, overlap=0.25)
    assert not hy.use_cache and hy.dataset.onset_target == "regress" and hy.dataset.onset_width == 2


# ------------------------------------------------------------------ 3. the refinement kernel
def _tri(L, centre, J, lo=0.02, hi=0.98):
    g = np.arange(L, dtype=np.float64)
    q = np.clip(1.0 - np.abs(g - centre) / J, lo, hi)
    return np.log(q / (1.0 - q)).astype(np.float32)


def _check_refine(mta, logits, lengths, chunks, notes_by_row, reaches=(0, 2, 8)):
    """notes_by_row[r] = [(s, e), ...]; compares refine_onsets_device with the float64 reference at every reach."""
    from music_transcription_amd.notes import refine_onsets_device
    NB, P, T = logits.shape
    rows = P if chunks else NB * P
    starts = np.array([s for r in range(rows) for s, _ in notes_by_row.get(r, [])], np.int32)
    ends = np.array([e for r in range(rows) for _, e in notes_by_row.get(r, [])], np.int32)
    row_off = np.concatenate([[0], np.cumsum([len(notes_by_row.get(r, [])) for r in range(rows)])]).astype(np.int64)
    if chunks:
        rows_q = [OR.sigmoid64(np.concatenate([logits[nb, p] for nb in range(NB)])) for p in range(P)]
    else:
        rows_q = [OR.sigmoid64(logits[r // P, r % P, :T if lengths is None else min(max(int(lengths[r // P]), 0), T)]) for r in range(rows)]
    x = torch.from_numpy(logits).cuda()
    worst, left_out = 0, 0
    for reach in reaches:
        want, margin = OR.refine_onsets(rows_q, starts, ends, row_off, reach)
        left_out += int(((margin < 0.05) & (margin > 2.0 ** -12)).sum())
        got = refine_onsets_device(_dev(starts, np.int32), _dev(ends, np.int32), _dev(row_off, np.int64), x, lengths=lengths, chunks=chunks, reach=reach)
        again = refine_onsets_device(_dev(starts, np.int32), _dev(ends, np.int32), _dev(row_off, np.int64), x, lengths=lengths, chunks=chunks, reach=reach)
        assert got.dtype == torch.int32 and torch.equal(got, again)
        g = got.cpu().numpy().astype(np.int64)
        worst = max(worst, int(np.abs(g - want).max()) if len(g) else 0)
        assert (g < 320 * ends).all() and (g >= 0).all()
        for r in range(rows):                                                # the onsets of a row stay sorted
            assert (np.diff(g[row_off[r]:row_off[r + 1]]) >= 0).all()
    assert left_out == 0, left_out                                           # every case is clearly on one side of the 2^-10 guard
    return worst, want


def test_refine_batch_layout_with_lengths_and_nan_padding(mta):
    B, P, T = 2, 3, 12
    x = np.full((B, P, T), -4.0, np.float32)
    x[0, 0] = np.maximum(_tri(T, 4.3, 2), np.where(np.arange(T) >= 9, (np.arange(T) - 9.0) * 1.5 - 1.0, -4.0)).astype(np.float32)
    x[0, 1, 5], x[0, 1, 6] = 1.0, 3.0                                        # a one-frame note under a higher neighbour
    x[0, 2, 1:8] = 2.0                                                       # a plateau
    x[1, 0] = _tri(T, 5.0, 3)                                                # A == C
    x[1, 1, :9] = _tri(9, 8.4, 2)                                            # the peak on the last valid frame
    x[1, :, 9:] = np.nan
    notes = {0: [(3, 7), (9, 12)], 1: [(5, 6)], 2: [(3, 6)], 3: [(3, 8)], 4: [(6, 9)]}
    worst, want = _check_refine(mta, x, [12, 9], False, notes)
    print(f"batch layout: worst |device - float64 reference| = {worst} ticks; reference at reach 8: {want.tolist()}")
    assert worst <= 1
    w2, _ = OR.refine_onsets([OR.sigmoid64(x[r // P, r % P, :(12, 9)[r // P]]) for r in range(B * P)],
                             *[np.array(v) for v in ([3, 9, 5, 3, 3, 6], [7, 12, 6, 6, 8, 9], [0, 2, 3, 4, 5, 6, 6])], 2)
    # the reference on the cases named above: the interpolated peak, the one-frame note (k = s, shift clamped to 0.5), the plateau
    # (shift 0), A == C (shift 0); a peak on the last valid frame has C = 0 outside the row and leans back towards A
    assert w2[0] == round(320 * 4.3) and w2[2] == 320 * 5 + 160 <= 320 * 6 - 1 and w2[3] == 320 * 3 and w2[4] == 320 * 5
    assert 320 * 10 < w2[1] < 320 * 11 and 320 * 7 < w2[5] < 320 * 8


def test_refine_chunk_layout_across_chunk_boundaries(mta):
    NB, P, T = 3, 2, 7
    rows = np.stack([np.maximum(_tri(21, 7.0, 2), _tri(21, 13.6, 3)), np.maximum(_tri(21, 6.6, 2), _tri(21, 20.0, 2))])
    x = np.ascontiguousarray(rows.reshape(P, NB, T).transpose(1, 0, 2))
    worst, want = _check_refine(mta, x, None, True, {0: [(6, 9), (12, 16)], 1: [(5, 8), (19, 21)]})
    print(f"chunk layout: worst |device - float64 reference| = {worst} ticks; reference at reach 8: {want.tolist()}")
    assert worst <= 1
    assert want[0] == 320 * 7 and want[1] == round(320 * 13.6) and want[2] == round(320 * 6.6) and 320 * 19 < want[3] < 320 * 20


def test_refine_without_notes_writes_nothing(mta):
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import refine_onsets_device
    x = torch.zeros(2, 88, 16, device="cuda")
    e32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    out = refine_onsets_device(e32, e32, torch.zeros(2 * 88 + 1, dtype=torch.int64, device="cuda"), x)
    assert out.numel() == 0 and out.dtype == torch.int32
    sentinel = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    row_off = torch.zeros(89, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib.mt_refine_onsets(_lib.ptr(sentinel), _lib.ptr(sentinel), _lib.ptr(row_off), 88, 0, _lib.ptr(x), 2, 88, 16, None, 1, 2,
                                         _lib.ptr(sentinel), _lib.stream_ptr()), "mt_refine_onsets")
    torch.cuda.synchronize()
    assert bool((sentinel == -7).all())
    with pytest.raises(ValueError, match="row_off"):
        refine_onsets_device(e32, e32, torch.ones(2 * 88 + 1, dtype=torch.int64, device="cuda"), x)


# ------------------------------------------------------------------ 4. the round trip on the device
@pytest.mark.parametrize("J", [2, 4])
def test_round_trip_on_the_device(mta, J):
    from music_transcription_amd.notes import FS, heads_to_notes_device, notes_batch_device
    phases = [(p * 8 + 3) % 320 for p in range(40)]
    on = {(0, 20 + p): [320 * (12 + p % 7) + ph, 320 * (40 + p % 5) + (ph * 7) % 320] for p, ph in enumerate(phases)}
    on_tick, tick_off = _tables(on)
    T = 64
    y = torch.from_numpy(_target(on_tick, tick_off, [0, 0], [0, 0], [T, T - 9], T, J)).cuda()
    logits = torch.logit(y, eps=1e-6)
    lengths = [T, T - 9]
    plain = notes_batch_device(logits, logits, lengths=lengths)
    assert notes_batch_device(logits, logits, lengths=lengths, refine_onsets=False) == plain
    fine = notes_batch_device(logits, logits, lengths=lengths, refine_onsets=True, refine_reach=J)
    worst = worst_grid = 0
    for b in range(2):
        assert len(fine[b]) == len(plain[b]) == 80 and [(n[0], n[2]) for n in fine[b]] == [(n[0], n[2]) for n in plain[b]]
        want = sorted((21 + p, t) for (_, p), ts in on.items() for t in ts)
        for (pitch, t0, _), (_, g0, _), (wp, wt) in zip(fine[b], plain[b], want):
            assert pitch == wp and abs(g0 * FS - round(g0 * FS)) < 1e-9
            worst = max(worst, abs(round(t0 * 1e4) - wt))
            worst_grid = max(worst_grid, abs(round(g0 * 1e4) - wt))
    print(f"J {J}: refined onsets within {worst} ticks of the MIDI on_tick at 80 phases; frame-grid stamps within {worst_grid}")
    assert worst <= 1 and worst_grid >= 300
    # the chunk layout: the same rows as two chunks of 32 frames
    x2 = logits[0].reshape(88, 2, 32).permute(1, 0, 2).contiguous()
    chunked = heads_to_notes_device(x2, x2, refine_onsets=True, refine_reach=J)
    assert chunked == fine[0]
    assert heads_to_notes_device(x2, x2, refine_onsets=False) == heads_to_notes_device(x2, x2) == plain[0]
    off = torch.full_like(x2, -20.0)
    assert heads_to_notes_device(x2, x2, offset_logits=off, refine_onsets=True, refine_reach=J) == fine[0]
    assert heads_to_notes_device(x2, x2, min_note_frames=1, bridge_frames=1, refine_onsets=True, refine_reach=J) == fine[0]


# ------------------------------------------------------------------ 5. the scripts
def test_evaluate_script_with_refined_onsets(mta, tree, tmp_path, monkeypatch, capsys):
    """Logits built from the regression targets of a two-recording tree: every MIDI note-on is found, refined or not at width 2; at
    width 4 the frame-grid stamp is up to two frames early and only the refined onsets keep onset F1 = 1."""
    from oracle import model_ref as R
    from music_transcription_amd import evaluate as E
    nm, H, L = 64, 24, 3
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", nm, H, L, 5), ckpt)
    spec = importlib.util.spec_from_file_location("evaluate_script", os.path.join(ROOT, "scripts", "evaluate.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    f1 = {}
    for J in (2, 4):
        src = mta.MaestroDataset(tree, split="train", n_mels=nm, onset_labels="midi", onset_target="regress", onset_width=J)

        def fake(model, dataset, indices, device="cuda", max_batch=128, all_heads=False, with_offset=False):
            out = []
            for i in indices:
                _, lab, _ = src.get_batch([i])
                on = torch.logit(lab["onset"][0], eps=1e-6)
                item = (i, (lab["frame"][0] * 20.0 - 10.0).contiguous(), lab["frame"][0].contiguous())
                out.append(item + ((on, torch.full_like(on, -20.0)) if with_offset else (on,)) if all_heads else item)
            return out
        monkeypatch.setattr(E, "collect_logits", fake)
        for dec in ("onset", "onset_offset"):
            for refine in (True, False):
                argv = ["evaluate.py", "--model", ckpt, "--data_source", "full", "--root_dir", tree, "--split", "train", "--model_type", "cnn_rnn_large",
                        "--n_mels", str(nm), "--hidden_size", str(H), "--num_layers", str(L), "--dropout", "0.0", "--cache_dir", str(tmp_path / "none"),
                        "--note_metrics", "--note_reference", "midi", "--decoder", dec, "--headless"]
                monkeypatch.setattr(sys, "argv", argv + (["--refine_onsets", "--refine_reach", str(J)] if refine else []))
                assert script.main() == 0
                out = capsys.readouterr().out.strip().splitlines()
                assert [l.split("=")[0] for l in out] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1"], out
                f1[J, dec, refine] = float(out[1].split("=")[1])
    print("note-onset F1 (width, decoder, refined):", json.dumps({str(k): v for k, v in f1.items()}))
    for J in (2, 4):
        for dec in ("onset", "onset_offset"):
            assert f1[J, dec, True] == 1.0
    assert f1[2, "onset", False] == 1.0 and f1[4, "onset", False] < 1.0


def test_train_script_one_epoch_of_regression_targets(mta, tree, tmp_path):
    run_dir = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--epochs", "1", "--batch_size", "2", "--n_mels", "64",
                        "--model", "cnn_rnn_large", "--hidden_size", "24", "--num_layers", "3", "--seed", "3", "--num_workers", "0", "--train_all_heads",
                        "--onset_labels", "midi", "--onset_target", "regress", "--onset_width", "3", "--augment_pitch_cents", "20",
                        "--cached_dir", str(tmp_path / "none"), "--root_dir", tree, "--chunk_length", "5", "--run_dir", str(run_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Onset target (training set): regression triangles of 3 frames" in r.stdout
    hist = json.load(open(run_dir / "history.json"))
    print(hist)
    assert len(hist) == 1 and hist[0]["steps"] > 0 and np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"])
