"""CPU tests of the sub-frame onsets (DESIGN.md 6c "Sub-frame onsets"): the identity between the regression target and the peak
interpolation on the numpy reference (onset_regress_ref), the host matcher notes.note_match_ticks against scipy's maximum bipartite
matching and against the frame-grid reference, and the refusals of the new options that need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import onset_regress_ref as OR  # noqa: E402


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _tables(per_pitch, n_rec=1):
    """{(rec, pitch): [on_tick, ...]} -> (on_tick int32, tick_off int64 (n_rec * 89,))."""
    ticks, off = [], []
    for r in range(n_rec):
        for p in range(89):
            off.append(len(ticks))
            if p < 88:
                ticks += sorted(per_pitch.get((r, p), []))
    return np.array(ticks, np.int32), np.array(off, np.int64)


@pytest.mark.parametrize("J", [2, 3, 4])
def test_identity_target_then_interpolation(J):
    """One isolated onset per pitch row, the pitch's next onset 2J + 2 frames later: the reference target, logit, the 0.5 edge as the
    note start and the reference refinement give back on_tick to within 1 tick (half a tick from rint, half from tau in 12.5 us units;
    not measured), at every phase of the onset inside its frame.  The frame-grid stamp 320 s is off by up to 319 ticks and more."""
    T, f0, worst, worst_grid = 40, 10, 0, 0
    for phase in range(320):
        on = 320 * f0 + phase
        ticks, off = _tables({(0, 40): [on, on + 320 * (2 * J + 2)]})
        y = OR.regress_target(ticks, off, [0], [0], [T], T, J)[0, 40].astype(np.float64)
        with np.errstate(divide="ignore"):
            q = OR.sigmoid64(np.log(y) - np.log1p(-y))
        notes = OR.onset_notes_of(q > 0.5)
        assert len(notes) == 2
        for (s, e), want in zip(notes, (on, on + 320 * (2 * J + 2))):
            got, k, margin = OR.refine_one(q, s, e, J)
            assert margin >= 2.0 ** -10
            worst = max(worst, abs(got - want))
            worst_grid = max(worst_grid, abs(320 * s - want))
    assert worst <= 1, worst
    assert worst_grid >= 319 and (J != 2 or worst_grid == 319), worst_grid


def test_target_reference_edges():
    ticks, off = _tables({(0, 3): [1000, 1100], (1, 3): [0]}, n_rec=2)
    y = OR.regress_target(ticks, off, [0, 1, 0], [0, 7, 300], [6, 6, 2], 6, 2)
    assert y.shape == (3, 88, 6) and y.dtype == np.float32
    assert not y[:, :3].any() and not y[:, 4:].any()                 # pitches without notes
    # window 0: frame 3 is centred at tick 960: 40 ticks before the first onset, nearer than the second
    assert y[0, 3, 3] == np.float32(5120 - 8 * 40) / np.float32(5120)
    assert y[1, 3, 0] == np.float32(5120 - 35) / np.float32(5120)   # start 7 samples = 35 units after the onset at 0
    assert not y[2, 3, 2:].any() and y[2, 3, 1] > 0                  # t_keep = 2: zero fill
    fast = OR.frame_centres(0, 4, int(1.03 * OR.ONE_Q32))
    assert fast[0] == 0 and fast[3] == (3 * 2560 * int(1.03 * OR.ONE_Q32) + (1 << 31)) >> 32


def _random_rows(rng, rows):
    """Reference and estimated note lists in ticks, estimates off the grid and often three inside one onset window."""
    r_on, r_off, r_ptr, e_on, e_off, e_ptr = [], [], [0], [], [], [0]
    for _ in range(rows):
        n = int(rng.integers(0, 7)) if rng.random() < 0.7 else 0
        on = np.sort(rng.choice(np.arange(0, 12000, 37), size=n, replace=False)) if n else np.zeros(0, np.int64)
        ln = rng.integers(50, 4000, size=n)
        off = on + ln
        if n > 1:
            off[:-1] = np.maximum(np.minimum(off[:-1], on[1:]), on[:-1] + 1)
        r_on += on.tolist()
        r_off += off.tolist()
        r_ptr.append(len(r_on))
        est = []
        for a, b in zip(on, off):
            for _ in range(int(rng.integers(0, 3))):
                est.append((int(a + rng.integers(-700, 701)), int(b + rng.integers(-900, 901))))
        for _ in range(int(rng.integers(0, 3))):
            a = int(rng.integers(0, 12000))
            est.append((a, a + int(rng.integers(1, 3000))))
        est = sorted((max(a, 0), max(b, max(a, 0) + 1)) for a, b in est)
        e_on += [a for a, _ in est]
        e_off += [b for _, b in est]
        e_ptr.append(len(e_on))
    i32 = lambda v: np.array(v, np.int32)
    return ({"on": i32(e_on), "off": i32(e_off), "ptr": np.array(e_ptr, np.int64)},
            {"on": i32(r_on), "off": i32(r_off), "ptr": np.array(r_ptr, np.int64)})


def _scipy_counts(est, ref):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    rows = len(ref["ptr"]) - 1
    out, per_row = np.zeros((rows // 88, 4), np.uint64), np.zeros((rows, 2), np.int64)
    for r in range(rows):
        eo, ef = (est[k][est["ptr"][r]:est["ptr"][r + 1]].astype(np.int64) for k in ("on", "off"))
        ro, rf = (ref[k][ref["ptr"][r]:ref["ptr"][r + 1]].astype(np.int64) for k in ("on", "off"))
        out[r // 88, 0] += len(ro)
        out[r // 88, 1] += len(eo)
        if not len(ro) or not len(eo):
            continue
        near = np.abs(ro[:, None] - eo[None, :]) <= 500
        both = near & (5 * np.abs(rf[:, None] - ef[None, :]) <= np.maximum(2500, rf - ro)[:, None])
        for c, g in enumerate((near, both)):
            per_row[r, c] = int((maximum_bipartite_matching(csr_matrix(g.astype(np.int8)), perm_type="column") >= 0).sum())
            out[r // 88, 2 + c] += per_row[r, c]
    return out, per_row


def test_note_match_ticks_is_a_maximum_matching(mta):
    pytest.importorskip("scipy")
    from music_transcription_amd.notes import note_match_ticks
    est, ref = _random_rows(np.random.default_rng(5), 3 * 88)
    want, per_row = _scipy_counts(est, ref)
    assert (per_row[:, 0] > 0).mean() >= 0.3 and (per_row[:, 1] > 0).mean() >= 0.3, (per_row > 0).mean(axis=0)
    got = note_match_ticks(est, ref)
    assert got.dtype == np.uint64 and got.shape == (3, 4)
    assert np.array_equal(got, want), (got, want)
    assert (want[:, 3] < want[:, 2]).any() and (want[:, 2] < np.minimum(want[:, 0], want[:, 1])).all()
    import torch
    as_t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    assert np.array_equal(note_match_ticks(as_t(est), as_t(ref)), want)
    with pytest.raises(ValueError):
        note_match_ticks({**est, "ptr": est["ptr"][:-1]}, ref)


def test_note_match_ticks_on_the_grid_equals_the_list_reference(mta):
    pytest.importorskip("scipy")
    import note_list_ref as LR
    from music_transcription_amd.notes import note_match_ticks
    rng = np.random.default_rng(11)
    _, ref = _random_rows(rng, 88)
    e_on, e_off, e_ptr, want, hit = [], [], [0], np.zeros(4, np.int64), 0
    for r in range(88):
        ro, rf = (ref[k][ref["ptr"][r]:ref["ptr"][r + 1]] for k in ("on", "off"))
        near = [int(a) // 320 + int(rng.integers(-2, 3)) for a in ro if rng.random() < 0.8]          # frames around the reference onsets
        s = np.unique(np.clip(near + rng.choice(40, size=int(rng.integers(0, 3)), replace=False).tolist(), 0, 39)).astype(np.int64)
        est = [(int(a), int(min(a + rng.integers(1, 9), b))) for a, b in zip(s, list(s[1:]) + [48])]
        e_on += [320 * a for a, _ in est]
        e_off += [320 * b for _, b in est]
        e_ptr.append(len(e_on))
        row = LR.list_row_counts(ro, rf, est)
        want += row
        hit += row[2] > 0
    assert hit >= 0.3 * 88, hit
    est = {"on": np.array(e_on, np.int32), "off": np.array(e_off, np.int32), "ptr": np.array(e_ptr, np.int64)}
    assert np.array_equal(note_match_ticks(est, ref)[0].astype(np.int64), want)


def test_entry_points_refuse_bad_arguments_without_a_gpu(mta):
    from music_transcription_amd import _lib
    lib, one = _lib.lib, np.zeros(4, np.int64).ctypes.data
    for J, T_out in ((1, 8), (9, 8), (2, (1 << 19) + 1)):
        assert lib.mt_onset_regress_windows(one, one, one, one, None, one, 1, T_out, J, one, None) != 0
        assert "onset" in _lib.last_error()
    assert lib.mt_refine_onsets(one, one, one, 88, 1, one, 1, 88, 8, None, 0, 9, one, None) != 0       # reach
    assert lib.mt_refine_onsets(one, one, one, 87, 1, one, 1, 88, 8, None, 0, 2, one, None) != 0       # rows of the layout
    assert lib.mt_refine_onsets(one, one, one, 88, 1, one, 1, 88, 8, one, 1, 2, one, None) != 0        # chunks with lengths
    assert lib.mt_refine_onsets(one, one, one, 88, 1, one, 4, 88, 1 << 21, None, 1, 2, one, None) != 0  # 320 L past int32
    assert lib.mt_refine_onsets(None, None, None, 88, 0, None, 1, 88, 8, None, 0, 2, None, None) == 0  # no notes: nothing to do


def test_options_are_checked_before_any_gpu_work(mta):
    from music_transcription_amd import notes as N, transcribe as TR
    with pytest.raises(ValueError, match="onset_target"):
        mta.MaestroDataset("nowhere", onset_labels="midi", onset_target="triangle")
    with pytest.raises(ValueError, match="onset_labels='midi'"):
        mta.MaestroDataset("nowhere", onset_target="regress")
    for w in (1, 9, 2.0, True):
        with pytest.raises(ValueError, match="onset_width"):
            mta.MaestroDataset("nowhere", onset_labels="midi", onset_target="regress", onset_width=w)
    with pytest.raises(ValueError, match="sr 16000, hop 512"):
        mta.MaestroDataset("nowhere", onset_labels="midi", onset_target="regress", hop_length=256)
    with pytest.raises(ValueError, match="frame decoder"):
        N.heads_to_notes_device(None, None, refine_onsets=True)
    with pytest.raises(ValueError, match="frame decoder"):
        N.notes_batch_device(None, None, refine_onsets=True)
    with pytest.raises(ValueError, match="refine_reach"):
        N.notes_batch_device(None, object(), refine_onsets=True, refine_reach=9)
    with pytest.raises(ValueError, match="onset"):
        TR.transcribe_audio("a.wav", "m.pth", decoder="frame", refine_onsets=True)


def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [["--onset_target", "regress"], ["--onset_target", "regress", "--train_all_heads", "--model", "cnn_rnn_large"],
                                  ["--onset_target", "regress", "--onset_labels", "midi"],
                                  ["--onset_target", "regress", "--onset_labels", "midi", "--train_all_heads", "--model", "cnn_rnn_large",
                                   "--onset_width", "1"]])
def test_train_script_refuses(args):
    r = _run("scripts/train_cnn.py", *args)
    assert r.returncode == 2 and ("--onset_target regress" in r.stderr or "--onset_width" in r.stderr or "--onset_labels midi" in r.stderr), r.stderr


@pytest.mark.parametrize("args", [["--refine_onsets"], ["--refine_onsets", "--note_metrics"],
                                  ["--refine_onsets", "--note_metrics", "--note_reference", "midi"],
                                  ["--refine_onsets", "--note_metrics", "--note_reference", "midi", "--decoder", "onset", "--tune_threshold"],
                                  ["--refine_onsets", "--note_metrics", "--note_reference", "midi", "--decoder", "onset", "--tune_note_thresholds"],
                                  ["--refine_onsets", "--note_metrics", "--note_reference", "midi", "--decoder", "onset_offset", "--tune_note_decoder"],
                                  ["--refine_onsets", "--note_metrics", "--note_reference", "midi", "--decoder", "onset", "--refine_reach", "9"]])
def test_evaluate_script_refuses(args):
    r = _run("scripts/evaluate.py", "--model", "none.pth", *args)
    assert r.returncode == 2 and "--refine_" in r.stderr, r.stderr


def test_main_refuses_refinement_with_the_frame_decoder():
    r = _run("main.py", "a.wav", "m.pth", "--refine-onsets")
    assert r.returncode == 2 and "refine_onsets needs decoder" in r.stderr, r.stderr
    for script in ("main.py", "scripts/evaluate.py", "scripts/train_cnn.py"):
        h = _run(script, "--help").stdout
        assert ("--refine-onsets" in h) or ("--refine_onsets" in h) or ("--onset_target" in h), script
