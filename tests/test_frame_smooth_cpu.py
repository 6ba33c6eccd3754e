"""Frame smoothing without a GPU (DESIGN.md 6c "Frame smoothing"): the specification of frame_smooth_ref.py against a brute force over
all paths, its reduction to the threshold at (0, 0), the two hand cases, the quantiser's edges, and the host-side surface (argument
checks, the tuners' refusals and the command lines' flags, all of them before anything touches a GPU)."""
import itertools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import frame_smooth_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENALTIES = [(a, b) for a in (0, 1, 2, 5) for b in (0, 1, 2, 5)]


def _check_optimal(q):
    """Rows q (N, T): the scan's score is the brute-force maximum, and where that maximum is unique the path is the same."""
    unique = 0
    for a, b in PENALTIES:
        s = FR.viterbi_path(q, a, b)
        best, n_best, arg = FR.best_paths(q, a, b)
        assert np.array_equal(FR.score(q, s, a, b), best), (a, b)
        one = n_best == 1
        assert np.array_equal(s[one], arg[one]), (a, b)
        unique += int(one.sum())
    return unique


@pytest.mark.parametrize("T", range(1, 8))
def test_the_scan_is_optimal_on_every_small_row(T):
    q = np.asarray(list(itertools.product(range(-3, 4), repeat=T)), np.int64).reshape(-1, T)
    assert len(q) == 7 ** T
    unique = sum(_check_optimal(q[i:i + 100000]) for i in range(0, len(q), 100000))
    assert unique > len(q)                                                       # (of 16 x 7^T cases: the path is compared, too)


def test_the_scan_is_optimal_on_random_rows():
    rng = np.random.default_rng(7)
    lengths = rng.integers(1, 13, 2000)
    for T in range(1, 13):
        n = int((lengths == T).sum())
        assert n > 0
        _check_optimal(rng.integers(-9, 10, (n, T)))


def test_no_penalty_is_the_threshold():
    rng = np.random.default_rng(8)
    q = rng.integers(-50, 51, (200, 40))
    assert np.array_equal(FR.viterbi_path(q, 0, 0), q > 0)
    x = rng.normal(0, 2, (2, 3, 50)).astype(np.float32)
    for thr in (0.3, 0.5, 0.8):
        assert np.array_equal(FR.smooth_ref(x, thr, 0.0, 0.0) > 0, FR.active(x, thr))


def test_hand_cases():
    blip = np.float32([-5, -5, 1, 1, -5, -5])
    drop = np.float32([5, 5, -0.2, 5, 5, 5])
    path = lambda x, p: (FR.smooth_ref(x[None, None], 0.5, p, p)[0, 0] > 0).astype(int).tolist()
    assert FR.penalty(1.5) == 96 and FR.quantise(blip, 0.5).tolist() == [-320, -320, 64, 64, -320, -320]
    assert path(blip, 1.5) == [0] * 6                                            # 128 of evidence against a + b = 192
    assert path(drop, 1.5) == [1] * 6                                            # 13 of counter-evidence against 192
    # on = off = 1.0: the blip's evidence of 128 equals a + b, so keeping and removing it score the same.  The back-pointer rule
    # (s_t = 1 only if d_t > b: a tie from on goes to off) removes it; one grid step less on either penalty and it stays.
    best, n_best, _ = FR.best_paths(FR.quantise(blip, 0.5)[None], 64, 64)
    assert n_best[0] == 2 and FR.score(FR.quantise(blip, 0.5), [0, 0, 1, 1, 0, 0], 64, 64) == best[0] == 0
    assert path(blip, 1.0) == [0] * 6
    keep = lambda on, off: (FR.smooth_ref(blip[None, None], 0.5, on, off)[0, 0] > 0).astype(int).tolist()
    assert keep(63 / 64, 1.0) == keep(1.0, 63 / 64) == [0, 0, 1, 1, 0, 0]
    assert path(blip, 0.0) == [0, 0, 1, 1, 0, 0] and path(drop, 0.0) == [1, 1, 0, 1, 1, 1]
    assert set(np.unique(FR.smooth_ref(drop[None, None], 0.5, 1.5, 1.5))) == {np.float32(64.0)}


def test_quantise_edges():
    for thr in (0.3, 0.5, 0.8):
        c = FR.centre(thr)
        up, down = np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))
        x = np.float32([down, c, up])
        for act in ([False, False, True], [False, True, True], [True, True, True], [False, False, False]):
            q = FR.quantise(x, thr, act)                                         # the grid value is 0 on all three: the activity decides
            assert q.tolist() == [1 if v else 0 for v in act]
        q = FR.quantise(x, thr)                                                  # numpy's own activity: still consistent with the sign
        assert np.array_equal(q > 0, FR.active(x, thr)) and (np.abs(q) <= 1).all()
    inf = np.float32(np.inf)
    assert FR.quantise(np.float32([64, 65, 1e30, inf, -64, -65, -1e30, -inf]), 0.5).tolist() == [4096] * 4 + [-4096] * 4
    assert FR.quantise(np.float32([np.nan]), 0.5).tolist() == [-4096]
    assert FR.quantise(np.float32([np.nan]), 0.5, [False]).tolist() == [-4096]
    assert FR.quantise(np.float32([0.25 + 1 / 128, 0.25 + 3 / 128, -0.3]), 0.5).tolist() == [16, 18, -19]     # halves go to even
    assert FR.centre(0.5) == 0 and FR.penalty(64) == 4096 and FR.penalty(0.5) == 32


# ------------------------------------------------------------------------------------------------ the host-side surface
BAD = [dict(smooth_on=-0.5), dict(smooth_off=-1e-3), dict(smooth_on=64.5), dict(smooth_off=1e9), dict(smooth_on=float("nan")),
       dict(smooth_off=float("inf")), dict(smooth_on="1"), dict(smooth_off=True), dict(smooth_on=None)]


def test_check_smoothing():
    from music_transcription_amd.notes import check_smoothing
    assert check_smoothing() == (0.0, 0.0) and check_smoothing(1, 2.5) == (1.0, 2.5) and check_smoothing(64, np.float32(0.1)) == (64.0, float(np.float32(0.1)))
    for kw in BAD:
        with pytest.raises(ValueError, match="smooth_on|smooth_off"):
            check_smoothing(**kw)


@pytest.mark.parametrize("kw", BAD)
def test_range_errors_come_before_any_gpu_work(kw):
    """Host tensors and stand-in models: anything past the range check would fail differently."""
    import torch
    from music_transcription_amd import evaluate, notes, transcribe
    x = torch.zeros(1, 88, 8)
    tables = {"on": torch.zeros(0, dtype=torch.int32), "off": torch.zeros(0, dtype=torch.int32), "ptr": torch.zeros(89, dtype=torch.int64)}
    model = types.SimpleNamespace(model=None)

    def never(*a, **k):
        raise AssertionError("the refusal comes before any audio is asked for")
    pen = {("on_penalty" if k == "smooth_on" else "off_penalty"): v for k, v in kw.items()}
    calls = [lambda: notes.smooth_frame_logits(x, **pen), lambda: notes.note_match_counts(x, x, **kw), lambda: notes.note_match_list(x, tables, **kw),
             lambda: notes.heads_to_notes_device(x, x, **kw), lambda: notes.notes_batch_device(x, **kw),
             lambda: transcribe.notes_from_logits_device(x, **kw), lambda: transcribe.transcribe_chunks_to_notes(model, never, **kw),
             lambda: transcribe.transcribe_windows_to_notes(model, never, 2.0, **kw),
             lambda: transcribe.transcribe_audio("none.wav", "none.pth", **kw),
             lambda: evaluate.note_metrics_dataset(model, never, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="smooth_on|smooth_off"):
            call()


def test_no_smoothing_returns_the_input_and_launches_nothing(monkeypatch):
    import torch
    from music_transcription_amd import notes

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"{name}: nothing is launched at (0, 0)")
    monkeypatch.setattr(notes, "lib", NoLib())
    x = torch.zeros(2, 3, 8)                                                     # a host tensor: any launch path would refuse it
    assert notes.smooth_frame_logits(x) is x and notes.smooth_frame_logits(x, 0.3, 0.0, 0.0, lengths=[8, 2]) is x
    with pytest.raises(ValueError, match="threshold"):
        notes.smooth_frame_logits(x, 1.0)
    with pytest.raises(ValueError, match="chunks"):
        notes.smooth_frame_logits(x, 0.5, 1.0, 1.0, lengths=[8, 2], chunks=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        notes.smooth_frame_logits(x, 0.5, 1.0, 1.0)


def test_smoothing_a_roll_is_refused():
    import torch
    from music_transcription_amd import transcribe
    with pytest.raises(ValueError, match="is_roll"):
        transcribe.notes_from_logits_device(torch.zeros(1, 88, 8), is_roll=True, smooth_on=1.0)


def test_tuning_with_smoothing_is_refused():
    from music_transcription_amd import evaluate

    def never(*a, **k):
        raise AssertionError("the refusal comes first")
    for kw in (dict(smooth_on=1.0), dict(smooth_off=0.5), dict(smooth_on=64, smooth_off=64)):
        for tuner in (evaluate.tune_threshold, evaluate.tune_note_thresholds, evaluate.tune_note_decoder):
            with pytest.raises(ValueError, match=f"{tuner.__name__}: the tuners do not smooth.*tune without smoothing, then evaluate with it"):
                tuner(never, never, log=None, **kw)
    with pytest.raises(ValueError, match="smooth_on"):
        evaluate.tune_note_decoder(never, never, log=None, smooth_on=-1)


def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *args], capture_output=True, text=True, timeout=300)


def test_command_lines_name_the_flags_and_refuse_before_anything_is_loaded():
    main, evaluate = _run("main.py", "--help"), _run("scripts/evaluate.py", "--help")
    assert main.returncode == 0 and "--smooth-on" in main.stdout and "--smooth-off" in main.stdout
    assert evaluate.returncode == 0 and "--smooth_on" in evaluate.stdout and "--smooth_off" in evaluate.stdout
    assert "raw threshold" in " ".join(evaluate.stdout.split())
    for flag, v in (("--smooth-on", "64.5"), ("--smooth-off", "-1"), ("--smooth-on", "nan")):     # (the files named do not exist)
        r = _run("main.py", "none.wav", "none.pth", flag, v)
        assert r.returncode == 2 and flag[2:].replace("-", "_") in r.stderr, r.stderr
    r = _run("scripts/evaluate.py", "--model", "none.pth", "--note_metrics", "--smooth_off", "65")
    assert r.returncode == 2 and "smooth_off" in r.stderr, r.stderr
    r = _run("scripts/evaluate.py", "--model", "none.pth", "--smooth_on", "1")
    assert r.returncode == 2 and "--note_metrics" in r.stderr, r.stderr
    for tuner in ("--tune_threshold", "--tune_note_thresholds", "--tune_note_decoder"):
        r = _run("scripts/evaluate.py", "--model", "none.pth", "--note_metrics", tuner, "--smooth_on", "1", "--smooth_off", "1")
        assert r.returncode == 2 and tuner in r.stderr and "do not smooth" in r.stderr, r.stderr
