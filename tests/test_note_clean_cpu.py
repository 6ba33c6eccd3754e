"""Note cleanup without a GPU: the literal scan of note_clean_ref.py against the decoders' own references at (1, 0) and against a
restatement on note lists, the milliseconds -> frames table, and the host-side surface (the command lines' flags and the refusals
of notes.py, transcribe.py, evaluate.py, corpus.py and the scripts, all of them before anything is loaded)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import note_clean_ref as CR
import note_metrics_ref as NR
import offset_decode_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        T = int(rng.integers(1, 400))
        p_on, p_off = rng.choice([0.02, 0.1, 0.3]), rng.choice([0.05, 0.3, 0.6])
        yield OR.markov(rng, (T,), p_on, p_off), OR.markov(rng, (T,), 0.08, 0.5), OR.markov(rng, (T,), 0.06, 0.5)


def test_no_cleanup_is_the_three_decoders():
    n = 0
    for f, o, k in _rows(300, 1):
        assert CR.clean_notes(f) == [tuple(x) for x in NR.frame_notes(f)]
        assert CR.clean_notes(f, o) == [tuple(x) for x in NR.onset_notes(f, o)]
        assert CR.clean_notes(f, o, k) == OR.onset_offset_notes(f, o, k)
        n += len(CR.clean_notes(f, o, k))
    assert n > 1000


@pytest.mark.parametrize("M,G", [(1, 0), (2, 0), (1, 1), (3, 2), (5, 10), (64, 63), (64, 0), (1, 63)])
def test_frame_decoder_is_merge_then_drop_on_the_note_list(M, G):
    changed = 0
    for f, _, _ in _rows(300, 2):
        got = CR.clean_notes(f, None, None, M, G)
        assert got == CR.frame_notes_list_rule(f, M, G)
        changed += got != CR.clean_notes(f)
    assert changed > 50 or (M, G) == (1, 0)


def test_cleaned_notes_keep_what_the_matchers_rest_on():
    """Onsets of one pitch >= 2 frames apart, a note ended when the next starts, every note at least M frames, inside the row."""
    for f, o, k in _rows(200, 3):
        for M, G in ((3, 2), (1, 63), (64, 5)):
            for heads in ((f, None, None), (f, o, None), (f, o, k)):
                notes = CR.clean_notes(*heads, M, G)
                assert all(0 <= s < e <= len(f) and e - s >= M for s, e in notes)
                assert all(b[0] >= a[1] and b[0] - a[0] >= 2 for a, b in zip(notes, notes[1:]))
                if heads[1] is not None:                                         # the other two keep their onsets: starts are a subset
                    assert {s for s, _ in notes} <= {s for s, _ in CR.clean_notes(*heads, 1, G)}


@pytest.mark.parametrize("f,o,k,M,G,want", [
    ("0011100111", None, None, 1, 2, [(2, 10)]),                                   # a gap of G is bridged,
    ("0011100011", None, None, 1, 2, [(2, 5), (8, 10)]),                           # one of G + 1 is not,
    ("0011100", None, None, 1, 2, [(2, 5)]),                                       # nor one that reaches the end of the row,
    ("0011100", None, None, 1, 63, [(2, 5)]),                                      # nor the leading one
    ("0011100111", "0010000100", None, 1, 2, [(2, 7), (7, 10)]),                   # the onset edge still splits,
    ("0011100111", "0010000000", None, 1, 2, [(2, 10)]),                           # and without it the note carries on
    ("0011100111", "0010000000", None, 1, 0, [(2, 5)]),                            # instead of ending there with nothing opened after it
    ("0011100111", "0010000000", "0000100000", 1, 2, [(2, 5)]),                    # an offset edge cuts through the bridged gap
    ("0110111101", None, None, 3, 0, [(4, 8)]),                                    # short notes go, their neighbour is not extended
    ("0110111101", None, None, 3, 1, [(1, 10)]),                                   # bridged first: one note, long enough
    ("0111111", "0100100", None, 4, 0, []),                                        # closed by a re-strike, then open at the end: both short
    ("0111111", "0100100", None, 3, 0, [(1, 4), (4, 7)]),
    ("0111111", "0100000", "0001000", 4, 0, []),                                   # cut by an offset edge after 3 frames
])
def test_hand_written_rows(f, o, k, M, G, want):
    row = lambda s: None if s is None else np.array([c == "1" for c in s])
    assert CR.clean_notes(row(f), row(o), row(k), M, G) == want


def _notes_module():
    from music_transcription_amd import notes
    return notes


def test_milliseconds_to_frames():
    c = _notes_module().cleanup_frames
    assert c() == (1, 0)
    table = {0: (1, 0), 31.9: (1, 0), 32: (1, 1), 32.1: (2, 1), 64: (2, 2), 2048: (64, 64), 2047.9: (64, 63)}
    for ms, (M, G) in table.items():
        assert c(ms, 0)[0] == M, ms
        if G <= 63:
            assert c(0, ms)[1] == G, ms
    assert c(2048, 2047.999) == (64, 63)                                          # the two limits
    with pytest.raises(ValueError, match="2048 ms"):
        c(2048.001, 0)
    with pytest.raises(ValueError, match="2048 ms"):
        c(0, 2048)
    for bad in (-1, float("nan"), float("inf"), "64"):
        with pytest.raises(ValueError):
            c(bad, 0)
        with pytest.raises(ValueError):
            c(0, bad)


def _help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_command_lines_name_the_flags():
    main, evaluate, corpus = _help("main.py"), _help("scripts/evaluate.py"), _help("scripts/transcribe_corpus.py")
    assert "--min-note-ms" in main and "--bridge-gap-ms" in main
    assert "--min_note_ms" in evaluate and "--bridge_gap_ms" in evaluate
    assert "--min-note-ms" in corpus and "--bridge-gap-ms" in corpus


def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *args], capture_output=True, text=True, timeout=300)


def test_scripts_refuse_before_anything_is_loaded():
    """argparse's error exit (2) in every case; the files named do not exist, so anything later would have complained about them."""
    for flag, ms in (("--min-note-ms", "2048.5"), ("--bridge-gap-ms", "2048"), ("--min-note-ms", "-1")):
        r = _run("main.py", "none.wav", "none.pth", flag, ms)
        assert r.returncode == 2 and flag[2:].replace("-", "_") in r.stderr, r.stderr
        r = _run("scripts/transcribe_corpus.py", "--wav-dir", "none", flag, ms)
        assert r.returncode == 2 and flag[2:].replace("-", "_") in r.stderr, r.stderr
    r = _run("scripts/evaluate.py", "--model", "none.pth", "--note_metrics", "--bridge_gap_ms", "2048")
    assert r.returncode == 2 and "2048 ms" in r.stderr, r.stderr
    r = _run("scripts/evaluate.py", "--model", "none.pth", "--min_note_ms", "64")
    assert r.returncode == 2 and "--note_metrics" in r.stderr, r.stderr
    r = _run("scripts/evaluate.py", "--model", "none.pth", "--note_metrics", "--tune_note_thresholds", "--bridge_gap_ms", "32")
    assert r.returncode == 2 and "--tune_note_thresholds" in r.stderr and "do not clean" in r.stderr, r.stderr


BAD = [dict(min_note_frames=0), dict(min_note_frames=65), dict(bridge_frames=-1), dict(bridge_frames=64), dict(min_note_frames=2.5),
       dict(bridge_frames=True)]


@pytest.mark.parametrize("kw", BAD)
def test_range_errors_come_before_any_gpu_work(kw):
    """Host tensors and stand-in models: anything past the range check would fail differently."""
    import torch
    from music_transcription_amd import corpus, evaluate, notes, transcribe
    x = torch.zeros(1, 88, 8)
    tables = {"on": torch.zeros(0, dtype=torch.int32), "off": torch.zeros(0, dtype=torch.int32), "ptr": torch.zeros(89, dtype=torch.int64)}
    model = types.SimpleNamespace(model=None)

    def never(*a, **k):
        raise AssertionError("the refusal comes before any audio is asked for")
    calls = [lambda: notes.note_match_counts(x, x, **kw), lambda: notes.note_match_list(x, tables, **kw),
             lambda: notes.heads_to_notes_device(x, x, **kw), lambda: notes.notes_batch_device(x, **kw),
             lambda: transcribe.notes_from_logits_device(x, **kw), lambda: transcribe.transcribe_chunks_to_notes(model, never, **kw),
             lambda: transcribe.transcribe_windows_to_notes(model, never, 2.0, **kw),
             lambda: transcribe.transcribe_audio("none.wav", "none.pth", **kw),
             lambda: evaluate.note_metrics_dataset(model, never, **kw),
             lambda: corpus.transcribe_shard(model, [0], never, n_mels=32, device="cuda", **kw),
             lambda: corpus.transcribe_shard_windows(model, [0], never, overlap_s=1.0, n_mels=32, device="cuda", **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="min_note_frames|bridge_frames"):
            call()


def test_tuning_with_cleanup_is_refused():
    from music_transcription_amd import evaluate

    def never(*a, **k):
        raise AssertionError("the refusal comes first")
    for kw in (dict(min_note_frames=2), dict(bridge_frames=1), dict(min_note_frames=64, bridge_frames=63)):
        with pytest.raises(ValueError, match="do not clean.*tune without cleanup, then evaluate with it"):
            evaluate.tune_note_thresholds(never, never, log=None, **kw)
    with pytest.raises(ValueError, match="min_note_frames"):
        evaluate.tune_note_thresholds(never, never, log=None, min_note_frames=0)


def test_corpus_paths_keep_refusing_the_offset_gated_decoder(monkeypatch):
    from music_transcription_amd import corpus, evaluate
    monkeypatch.setattr(evaluate, "require_heads", lambda model, what: None)
    model = types.SimpleNamespace(model=None)
    with pytest.raises(ValueError, match="corpus"):
        corpus.transcribe_shard(model, [0], None, n_mels=32, device="cuda", decoder="onset_offset", min_note_frames=2)
    with pytest.raises(ValueError, match="corpus"):
        corpus.transcribe_shard_windows(model, [0], None, overlap_s=1.0, n_mels=32, device="cuda", decoder="onset_offset", bridge_frames=2)
