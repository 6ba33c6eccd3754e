"""Note decoders and note matching on the host (note_metrics_ref.py), note_prf, and the CLI flags of the note-level features.

The kernels of csrc/notes.hip count matches with a streaming greedy: within one pitch, each reference note in time order takes
the earliest unmatched compatible estimate.  That is exact only because both note lists are disjoint runs; the random cases
here check it against scipy's maximum bipartite matching, for both of mir_eval's criteria."""
import os
import subprocess
import sys

import numpy as np
import pytest

import note_metrics_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(ref, est):
    return NR.max_matching(ref, est, False), NR.max_matching(ref, est, True)


def test_restrike_is_split_by_an_onset_edge():
    f = np.zeros(20, bool)
    f[2:15] = True
    o = np.zeros(20, bool)
    o[2:4] = True                                # onset held for two frames: one edge
    o[9] = True                                  # a new edge inside the held note
    assert NR.onset_notes(f, o) == [(2, 9), (9, 15)]
    assert NR.frame_notes(f) == [(2, 15)]
    o2 = np.zeros(20, bool)
    o2[17] = True                                # onset without frame activity: a one-frame note
    assert NR.onset_notes(f, o2) == [(17, 18)]   # frame activity without an onset starts nothing
    o3 = np.zeros(20, bool)
    o3[18:] = True                               # runs to the end
    assert NR.onset_notes(f, o3) == [(18, 20)]


@pytest.mark.parametrize("d,hit", [(-2, False), (-1, True), (0, True), (1, True), (2, False)])
def test_onset_tolerance_is_one_frame(d, hit):
    ref = [(10, 20)]
    est = [(10 + d, 20)]
    assert _counts(ref, est)[0] == int(hit)
    assert NR.greedy_matching(ref, est, False) == int(hit)


def test_offset_boundary():
    # len_r = 10: |d off| <= max(1, 10 / 5) = 2 frames is in, 3 is out
    assert _counts([(0, 10)], [(0, 12)]) == (1, 1)
    assert _counts([(0, 10)], [(0, 13)]) == (1, 0)
    assert _counts([(0, 10)], [(0, 8)]) == (1, 1)
    assert _counts([(0, 10)], [(0, 7)]) == (1, 0)
    # short notes: 50 ms = 1 frame of slack whatever the length
    assert _counts([(0, 2)], [(1, 3)]) == (1, 1)
    assert _counts([(0, 2)], [(0, 4)]) == (1, 0)
    # len_r = 15 -> 3 frames in, 4 out
    assert _counts([(5, 20)], [(4, 23)]) == (1, 1)
    assert _counts([(5, 20)], [(4, 24)]) == (1, 0)


def test_empty_lists_and_prf():
    assert _counts([], [(0, 3)]) == (0, 0) and _counts([(0, 3)], []) == (0, 0)
    assert NR.prf(0, 0, 0) == (0.0, 0.0, 0.0)
    assert NR.prf(0, 3, 0) == (0.0, 0.0, 0.0)
    assert NR.prf(2, 4, 2) == (1.0, 0.5, 2 * 2 / 6)


def test_lengths_cut_notes():
    f = np.zeros((1, 1, 12), bool)
    f[0, 0, 3:12] = True
    ref = np.zeros((1, 1, 12), np.float32)
    ref[0, 0, 3:7] = 1.0
    ref[0, 0, 9:12] = 1.0
    # with 8 valid frames: est (3, 8), ref (3, 7) -> onset match, offsets 1 apart -> both criteria
    np.testing.assert_array_equal(NR.match_counts_active(f, ref, lengths=[8]), [[1, 1, 1, 1]])
    np.testing.assert_array_equal(NR.match_counts_active(f, ref), [[2, 1, 1, 0]])
    np.testing.assert_array_equal(NR.match_counts_active(f, ref, lengths=[0]), [[0, 0, 0, 0]])


def _random_runs(rng, T, p_on, p_off):
    out = np.zeros(T, bool)
    s = False
    for t in range(T):
        s = (rng.random() >= p_off) if s else (rng.random() < p_on)
        out[t] = s
    return out


def test_greedy_in_order_matching_is_maximum():
    rng = np.random.default_rng(0)
    n_nontrivial = 0
    for k in range(400):
        T = int(rng.integers(5, 120))
        p_on, p_off = rng.uniform(0.05, 0.6), rng.uniform(0.1, 0.9)
        ref = NR.frame_notes(_random_runs(rng, T, p_on, p_off))
        f = _random_runs(rng, T, p_on, p_off)
        o = _random_runs(rng, T, rng.uniform(0.05, 0.5), 0.7)
        for est in (NR.frame_notes(f), NR.onset_notes(f, o)):
            for off in (False, True):
                a, b = NR.greedy_matching(ref, est, off), NR.max_matching(ref, est, off)
                assert a == b, (k, off, ref, est)
                n_nontrivial += a > 0
    assert n_nontrivial > 300


def test_onset_decoder_with_onset_equal_frame_is_the_frame_decoder():
    rng = np.random.default_rng(1)
    for _ in range(300):
        f = _random_runs(rng, int(rng.integers(1, 200)), rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9))
        assert NR.onset_notes(f, f) == NR.frame_notes(f)


def test_note_prf_on_counts():
    from music_transcription_amd.notes import note_prf
    got = note_prf(np.array([[4, 2, 2, 1], [0, 0, 0, 0], [3, 0, 0, 0], [5, 5, 5, 5]]))
    assert got[0] == {"onset": (1.0, 0.5, 2 * 2 / 6), "onset_offset": (0.5, 0.25, 2 / 6)}
    assert got[1]["onset"] == (0.0, 0.0, 0.0) and got[2]["onset_offset"] == (0.0, 0.0, 0.0)
    assert got[3]["onset_offset"] == (1.0, 1.0, 1.0)


@pytest.mark.parametrize("script,flags", [
    ("main.py", ["--decoder", "--onset-threshold"]),
    ("scripts/evaluate.py", ["--note_metrics", "--decoder", "--onset_threshold"]),
    ("scripts/transcribe_corpus.py", ["--decoder", "--onset-threshold", "--note-metrics"]),
    ("scripts/train_cnn.py", ["--train_all_heads"]),
])
def test_cli_flags_exist(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for f in flags:
        assert f in r.stdout, (script, f)


def test_train_all_heads_refuses_models_without_heads():
    for extra in (["--model", "cnn_rnn"], ["--model", "cnn_rnn_large", "--no_onset_offset_heads"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--train_all_heads"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--train_all_heads" in r.stderr, r.stderr[-2000:]
