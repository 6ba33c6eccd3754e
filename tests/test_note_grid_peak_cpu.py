"""Peak-picked onsets in the decoder grid, without a GPU (DESIGN.md 6c "Peak picking in the decoder grid"): the ridge identity the kernel
rests on, the search over the third discrete axis, the refusals of the Python calls, the entry points and the script, and the coverage
condition of the grid that test_gpu_note_grid_peak.py runs."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_grid_peak_case as PC  # noqa: E402
import peak_decode_ref as PR  # noqa: E402
from note_grid_case import LENGTHS  # noqa: E402


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    return m


def _rows(rng, n, L):
    """Random logits on a coarse lattice (ties abound) with planted plateaus of 2-5 equal frames, at the row's ends too."""
    for _ in range(n):
        x = (rng.integers(-12, 13, size=L) / 4.0).astype(np.float32)
        for s in list(rng.integers(0, max(1, L - 5), size=6)) + [0, max(0, L - 3)]:
            x[s:s + int(rng.integers(2, 6))] = np.float32(rng.integers(0, 13) / 4.0)
        yield x


def test_peak_mask_is_the_onset_mask_and_the_ridge():
    rng = np.random.default_rng(0)
    seen = 0
    for L in (1, 2, 3, 9, 64, 65, 150):
        for x in _rows(rng, 6, L):
            for thr in (0.3, 0.5, 0.8):
                o = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))) > np.float32(thr)
                for R in range(1, 9):
                    want = PR.peak_mask(x, o, R)
                    np.testing.assert_array_equal(o & PC.ridge(x, R), want)
                    np.testing.assert_array_equal(PC.starts(x, o, R), want)
                    seen += int(want.sum())
                np.testing.assert_array_equal(PC.ridge(x, 0), np.ones(L, bool))
    assert seen > 500
    # the ridge of reach R is the ridge of R - 1 with the comparisons at distance R added
    x = next(_rows(rng, 1, 200))
    for R in range(1, 9):
        assert not (PC.ridge(x, R) & ~PC.ridge(x, R - 1)).any()


def test_fast_notes_is_the_literal_scan():
    case = PC.Case()
    n = 0
    for (b, p), (M, G), R, with_k in itertools.product(((0, 0), (1, 3), (4, 1), (7, 2), (10, 4)), ((1, 0), (3, 2), (64, 63)), (0, 1, 8),
                                                       (False, True)):
        L = LENGTHS[b]
        f, o, k = (case.host_act(h, t)[b, p, :L] for h, t in (("frame", 0.5), ("onset", 0.35), ("offset", 0.5)))
        st = PC.starts(case.onset[b, p, :L], o, R)
        want = PR.peak_notes(f, o, st, k if with_k else None, M, G)
        assert PC.fast_notes(f, o, st, k if with_k else None, M, G) == want
        n += len(want)
    assert n > 300


def test_search_finds_a_planted_optimum_at_a_nonzero_reach(mta):
    from music_transcription_amd import evaluate as E
    cleanups, smoothings, reaches = [(1, 0), (3, 2)], [(0.0, 0.0), (1.0, 0.5), (2.0, 2.0)], [0, 1, 4]
    n_disc = len(cleanups) * len(smoothings) * len(reaches)
    target = (0.35, 0.65, 1, 2, 2)                          # frame, onset thresholds; cleanup, smoothing, reach indices

    def mean_f1(fts, ots, kts):
        assert kts is None
        out = np.zeros((len(fts), len(ots), 1, n_disc))
        for (i, a), (j, o), d in itertools.product(enumerate(fts), enumerate(ots), range(n_disc)):
            c, s, r = d // len(reaches) // len(smoothings), d // len(reaches) % len(smoothings), d % len(reaches)
            out[i, j, 0, d] = 1.0 - abs(a - target[0]) - abs(o - target[1]) - 0.1 * ((c, s, r) != target[2:])
        return out
    thr, othr, kthr, d, best = E.search_note_decoder(mean_f1, 2, n_disc)
    assert kthr is None and abs(thr - 0.35) < 0.02 and abs(othr - 0.65) < 0.02 and best > 0.97
    assert E.decoder_candidate(d, cleanups, smoothings, reaches) == ((3, 2), (2.0, 2.0), 4)
    # the order of the discrete axis: cleanup-major, reaches innermost; without reaches the pairs as before
    got = [E.decoder_candidate(d, cleanups, smoothings, reaches) for d in range(n_disc)]
    assert got == [(c, s, r) for c in cleanups for s in smoothings for r in reaches]
    assert E.decoder_candidate(4, cleanups, smoothings) == ((3, 2), (1.0, 0.5))
    with pytest.raises(ValueError):
        E.decoder_candidate(n_disc, cleanups, smoothings, reaches)
    f1 = np.arange(2 * 3 * 3 * 4 * 1 * 2 * 3, dtype=np.float64).reshape(2, 3, 3, 4, 1, 2, 3)      # (n, Kf, Ks, Ko, Kk, Kc, Kr)
    folded = E.fold_reaches(f1)
    assert folded.shape == (2, 3, 4, 1, 18)
    for c, s, r in itertools.product(range(2), range(3), range(3)):
        np.testing.assert_array_equal(folded[..., (c * 3 + s) * 3 + r], f1[:, :, s, :, :, c, r])


def test_python_calls_refuse_before_any_gpu_work(mta):
    from music_transcription_amd import evaluate as E, notes as N
    x = object()                                            # never looked at: the reaches are checked first
    for bad in ([9], [-1], [True], [1.5], [], [0, 1, 9], 9, True, "12"):
        with pytest.raises(ValueError, match="peak_reaches"):
            N.note_grid_counts(x, x, [0.5], onset_logits=x, onset_thresholds=[0.5], peak_reaches=bad)
        with pytest.raises(ValueError, match="peak_reaches"):
            E.tune_note_decoder(x, x, decoder="onset", peak_reaches=bad)
    with pytest.raises(ValueError, match="onset_logits"):
        N.note_grid_counts(x, x, [0.5], peak_reaches=[0, 1])
    with pytest.raises(ValueError, match="decoder 'onset'"):
        E.tune_note_decoder(x, x, decoder="frame", peak_reaches=[0, 1])
    assert list(N.check_peak_reaches([0, 8, np.int64(3), 3])) == [0, 8, 3, 3]
    # a fixed detector stays refused, and the message names the way in
    for call in (lambda: N.note_grid_counts(x, x, [0.5], onset_detect="peak"), lambda: E.tune_note_decoder(x, x, onset_detect="peak"),
                 lambda: E.tune_note_decoder(x, x, onset_detect="peak", peak_reaches=[1])):
        with pytest.raises(ValueError, match="out of scope.*peak_reaches="):
            call()
    with pytest.raises(ValueError, match="out of scope") as e:
        N.note_sweep_counts(x, x, [0.5], onset_detect="peak")
    assert "peak_reaches" not in str(e.value)


def test_entry_points_refuse_bad_arguments_without_a_gpu(mta):
    """NULL onset logits, Kr = 0, a reach of 9 (or -1) and a product of 65: MT_EINVAL before anything is launched or written (there is no
    GPU here, and the dummy pointers are host memory that holds the same zeros afterwards)."""
    from music_transcription_amd import _lib
    import ctypes
    lib = _lib.lib
    buf = np.zeros(4 * 80, np.int64)
    one = buf.ctypes.data
    thr = np.full(16, 0.5, np.float32).ctypes.data
    clean = np.array([[1, 0]] * 16, np.int32)
    reach = lambda *r: (ctypes.c_int * len(r))(*r)
    ok = reach(0, 1, 2, 8)
    cases = [  # onset, (Kf, Ko, Kk, Kc), reaches, Kr
        (None, (1, 1, 1, 1), ok, 4), (one, (1, 1, 1, 1), ok, 0), (one, (1, 1, 1, 1), reach(0, 9), 2), (one, (1, 1, 1, 1), reach(-1), 1),
        (one, (1, 13, 1, 1), reach(0, 1, 2, 3, 4), 5), (one, (1, 1, 1, 1), None, 1), (one, (1, 1, 1, 1), reach(*range(9), *range(8)), 17)]
    for off in (None, one):
        for on, (Kf, Ko, Kk, Kc), r, Kr in cases:
            heads = (on, off, thr, Ko, thr, Kk, clean.ctypes.data, Kc, r, Kr)
            calls = {"mt_note_grid_counts_peak": lambda: lib.mt_note_grid_counts_peak(one, *heads[:2], thr, Kf, *heads[2:], one, None, one, 1, 88, 8, None),
                     "mt_note_grid_list_peak": lambda: lib.mt_note_grid_list_peak(one, *heads[:2], thr, Kf, *heads[2:], one, one, one, None, one, 1, 88, 8, None),
                     "mt_note_grid_counts_paths_peak": lambda: lib.mt_note_grid_counts_paths_peak(one, Kf, *heads, one, None, one, 1, 88, 8, None),
                     "mt_note_grid_list_paths_peak": lambda: lib.mt_note_grid_list_paths_peak(one, Kf, *heads, one, one, one, None, one, 1, 88, 8, None)}
            for name, call in calls.items():
                assert call() == -1, (name, on, Kr)
                assert name in _lib.last_error(), _lib.last_error()
    assert "Kr" in _lib.last_error()
    assert not buf.any()
    for name in ("mt_note_grid_counts_peak", "mt_note_grid_list_peak", "mt_note_grid_counts_paths_peak", "mt_note_grid_list_paths_peak"):
        assert name in _lib.EXPORTS


def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [["--tune_peak_reach", "1"], ["--note_metrics", "--decoder", "onset", "--tune_peak_reach", "0", "1"],
                                  ["--note_metrics", "--tune_note_decoder", "--decoder", "frame", "--tune_peak_reach", "1"],
                                  ["--note_metrics", "--tune_note_decoder", "--tune_peak_reach", "1"],
                                  ["--note_metrics", "--tune_note_decoder", "--decoder", "onset", "--tune_peak_reach", "0", "9"],
                                  ["--note_metrics", "--tune_note_decoder", "--decoder", "onset_offset", "--tune_peak_reach", "-1"],
                                  ["--note_metrics", "--tune_note_decoder", "--decoder", "onset", "--tune_peak_reach", "1.5"],
                                  ["--note_metrics", "--tune_note_decoder", "--decoder", "onset", "--tune_peak_reach"]])
def test_evaluate_script_refuses(args):
    r = _run("--model", "none.pth", *args)
    assert r.returncode == 2 and "--tune_peak_reach" in r.stderr, r.stderr


def test_evaluate_script_documents_the_flag():
    r = _run("--help")
    assert r.returncode == 0 and "--tune_peak_reach" in r.stdout and "EVAL_NOTE_PEAK_REACH=" in r.stdout.replace("\n", " ")


def test_the_gpu_grid_is_not_vacuous():
    """The coverage condition of test_gpu_note_grid_peak.py's 2 x 2 x 2 x 2 x 4 grid (offset-gated decoder, roll reference, LENGTHS) on the
    numpy restatement: at least half of the 64 count rows are pairwise distinct, and every two candidate reaches differ in some cell."""
    case = PC.Case()
    g = PC.GRID_PEAK
    want = PC.cpu_counts(case, "roll", "onset_offset", g["tf"], g["to"], g["tk"], g["cleanups"], g["reaches"], LENGTHS)
    assert want.shape[1:] == (2, 2, 2, 2, 4, 4)
    rows = {tuple(want[(slice(None), *idx)].reshape(-1)) for idx in np.ndindex(2, 2, 2, 2, 4)}
    print("distinct count rows:", len(rows))
    assert len(rows) >= 32, len(rows)
    for r1, r2 in itertools.combinations(range(4), 2):
        differ = int((want[..., r1, :] != want[..., r2, :]).any(axis=(0, -1)).sum())
        print("reaches", g["reaches"][r1], g["reaches"][r2], "differ in", differ, "of 16 cells")
        assert differ >= 1
    # the plateaus are there, also at the ends of the rows, and the planted maxima straddle the slab boundaries
    x = case.onset
    for b, L in enumerate(LENGTHS):
        for t in (0, 63, 511, 1023, L - 2):
            if 0 <= t and t + 1 < L:
                assert (x[b, :, t] == x[b, :, t + 1]).all()
    assert (x[0, :, 504:512].max(axis=1) >= 4.5).any() and (x[0, :, 512:520].max(axis=1) >= 4.5).any()
    assert (x[0, :, 1016:1024].max(axis=1) >= 4.5).any() and (x[0, :, 1024:1032].max(axis=1) >= 4.5).any()
    assert want[..., 2].sum() > 0 and (want[..., 3] <= want[..., 2]).all()
