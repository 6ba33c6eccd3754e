"""CPU tests of peak-picked onsets (DESIGN.md 6c "Peak-picked onsets"): the numpy reference peak_decode_ref on hand-written rows, the
demonstration that the edge rule merges two triangles that the peak rule keeps apart, the spacing of peaks, and every refusal of the
new arguments that needs no GPU: Python, command lines and the C ABI."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_clean_ref as CR  # noqa: E402
import note_metrics_ref as NR  # noqa: E402
import onset_regress_ref as OG  # noqa: E402
import peak_decode_ref as PR  # noqa: E402


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _peaks(x, R, thr=0.5):
    x = np.asarray(x, np.float32)
    return np.flatnonzero(PR.peak_mask(x, NR.sigmoid_active(x, thr), R)).tolist()


# ------------------------------------------------------------------------------------------------ the reference on hand-written rows
def test_plateau_gives_its_first_frame():
    assert _peaks([-3, 1, 2, 2, 2, 1, -3], 1) == [2]
    assert _peaks([-3, 1, 2, 2, 2, 1, -3], 3) == [2]
    assert _peaks([2, 2, 2], 1) == [0]                     # a plateau from frame 0 to frame L - 1
    assert _peaks([1, 2, 2, 3, 3, 1], 1) == [1, 3]         # a ledge is a plateau to reach 1, which does not see the step behind it
    assert _peaks([1, 2, 2, 3, 3, 1], 2) == [3]            # reach 2 does: only the top's first frame


def test_peaks_on_the_first_and_the_last_frame():
    assert _peaks([3, 1, -2, 1, 3], 1) == [0, 4]           # frames before 0 and past L - 1 do not exist
    assert _peaks([3, 1, -2, 1, 3], 8) == [0]              # frame 4 ties with frame 0, four frames before it
    assert _peaks([3, 1, -2, 1, 4], 8) == [4]              # and frame 0 has a larger one within its reach
    assert _peaks([2], 1) == [0] and _peaks([-2], 1) == [] and _peaks([], 3) == []


@pytest.mark.parametrize("R", [1, 2, 8])
def test_two_peaks_exactly_reach_plus_one_apart(R):
    x = np.full(40, -4.0, np.float32)
    x[10] = x[10 + R + 1] = 3.0                            # equal heights: neither is inside the other's reach
    assert _peaks(x, R) == [10, 11 + R]
    x[10 + R + 1] = 2.0
    assert _peaks(x, R) == [10, 11 + R]


@pytest.mark.parametrize("R", [1, 2, 8])
def test_a_would_be_peak_reach_frames_from_a_higher_one(R):
    x = np.full(40, -4.0, np.float32)
    x[10], x[10 + R] = 2.0, 3.0                            # the higher one exactly R frames later
    assert _peaks(x, R) == [10 + R]
    x[10], x[10 + R] = 3.0, 2.0                            # and exactly R frames earlier
    assert _peaks(x, R) == [10]
    x[10 + R] = 3.0                                        # a tie R frames apart: the first one
    assert _peaks(x, R) == [10]


def test_threshold_is_part_of_the_rule():
    x = [-5, -1, -5, 1, -5]
    assert _peaks(x, 1) == [3]                             # the maximum at frame 1 does not pass sigmoid > 0.5
    assert _peaks(x, 1, thr=0.2) == [1, 3]


def test_decoding_with_peak_starts():
    """Activity stays f | o, a note opens at each peak, closes when the activity drops or at the next peak; bridging fills the
    activity and leaves the peaks alone; short notes go last."""
    xo = np.array([-4, 1, 3, 2, 3, 1, -4, -4, 2, -4], np.float32)
    xf = np.array([-4, -4, 4, 4, 4, 4, 4, -4, -4, -4], np.float32)
    assert PR.row_notes(xf, xo, None, 10, 1) == [(2, 4), (4, 7), (8, 9)]           # frame 1 is onset-active but no peak: it opens nothing
    assert PR.row_notes(xf, xo, None, 10, 2) == [(2, 7), (8, 9)]                   # frame 4 ties with frame 2, inside its reach
    assert PR.row_notes(xf, xo, None, 10, 1, M=2) == [(2, 4), (4, 7)]
    assert PR.row_notes(xf, xo, None, 10, 1, G=1) == [(2, 4), (4, 8), (8, 9)]      # the gap at 7 is bridged; 8 still starts a note
    xk = np.array([-4, -4, -4, 4, -4, -4, -4, -4, -4, -4], np.float32)
    assert PR.row_notes(xf, xo, xk, 10, 2) == [(2, 4), (8, 9)]                     # the offset edge at 3 makes 3 the last frame
    assert PR.row_notes(xf, xo, None, 4, 1) == [(2, 4)]                            # frames at or past L do not exist


# ------------------------------------------------------------------------------------------------ merge demonstration
@pytest.mark.parametrize("J,on,gap", PR.triangle_pairs())
def test_edge_rule_merges_what_the_peak_rule_separates(J, on, gap):
    y, x = PR.triangle_row(J, on, gap)
    want = [int(round(on / 320)), int(round((on + gap) / 320))]
    dip = float(y[want[0]:want[1] + 1].min())
    assert abs(dip - 0.5) > 1e-3 and dip >= 1 - gap / (2 * 320 * J) - 1e-6, dip     # off the threshold; the continuous dip is a lower bound
    o = NR.sigmoid_active(x, 0.5)
    assert np.array_equal(o, y > 0.5)
    f = np.zeros(len(x), bool)
    edge = CR.clean_notes(f, o)
    assert len(edge) == (1 if dip > 0.5 else 2), (edge, dip)
    peak = PR.row_notes(np.full(len(x), -30.0, np.float32), x, None, len(x), 1)
    assert [s for s, _ in peak] == want, (peak, want)
    if dip > 0.5:
        assert edge[0][0] <= want[0] and edge[0][0] == int(np.flatnonzero(o)[0])   # and the merged note is stamped at the mask's first frame


def test_the_demonstration_covers_merged_pairs_at_every_width():
    merged = {J for J, on, gap in PR.triangle_pairs() if PR.triangle_row(J, on, gap)[0][10:int(round((on + gap) / 320)) + 1].min() > 0.5}
    assert merged == {2, 4, 8}


# ------------------------------------------------------------------------------------------------ spacing
@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_reference_peaks_are_more_than_reach_apart(R):
    rng = np.random.default_rng(R)
    for _ in range(20):
        L = int(rng.integers(1, 200))
        x = np.rint(4 * rng.standard_normal(L)) / 4         # many exact ties
        pk = _peaks(x, R, thr=0.3)
        assert all(b - a > R for a, b in zip(pk, pk[1:])), (R, pk)


# ------------------------------------------------------------------------------------------------ refusals
def test_check_onset_detect(mta):
    from music_transcription_amd import notes as N
    assert N.check_onset_detect() == 0 and N.check_onset_detect("edge", 8) == 0 and N.check_onset_detect("edge", 1, has_onset=False) == 0
    assert N.check_onset_detect("peak") == 1 and N.check_onset_detect("peak", 8) == 8 and N.check_onset_detect("peak", np.int64(3)) == 3
    for bad in ("Peak", "max", None, 1):
        with pytest.raises(ValueError, match="onset_detect"):
            N.check_onset_detect(bad)
    for bad in (0, 9, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="peak_reach"):
            N.check_onset_detect("peak", bad)
    with pytest.raises(ValueError, match="frame decoder"):
        N.check_onset_detect("peak", 1, has_onset=False)


def test_python_calls_refuse_before_any_gpu_work(mta):
    from music_transcription_amd import corpus as C, evaluate as E, notes as N, transcribe as TR
    x = object()                                           # never looked at: the detector is checked first
    for call in (lambda **k: N.note_match_counts(x, x, **k), lambda **k: N.note_match_list(x, {}, **k),
                 lambda **k: N.heads_to_notes_device(x, None, **k), lambda **k: N.notes_batch_device(x, None, **k)):
        with pytest.raises(ValueError, match="frame decoder"):
            call(onset_detect="peak")
    with pytest.raises(ValueError, match="frame decoder"):
        N.notes_ticks_device(x, None, onset_detect="peak")
    for call in (lambda **k: N.note_match_counts(x, x, onset_logits=x, **k), lambda **k: N.note_match_list(x, {}, onset_logits=x, **k),
                 lambda **k: N.heads_to_notes_device(x, x, **k), lambda **k: N.notes_batch_device(x, x, **k),
                 lambda **k: N.notes_ticks_device(x, x, **k)):
        with pytest.raises(ValueError, match="peak_reach"):
            call(onset_detect="peak", peak_reach=9)
        with pytest.raises(ValueError, match="onset_detect"):
            call(onset_detect="maxima")
    # the sweep and grid kernels, and the three tuners on top of them, have no peak mode
    for call in (lambda: N.note_sweep_counts(x, x, [0.5], onset_detect="peak"), lambda: N.note_grid_counts(x, x, [0.5], onset_detect="peak"),
                 lambda: E.tune_threshold(x, x, onset_detect="peak"), lambda: E.tune_note_thresholds(x, x, onset_detect="peak"),
                 lambda: E.tune_note_decoder(x, x, onset_detect="peak")):
        with pytest.raises(ValueError, match="out of scope"):
            call()
    with pytest.raises(ValueError, match="frame decoder"):
        E.note_metrics_dataset(x, x, onset_detect="peak")                      # onset_threshold None: the frame decoder
    with pytest.raises(ValueError, match="peak_reach"):
        E.note_metrics_dataset(x, x, onset_threshold=0.5, onset_detect="peak", peak_reach=0)
    with pytest.raises(ValueError, match="onset_detect='peak' needs decoder"):
        TR.transcribe_audio("a.wav", "m.pth", decoder="frame", onset_detect="peak")
    with pytest.raises(ValueError, match="peak_reach"):
        TR.transcribe_audio("a.wav", "m.pth", decoder="onset", onset_detect="peak", peak_reach=9)
    for fn in (TR.transcribe_chunks_to_notes, ):
        with pytest.raises(ValueError, match="onset_detect='peak' needs decoder"):
            fn(None, None, decoder="frame", onset_detect="peak")
    with pytest.raises(ValueError, match="onset_detect='peak' needs decoder"):
        TR.transcribe_windows_to_notes(None, None, 1.0, decoder="frame", onset_detect="peak")
    for fn, kw in ((C.transcribe_shard, {}), (C.transcribe_shard_windows, {"overlap_s": 1.0})):
        with pytest.raises(ValueError, match="onset_detect='peak' needs decoder"):
            fn(None, [], None, n_mels=64, device="cuda", decoder="frame", onset_detect="peak", **kw)


def test_entry_points_refuse_bad_arguments_without_a_gpu(mta):
    """onset_logits == NULL or peak_reach outside 1..8: MT_EINVAL before anything is launched or written (there is no GPU here, and the
    dummy pointers are host memory that holds the same zeros afterwards)."""
    from music_transcription_amd import _lib
    lib = _lib.lib
    buf = np.zeros(64, np.int64)
    one = buf.ctypes.data
    for on, reach in ((None, 1), (one, 0), (one, 9), (one, -1)):
        for off in (None, one):
            assert lib.mt_note_match_counts_peak(one, on, off, 0.5, 0.5, 0.5, one, None, one, 1, 88, 8, 1, 0, reach, None) == -1
            assert "peak_reach" in _lib.last_error() and "mt_note_match_counts_peak" in _lib.last_error()
            assert lib.mt_note_match_list_peak(one, on, off, 0.5, 0.5, 0.5, one, one, one, None, one, 1, 88, 8, 1, 0, reach, None) == -1
            assert "mt_note_match_list_peak" in _lib.last_error()
            assert lib.mt_heads_to_notes_peak(one, on, off, 0.5, 0.5, 0.5, 1, 88, 8, one, one, one, 16, 1, 0, reach, None) == -1
            assert "mt_heads_to_notes_peak" in _lib.last_error()
        assert lib.mt_notes_batch_peak(one, on, 0.5, 0.5, None, 1, 88, 8, one, one, one, one, 16, 1, 0, reach, None) == -1
        assert "mt_notes_batch_peak" in _lib.last_error()
    # the cleanup's own range is still checked, as in the _clean namesakes
    assert lib.mt_note_match_counts_peak(one, one, None, 0.5, 0.5, 0.5, one, None, one, 1, 88, 8, 65, 0, 1, None) == -1
    assert lib.mt_notes_batch_peak(one, one, 0.5, 0.5, None, 1, 88, 8, one, one, one, one, 16, 1, 64, 1, None) == -1
    assert not buf.any()


def _run(script, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args", [["--onset_detect", "peak"], ["--onset_detect", "peak", "--note_metrics"],
                                  ["--onset_detect", "peak", "--note_metrics", "--decoder", "frame"],
                                  ["--peak_reach", "2", "--note_metrics"],
                                  ["--onset_detect", "peak", "--note_metrics", "--decoder", "onset", "--tune_threshold"],
                                  ["--onset_detect", "peak", "--note_metrics", "--decoder", "onset", "--tune_note_thresholds"],
                                  ["--onset_detect", "peak", "--note_metrics", "--decoder", "onset_offset", "--tune_note_decoder"],
                                  ["--onset_detect", "peak", "--note_metrics", "--decoder", "onset", "--peak_reach", "9"],
                                  ["--onset_detect", "peak", "--note_metrics", "--decoder", "onset", "--peak_reach", "0"]])
def test_evaluate_script_refuses(args):
    r = _run("scripts/evaluate.py", "--model", "none.pth", *args)
    assert r.returncode == 2 and ("--onset_detect" in r.stderr or "--peak_reach" in r.stderr), r.stderr


@pytest.mark.parametrize("script,args", [("main.py", ["a.wav", "m.pth", "--onset-detect", "peak"]),
                                         ("main.py", ["a.wav", "m.pth", "--decoder", "onset", "--onset-detect", "peak", "--peak-reach", "9"]),
                                         ("main.py", ["a.wav", "m.pth", "--peak-reach", "2"]),
                                         ("scripts/transcribe_corpus.py", ["--onset-detect", "peak"]),
                                         ("scripts/transcribe_corpus.py", ["--decoder", "onset", "--onset-detect", "peak", "--peak-reach", "0"])])
def test_transcription_scripts_refuse(script, args):
    r = _run(script, *args)
    assert r.returncode == 2 and ("onset_detect='peak' needs decoder" in r.stderr or "peak_reach" in r.stderr), r.stderr


def test_scripts_document_the_flags():
    for script, flag in (("main.py", "--onset-detect"), ("scripts/transcribe_corpus.py", "--peak-reach"), ("scripts/evaluate.py", "--onset_detect")):
        assert flag in _run(script, "--help").stdout, script
