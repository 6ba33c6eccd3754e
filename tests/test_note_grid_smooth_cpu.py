"""Frame smoothing in the decoder grid without a GPU (DESIGN.md 6c "Smoothing in the decoder grid"): the index arithmetic of the tuner's
discrete axis cleanups x smoothings, the refusals of evaluate.tune_note_decoder(smoothings=...), of the other two tuners and of
mt_frame_smooth_paths / mt_note_grid_*_paths (all before any device call), the declarations, the command line of
scripts/evaluate.py --tune_smooth_on / --tune_smooth_off, and the batch of note_grid_smooth_case.py on the specification."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_smooth_ref as FR  # noqa: E402
import note_grid_case as GC  # noqa: E402
from note_grid_smooth_case import BLIP_SMOOTHINGS, blip_case, f1_of  # noqa: E402


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    return m


def test_discrete_axis_is_cleanup_major(mta):
    from music_transcription_amd import evaluate as E
    cleanups, smoothings = [(1, 0), (3, 2), (2, 0)], [(0.0, 0.0), (1.0, 0.5)]
    order = [E.decoder_candidate(d, cleanups, smoothings) for d in range(6)]
    assert order == [(c, s) for c in cleanups for s in smoothings]
    for d in (-1, 6):
        with pytest.raises(ValueError):
            E.decoder_candidate(d, cleanups, smoothings)
    n, Kf, Ks, Ko, Kk, Kc = 2, 3, 2, 2, 1, 3
    f1 = np.arange(n * Kf * Ks * Ko * Kk * Kc, dtype=np.float64).reshape(n, Kf, Ks, Ko, Kk, Kc)       # as note_grid_counts orders the cells
    folded = E.fold_smoothings(f1)
    assert folded.shape == (n, Kf, Ko, Kk, Kc * Ks)
    for idx in np.ndindex(n, Kf, Ko, Kk, Kc * Ks):
        c, s = divmod(idx[4], Ks)
        assert folded[idx] == f1[idx[0], idx[1], s, idx[2], idx[3], c]
        assert E.decoder_candidate(idx[4], cleanups, smoothings) == (cleanups[c], smoothings[s])

    # and a search over the folded array lands on the cell that was raised, whichever it is
    for peak in ((1, 0, 0, 2, 1), (2, 1, 0, 0, 0)):
        def mean_f1(fts, ots, kts, peak=peak):
            v = np.zeros((1, len(fts), Ks, len(ots), 1, Kc))
            v[0, peak[0], peak[4], peak[1], 0, peak[3]] = 1.0
            return E.fold_smoothings(v)[0]
        thr, othr, _, d, best = E.search_note_decoder(mean_f1, 2, Kc * Ks, tune_range=(0.3, 0.7), tune_step=0.2, tune_rounds=1)
        assert best == 1.0 and E.decoder_candidate(d, cleanups, smoothings) == (cleanups[peak[3]], smoothings[peak[4]])
        assert (thr, othr) == (pytest.approx(0.3 + 0.2 * peak[0]), pytest.approx(0.3 + 0.2 * peak[1]))


def test_refusals_of_the_tuners(mta):
    from music_transcription_amd import evaluate as E

    def never(*a, **k):
        raise AssertionError("the refusal comes first")
    with pytest.raises(ValueError, match="tune_note_decoder: smooth_on / smooth_off cannot be combined with smoothings"):
        E.tune_note_decoder(never, never, log=None, smooth_on=1.0, smoothings=[(0, 0), (1, 1)])
    with pytest.raises(ValueError, match="cannot be combined with smoothings"):
        E.tune_note_decoder(never, never, log=None, smooth_off=0.5, smoothings=[(0, 0)])
    with pytest.raises(ValueError, match="smoothings: expected a non-empty list"):
        E.tune_note_decoder(never, never, log=None, smoothings=[])
    for bad in ([(65.0, 0.0)], [(0.0, -1e-3)], [(float("nan"), 0.0)], [(1.0, "1")], [(True, 0.0)]):
        with pytest.raises(ValueError, match="smooth_on|smooth_off"):
            E.tune_note_decoder(never, never, log=None, smoothings=bad)
    for bad in ([(1.0,)], [(1.0, 1.0, 1.0)], 3, [1.0, 2.0]):
        with pytest.raises(ValueError, match="smoothings"):
            E.tune_note_decoder(never, never, log=None, smoothings=bad)
    with pytest.raises(ValueError, match="tune_note_decoder: the tuners do not smooth"):        # without candidates: as ever
        E.tune_note_decoder(never, never, log=None, smooth_on=1.0)
    for tuner in (E.tune_threshold, E.tune_note_thresholds):
        with pytest.raises(ValueError, match=f"{tuner.__name__}: the tuners do not smooth"):
            tuner(never, never, log=None, smooth_on=1.0, smooth_off=1.0)
        with pytest.raises(TypeError):
            tuner(never, never, log=None, smoothings=[(1.0, 1.0)])


def _code(name):
    hdr = open(os.path.join(ROOT, "include", "mt_hip.h")).read()
    return int(re.search(rf"#define {name}\s+(-?\d+)", hdr).group(1))


def test_entry_points_are_declared_and_exported(mta):
    from music_transcription_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mt_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mt_frame_smooth_paths", "mt_note_grid_counts_paths", "mt_note_grid_list_paths"):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert callable(mta.smooth_frame_paths) and callable(mta.smooth_frame_logits)


def test_arguments_are_refused_without_gpu(mta):
    """Every refusal happens before the first device call, so it needs no GPU: MT_EINVAL and a message that names the entry point."""
    from music_transcription_amd import _lib
    lib = _lib.lib
    einval = _code("MT_EINVAL")
    buf = np.zeros(4096, np.float32)                                         # stands for the device pointers: never dereferenced
    p, q, r = buf.ctypes.data, buf.ctypes.data + 4096, buf.ctypes.data + 8192
    ok = np.full(17, 0.5, np.float32)
    arr = lambda *v: np.array(v, np.float32)
    data = lambda a: None if a is None else a.ctypes.data

    def paths(x, thr, on, off, K, pa, wa, dims=(1, 2, 100)):
        return lib.mt_frame_smooth_paths(x, data(thr), data(on), data(off), K, None, *dims, pa, wa, None)
    bad = [("K = 0", (p, ok, ok, ok, 0, q, r)), ("K = 17", (p, ok, ok, ok, 17, q, r)), ("threshold 0", (p, arr(0.5, 0.0), ok, ok, 2, q, r)),
           ("threshold 1", (p, arr(1.0), ok, ok, 1, q, r)), ("threshold NaN", (p, arr(np.nan), ok, ok, 1, q, r)),
           ("on penalty -1", (p, ok, arr(0.0, -1.0), ok, 2, q, r)), ("on penalty 64.5", (p, ok, arr(64.5), ok, 1, q, r)),
           ("off penalty NaN", (p, ok, ok, arr(1.0, 2.0, np.nan), 3, q, r)), ("off penalty 1e9", (p, ok, ok, arr(1e9), 1, q, r)),
           ("null logits", (None, ok, ok, ok, 1, q, r)), ("null thr", (p, None, ok, ok, 1, q, r)), ("null on", (p, ok, None, ok, 1, q, r)),
           ("null off", (p, ok, ok, None, 1, q, r)), ("null paths", (p, ok, ok, ok, 1, None, r)), ("null work", (p, ok, ok, ok, 1, q, None)),
           ("B = 0", (p, ok, ok, ok, 1, q, r, (0, 2, 100))), ("P = -1", (p, ok, ok, ok, 1, q, r, (1, -1, 100))),
           ("T = 0", (p, ok, ok, ok, 1, q, r, (1, 2, 0))), ("B * P = 2^21", (p, ok, ok, ok, 1, q, r, (1 << 11, 1 << 10, 100))),
           ("T = 2^31 - 1", (p, ok, ok, ok, 1, q, r, (1, 2, (1 << 31) - 1))),
           ("paths is work", (p, ok, ok, ok, 1, q, q)), ("work inside paths", (p, ok, ok, ok, 2, q, q + 8)),
           ("paths inside the logits", (p, ok, ok, ok, 1, p + 8, r)), ("work inside the logits", (p, ok, ok, ok, 1, q, p + 792))]
    for what, args in bad:
        assert paths(*args) == einval, what
        msg = _lib.last_error()
        assert msg.startswith("mt_frame_smooth_paths:") and len(msg) > 30, (what, msg)
    cl = np.array([(1 + n, n) for n in range(17)], np.int32)

    def counts(pa, Kf, onset, offset, to, Ko, tk, Kk, clean, Kc, dims=(1, 88, 10)):
        return lib.mt_note_grid_counts_paths(pa, Kf, onset, offset, data(to), Ko, data(tk), Kk, data(clean), Kc, p, None, p, *dims, None)

    def listed(pa, Kf, onset, offset, to, Ko, tk, Kk, clean, Kc, dims=(1, 88, 10)):
        return lib.mt_note_grid_list_paths(pa, Kf, onset, offset, data(to), Ko, data(tk), Kk, data(clean), Kc, p, p, p, None, p, *dims, None)
    ok = np.linspace(0.1, 0.9, 17).astype(np.float32)
    for call, name in ((counts, "mt_note_grid_counts_paths"), (listed, "mt_note_grid_list_paths")):
        bad = [("null paths", (None, 1, p, p, ok, 1, ok, 1, cl, 1)), ("Kf = 0", (p, 0, p, p, ok, 1, ok, 1, cl, 1)),
               ("Kf = 17", (p, 17, p, p, ok, 1, ok, 1, cl, 1)), ("Ko = 17", (p, 1, p, p, ok, 17, ok, 1, cl, 1)),
               ("Kk = 0", (p, 1, p, p, ok, 1, ok, 0, cl, 1)), ("Kc = 17", (p, 1, p, p, ok, 1, ok, 1, cl, 17)),
               ("product 65", (p, 13, p, p, ok, 5, ok, 1, cl, 1)), ("product 81", (p, 3, p, p, ok, 3, ok, 3, cl, 3)),
               ("onset threshold 0", (p, 2, p, p, arr(0.5, 0.0), 2, ok, 2, cl, 2)), ("offset threshold NaN", (p, 2, p, p, ok, 2, arr(0.5, np.nan), 2, cl, 2)),
               ("offset logits without onset logits", (p, 2, None, p, None, 1, ok, 2, cl, 2)), ("Kk = 2 without offset logits", (p, 2, p, None, ok, 2, ok, 2, cl, 2)),
               ("Ko = 2 without onset logits", (p, 2, None, None, ok, 2, None, 1, cl, 2)), ("null thr_onset with onset logits", (p, 2, p, None, None, 2, None, 1, cl, 2)),
               ("null cleanups with Kc = 2", (p, 2, p, p, ok, 2, ok, 2, None, 2)), ("min_frames 65", (p, 2, p, p, ok, 2, ok, 2, np.array([(65, 0)], np.int32), 1)),
               ("bridge_frames 64", (p, 2, p, None, ok, 2, None, 1, np.array([(1, 64)], np.int32), 1)),
               ("B = 0", (p, 2, p, p, ok, 2, ok, 2, cl, 2, (0, 88, 10))), ("T = 0", (p, 2, p, p, ok, 2, ok, 2, cl, 2, (1, 88, 0))),
               ("T = 2^30", (p, 2, p, p, ok, 2, ok, 2, cl, 2, (1, 88, 1 << 30)))]
        for what, args in bad:
            assert call(*args) == einval, (name, what)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and len(msg) > len(name) + 5, (name, what, msg)
    assert listed(p, 1, None, None, None, 1, None, 1, None, 1, (1, 88, 7_000_000)) == einval               # 320 T past 31 bits
    assert _lib.last_error().startswith("mt_note_grid_list_paths:")


# ------------------------------------------------------------------ the command line
def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), *args], capture_output=True, text=True, timeout=300)


def test_command_line_of_the_smoothing_candidates():
    r = _run("--help")
    assert r.returncode == 0
    for flag in ("--tune_smooth_on", "--tune_smooth_off"):
        assert flag in r.stdout, flag
    for flags in (("--tune_smooth_on", "1"), ("--tune_smooth_off", "0", "2")):
        r = _run("--model", "none.pth", "--note_metrics", *flags)
        assert r.returncode == 2 and "--tune_note_decoder" in r.stderr and "--tune_smooth_on / --tune_smooth_off" in r.stderr, r.stderr
    base = ("--model", "none.pth", "--note_metrics", "--tune_note_decoder")
    r = _run(*base, "--tune_smooth_on", "1", "--tune_smooth_off", "0", "64.5")
    assert r.returncode == 2 and "smooth_off" in r.stderr, r.stderr
    r = _run(*base, "--tune_smooth_on", "0", "1", "--tune_smooth_off", "0", "1")                            # accepted: fails on the checkpoint
    assert r.returncode == 1 and "not found" in r.stdout, (r.stdout, r.stderr)


# ------------------------------------------------------------------ the batch on which smoothing pays, on the specification
def test_blip_case_on_the_specification():
    case = blip_case()
    assert case.blips > 500 and int((np.diff(case.ref, axis=-1) > 0).sum()) > 200
    f1 = {}
    for thr in (0.3, 0.5, 0.7):
        per = []
        for smooth in BLIP_SMOOTHINGS:
            act = lambda head, t, s=smooth: FR.smooth_ref(case.frame, t, *s) > 0
            per.append(GC.cpu_counts(case, "roll", "frame", [thr], None, None, [(1, 0)], None, act=act)[:, 0, 0, 0, 0])
        f1[thr] = f1_of(np.stack(per, axis=1))
    assert f1[0.5][1] == 1.0 and f1[0.5][0] < 0.8, f1                       # every blip is a false note until the path has to pay for it
    assert f1[0.3][0] < 0.8 < f1[0.3][1] < 1.0, f1                          # (what the search of the GPU test meets first, and then leaves)
    assert f1[0.7][0] == 1.0                                                # sigmoid(0.5) = 0.62: the blips are below this threshold, which comes last
    assert np.array_equal(FR.smooth_ref(case.frame, 0.5, 2.0, 2.0) > 0, case.ref > 0)
