"""The note threshold search without a GPU: the coarse-to-fine schedule of evaluate.search_note_thresholds on analytic surfaces,
the argument checks of mt_note_sweep_counts / mt_note_sweep_list (refused before any device call), and the sweep kernels'
scratch use as the compiler reports it."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "music-transcription_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


# ------------------------------------------------------------------ the search
PEAK = (0.37, 0.62)


def _peak(fts, ots):
    f = np.asarray(fts)[:, None]
    o = np.full((1, 1), PEAK[1]) if ots is None else np.asarray(ots)[None, :]
    return 1.0 - (f - PEAK[0]) ** 2 - (o - PEAK[1]) ** 2


def _recorded(surface):
    calls = []

    def f(fts, ots):
        calls.append((np.array(fts), None if ots is None else np.array(ots)))
        return surface(fts, ots)
    return f, calls


def _schedule(surface, two_axes, tune_range=(0.05, 0.95), step=0.1, min_step=0.01, rounds=6):
    """The stated schedule, written out on its own: the grids of every round and the final best."""
    lo = [tune_range[0], tune_range[0]]
    hi = [tune_range[1], tune_range[1]]
    best, best_v = [0.5, 0.5], -1.0
    grids = []
    for _ in range(rounds):
        g = [np.arange(lo[a], hi[a] + step / 2, step) for a in range(2 if two_axes else 1)]
        grids.append(g)
        v = np.asarray(surface(g[0], g[1] if two_axes else None))
        for i in range(len(g[0])):                                           # frame-threshold-major, then onset
            for j in range(v.shape[1]):
                if v[i, j] > best_v:
                    best_v = float(v[i, j])
                    best = [float(g[0][i]), float(g[1][j]) if two_axes else best[1]]
        for a in range(2):
            lo[a], hi[a] = max(0.01, best[a] - 2 * step), min(0.99, best[a] + 2 * step)
        step /= 2
        if step < min_step:
            break
    return grids, best, best_v


@pytest.mark.parametrize("two_axes", [True, False])
def test_search_lands_on_the_peak_and_visits_the_stated_grids(mta, two_axes):
    from music_transcription_amd.evaluate import search_note_thresholds
    f, calls = _recorded(_peak)
    bf, bo, bv = search_note_thresholds(f, two_axes)
    assert abs(bf - PEAK[0]) <= 0.01
    if two_axes:
        assert abs(bo - PEAK[1]) <= 0.01
    else:
        assert bo is None and all(c[1] is None for c in calls)
    grids, best, best_v = _schedule(_peak, two_axes)
    assert len(calls) == len(grids) == 4                                     # steps 0.1, 0.05, 0.025, 0.0125; 0.00625 < 0.01 stops
    for (cf, co), g in zip(calls, grids):
        np.testing.assert_array_equal(cf, g[0])
        if two_axes:
            np.testing.assert_array_equal(co, g[1])
    np.testing.assert_array_equal(calls[0][0], np.arange(0.05, 0.95 + 0.05, 0.1))
    assert len(calls[0][0]) == 10 and (not two_axes or len(calls[0][1]) == 10)
    assert bf == best[0] and bv == best_v and (not two_axes or bo == best[1])
    assert bv == float(_peak([bf], [bo] if two_axes else None)[0, 0])
    # every later window is best +- 2 steps clipped to [0.01, 0.99]
    assert calls[1][0][0] == pytest.approx(max(0.01, 0.35 - 0.2)) and calls[1][0][-1] <= min(0.99, 0.35 + 0.2) + 0.025


def test_search_keeps_the_first_of_equal_maxima(mta):
    from music_transcription_amd.evaluate import search_note_thresholds

    def two_peaks(fts, ots):
        f, o = np.asarray(fts)[:, None], np.asarray(ots)[None, :]
        a = np.isclose(f, 0.25) & np.isclose(o, 0.35)
        b = np.isclose(f, 0.55) & np.isclose(o, 0.15)
        return (a | b).astype(np.float64)
    f, calls = _recorded(two_peaks)
    bf, bo, bv = search_note_thresholds(f, True)
    assert two_peaks(calls[0][0], calls[0][1]).sum() == 2                    # both maxima are on the first grid
    assert (bf, bo, bv) == (pytest.approx(0.25), pytest.approx(0.35), 1.0)   # frame-major: (0.25, 0.35) is visited first and stays
    flat, calls = _recorded(lambda fts, ots: np.zeros((len(fts), len(ots))))
    bf, bo, bv = search_note_thresholds(flat, True)
    assert (bf, bo, bv) == (pytest.approx(0.05), pytest.approx(0.05), 0.0)   # a flat surface: the very first candidate beats -1, nothing after
    # one axis, two equal maxima
    f1, _ = _recorded(lambda fts, ots: (np.isclose(fts, 0.25) | np.isclose(fts, 0.65)).astype(np.float64)[:, None])
    assert search_note_thresholds(f1, False)[:2] == (pytest.approx(0.25), None)


def test_search_stops_by_the_step_rule(mta):
    from music_transcription_amd.evaluate import search_note_thresholds
    for kw, n in ((dict(tune_rounds=2), 2), (dict(tune_min_step=0.06), 1), (dict(tune_min_step=0.05), 2), (dict(tune_rounds=1), 1),
                  (dict(tune_step=0.2, tune_min_step=0.01), 5), (dict(tune_min_step=1e-4, tune_rounds=6), 6)):
        f, calls = _recorded(_peak)
        search_note_thresholds(f, True, **kw)
        assert len(calls) == n, (kw, len(calls))
        g, calls1 = _recorded(_peak)
        search_note_thresholds(g, False, **kw)
        assert len(calls1) == n, (kw, len(calls1))


# ------------------------------------------------------------------ the C ABI
def _code(name):
    hdr = open(os.path.join(ROOT, "include", "mt_hip.h")).read()
    return int(re.search(rf"#define {name}\s+(-?\d+)", hdr).group(1))


def test_sweep_entry_points_are_declared_and_exported(mta):
    from music_transcription_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mt_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mt_note_sweep_counts", "mt_note_sweep_list"):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert hasattr(mta, "note_sweep_counts")


def test_sweep_arguments_are_refused_without_gpu(mta):
    """Every refusal happens before the first device call, so it needs no GPU: MT_EINVAL and a message that names the entry point."""
    from music_transcription_amd import _lib
    lib = _lib.lib
    einval = _code("MT_EINVAL")
    buf = np.zeros(64, np.float32)                                           # stands for the device pointers: never dereferenced
    p = buf.ctypes.data
    arr = lambda *v: np.array(v, np.float32)
    ok16 = np.linspace(0.1, 0.9, 16).astype(np.float32)
    ok17 = np.linspace(0.1, 0.9, 17).astype(np.float32)

    def counts(frame, onset, tf, Kf, to, Ko):
        return lib.mt_note_sweep_counts(frame, onset, None if tf is None else tf.ctypes.data, Kf, None if to is None else to.ctypes.data, Ko,
                                        p, None, p, 1, 88, 10, None)

    def listed(frame, onset, tf, Kf, to, Ko):
        return lib.mt_note_sweep_list(frame, onset, None if tf is None else tf.ctypes.data, Kf, None if to is None else to.ctypes.data, Ko,
                                      p, p, p, None, p, 1, 88, 10, None)
    for call, name in ((counts, "mt_note_sweep_counts"), (listed, "mt_note_sweep_list")):
        bad = [
            ("Kf = 0", (p, p, ok16, 0, ok16, 1)),
            ("Kf = 17", (p, p, ok17, 17, ok16, 1)),
            ("Ko = 0", (p, p, ok16, 1, ok16, 0)),
            ("Ko = 17", (p, p, ok16, 1, ok17, 17)),
            ("Kf Ko = 65", (p, p, ok16, 13, ok16, 5)),
            ("Kf Ko = 256", (p, p, ok16, 16, ok16, 16)),
            ("frame threshold 0", (p, p, arr(0.5, 0.0), 2, ok16, 2)),
            ("frame threshold 1", (p, p, arr(1.0, 0.5), 2, ok16, 2)),
            ("onset threshold 0", (p, p, ok16, 2, arr(0.5, 0.0), 2)),
            ("onset threshold 1", (p, p, ok16, 2, arr(0.5, 0.3, 1.0), 3)),
            ("frame threshold NaN", (p, None, arr(np.nan), 1, None, 1)),
            ("null thr_frame", (p, p, None, 2, ok16, 2)),
            ("null thr_onset with onset logits", (p, p, ok16, 2, None, 2)),
            ("Ko = 2 without onset logits", (p, None, ok16, 2, ok16, 2)),
            ("null frame logits", (None, p, ok16, 2, ok16, 2)),
        ]
        for what, args in bad:
            assert call(*args) == einval, (name, what)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and len(msg) > len(name) + 5, (name, what, msg)
    assert lib.mt_note_sweep_list(p, None, ok16.ctypes.data, 1, None, 1, p, p, p, None, p, 1, 88, 7_000_000, None) == einval   # 320 T past 31 bits
    assert lib.mt_note_sweep_counts(p, None, ok16.ctypes.data, 1, None, 1, p, None, p, 0, 88, 10, None) == einval
    assert ctypes.sizeof(ctypes.c_float) == 4


# ------------------------------------------------------------------ the kernels' scratch
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sweep_kernels_use_no_scratch(tmp_path):
    """A pair's matcher state is parked in LDS between slabs and lives in registers inside one: nothing of it may end up in scratch
    (private_seg_size 0 in the compiler's metadata, for the roll and the list variant)."""
    out = tmp_path / "notes.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    os.path.join(CSRC, "notes.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (\S+)\.private_seg_size, (\d+)", out.read_text())}
    sweep = [k for k in scratch if "note_sweep_kernel" in k]
    assert len(sweep) == 2, sorted(scratch)
    for k in sweep:
        assert scratch[k] == 0, (k, scratch[k])
