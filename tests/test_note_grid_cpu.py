"""The decoder grid without a GPU: the coarse-to-fine schedule of evaluate.search_note_decoder on analytic surfaces, the argument checks
of mt_note_grid_counts / mt_note_grid_list (refused before any device call), the declarations, the grid kernels' scratch use as the
compiler reports it, and the command line of scripts/evaluate.py --tune_note_decoder."""
import os
import re
import shutil
import subprocess
import sys

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
PEAK = (0.37, 0.62, 0.21)
CLEAN_BONUS = (0.0, 0.02, 0.05, 0.01)                                        # of four cleanup candidates the third is best


def _surface(n_clean):
    def f(fts, ots, kts):
        axes = [np.full(1, PEAK[a]) if t is None else np.asarray(t) for a, t in enumerate((fts, ots, kts))]
        d = sum((axes[a].reshape([-1 if b == a else 1 for b in range(3)]) - PEAK[a]) ** 2 for a in range(3))
        return (1.0 - d)[..., None] + np.asarray(CLEAN_BONUS[:n_clean])
    return f


def _recorded(surface):
    calls = []

    def f(fts, ots, kts):
        calls.append(tuple(None if t is None else np.array(t) for t in (fts, ots, kts)))
        return surface(fts, ots, kts)
    return f, calls


def _schedule(surface, n_axes, n_clean, tune_range=(0.05, 0.95), step=0.1, min_step=0.01, rounds=6):
    """The stated schedule, written out on its own: the grids of every round and the final best."""
    lo, hi = [tune_range[0]] * 3, [tune_range[1]] * 3
    best, best_c, best_v = [0.5] * 3, 0, -1.0
    grids = []
    for _ in range(rounds):
        g = [np.arange(lo[a], hi[a] + step / 2, step) if a < n_axes else None for a in range(3)]
        grids.append(g)
        v = np.asarray(surface(*g))
        for i in range(v.shape[0]):                                          # frame-major, then onset, then offset, then cleanup
            for j in range(v.shape[1]):
                for k in range(v.shape[2]):
                    for c in range(n_clean):
                        if v[i, j, k, c] > best_v:
                            best_v, best_c = float(v[i, j, k, c]), c
                            for a, n in enumerate((i, j, k)):
                                if a < n_axes:
                                    best[a] = float(g[a][n])
        for a in range(3):
            lo[a], hi[a] = max(0.01, best[a] - 2 * step), min(0.99, best[a] + 2 * step)
        step /= 2
        if step < min_step:
            break
    return grids, best, best_c, best_v


@pytest.mark.parametrize("n_clean", [1, 4])
@pytest.mark.parametrize("n_axes", [1, 2, 3])
def test_search_lands_on_the_peak_and_visits_the_stated_grids(mta, n_axes, n_clean):
    from music_transcription_amd.evaluate import search_note_decoder
    f, calls = _recorded(_surface(n_clean))
    got = search_note_decoder(f, n_axes, n_clean)
    thr, c, v = got[:3], got[3], got[4]
    for a in range(3):
        if a < n_axes:
            assert abs(thr[a] - PEAK[a]) <= 0.01
        else:
            assert thr[a] is None and all(call[a] is None for call in calls)
    assert c == (2 if n_clean == 4 else 0)
    grids, best, best_c, best_v = _schedule(_surface(n_clean), n_axes, n_clean)
    assert len(calls) == len(grids) == 4                                     # steps 0.1, 0.05, 0.025, 0.0125; 0.00625 < 0.01 stops
    for call, g in zip(calls, grids):
        for a in range(n_axes):
            np.testing.assert_array_equal(call[a], g[a])
    np.testing.assert_array_equal(calls[0][0], np.arange(0.05, 0.95 + 0.05, 0.1))
    assert all(len(calls[0][a]) == 10 for a in range(n_axes))
    assert list(thr[:n_axes]) == best[:n_axes] and c == best_c and v == best_v
    # every later window is best +- 2 steps clipped to [0.01, 0.99]
    assert calls[1][0][0] == pytest.approx(max(0.01, 0.35 - 0.2)) and calls[1][0][-1] <= min(0.99, 0.35 + 0.2) + 0.025


def test_search_keeps_the_first_of_equal_maxima(mta):
    from music_transcription_amd.evaluate import search_note_decoder

    def peaks(fts, ots, kts):
        f, o, k = np.asarray(fts)[:, None, None, None], np.asarray(ots)[None, :, None, None], np.asarray(kts)[None, None, :, None]
        c = np.arange(3)[None, None, None, :]
        a = np.isclose(f, 0.25) & np.isclose(o, 0.35) & np.isclose(k, 0.45) & (c == 1)
        b = np.isclose(f, 0.25) & np.isclose(o, 0.35) & np.isclose(k, 0.45) & (c == 2)     # the same thresholds, a later cleanup
        d = np.isclose(f, 0.25) & np.isclose(o, 0.35) & np.isclose(k, 0.55) & (c == 0)     # a later offset threshold, an earlier cleanup
        e = np.isclose(f, 0.55) & np.isclose(o, 0.15) & np.isclose(k, 0.15) & (c == 0)     # a later frame threshold
        return (a | b | d | e).astype(np.float64)
    f, calls = _recorded(peaks)
    got = search_note_decoder(f, 3, 3)
    assert peaks(*calls[0]).sum() == 4                                       # all four maxima are on the first grid
    assert got == (pytest.approx(0.25), pytest.approx(0.35), pytest.approx(0.45), 1, 1.0)
    flat, _ = _recorded(lambda fts, ots, kts: np.zeros((len(fts), len(ots), len(kts), 2)))
    assert search_note_decoder(flat, 3, 2) == (pytest.approx(0.05), pytest.approx(0.05), pytest.approx(0.05), 0, 0.0)
    below, _ = _recorded(lambda fts, ots, kts: np.full((len(fts), 1, 1, 2), -2.0))       # nothing beats -1: the start stays
    assert search_note_decoder(below, 1, 2, tune_rounds=1) == (0.5, None, None, 0, -1.0)


def test_search_stops_by_the_step_rule(mta):
    from music_transcription_amd.evaluate import search_note_decoder
    for kw, n in ((dict(tune_rounds=2), 2), (dict(tune_min_step=0.06), 1), (dict(tune_min_step=0.05), 2), (dict(tune_rounds=1), 1),
                  (dict(tune_step=0.2, tune_min_step=0.01), 5), (dict(tune_min_step=1e-4, tune_rounds=6), 6)):
        for n_axes in (1, 3):
            f, calls = _recorded(_surface(2))
            search_note_decoder(f, n_axes, 2, **kw)
            assert len(calls) == n, (kw, n_axes, len(calls))
    with pytest.raises(ValueError):
        search_note_decoder(_surface(1), 4, 1)
    with pytest.raises(ValueError):
        search_note_decoder(_surface(1), 1, 0)


# ------------------------------------------------------------------ the C ABI
def _code(name):
    hdr = open(os.path.join(ROOT, "include", "mt_hip.h")).read()
    return int(re.search(rf"#define {name}\s+(-?\d+)", hdr).group(1))


def test_grid_entry_points_are_declared_and_exported(mta):
    from music_transcription_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mt_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mt_note_grid_counts", "mt_note_grid_list"):
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert hasattr(mta, "note_grid_counts")
    from music_transcription_amd import evaluate
    assert callable(evaluate.search_note_decoder) and callable(evaluate.tune_note_decoder)


def test_grid_arguments_are_refused_without_gpu(mta):
    """Every refusal happens before the first device call, so it needs no GPU: MT_EINVAL and a message that names the entry point."""
    from music_transcription_amd import _lib
    lib = _lib.lib
    einval = _code("MT_EINVAL")
    buf = np.zeros(64, np.float32)                                           # stands for the device pointers: never dereferenced
    p = buf.ctypes.data
    arr = lambda *v: np.array(v, np.float32)
    ok = np.linspace(0.1, 0.9, 17).astype(np.float32)
    cl = lambda *pairs: np.array(pairs, np.int32).reshape(-1, 2)
    ok_cl = cl(*[(1 + n, n) for n in range(17)])
    data = lambda a: None if a is None else a.ctypes.data

    def counts(frame, onset, offset, tf, Kf, to, Ko, tk, Kk, clean, Kc, dims=(1, 88, 10)):
        return lib.mt_note_grid_counts(frame, onset, offset, data(tf), Kf, data(to), Ko, data(tk), Kk, data(clean), Kc, p, None, p, *dims, None)

    def listed(frame, onset, offset, tf, Kf, to, Ko, tk, Kk, clean, Kc, dims=(1, 88, 10)):
        return lib.mt_note_grid_list(frame, onset, offset, data(tf), Kf, data(to), Ko, data(tk), Kk, data(clean), Kc, p, p, p, None, p, *dims, None)
    for call, name in ((counts, "mt_note_grid_counts"), (listed, "mt_note_grid_list")):
        bad = [
            ("Kf = 0", (p, p, p, ok, 0, ok, 1, ok, 1, ok_cl, 1)),
            ("Kf = 17", (p, p, p, ok, 17, ok, 1, ok, 1, ok_cl, 1)),
            ("Ko = 0", (p, p, p, ok, 1, ok, 0, ok, 1, ok_cl, 1)),
            ("Ko = 17", (p, p, p, ok, 1, ok, 17, ok, 1, ok_cl, 1)),
            ("Kk = 0", (p, p, p, ok, 1, ok, 1, ok, 0, ok_cl, 1)),
            ("Kk = 17", (p, p, p, ok, 1, ok, 1, ok, 17, ok_cl, 1)),
            ("Kc = 0", (p, p, p, ok, 1, ok, 1, ok, 1, ok_cl, 0)),
            ("Kc = 17", (p, p, p, ok, 1, ok, 1, ok, 1, ok_cl, 17)),
            ("product 65", (p, p, p, ok, 13, ok, 5, ok, 1, ok_cl, 1)),
            ("product 65 over four axes", (p, p, p, ok, 13, ok, 1, ok, 1, ok_cl, 5)),
            ("product 81", (p, p, p, ok, 3, ok, 3, ok, 3, ok_cl, 3)),
            ("frame threshold 0", (p, p, p, arr(0.5, 0.0), 2, ok, 2, ok, 2, ok_cl, 2)),
            ("frame threshold 1", (p, p, p, arr(1.0, 0.5), 2, ok, 2, ok, 2, ok_cl, 2)),
            ("frame threshold NaN", (p, None, None, arr(np.nan), 1, None, 1, None, 1, None, 1)),
            ("onset threshold 0", (p, p, p, ok, 2, arr(0.5, 0.0), 2, ok, 2, ok_cl, 2)),
            ("onset threshold 1", (p, p, None, ok, 2, arr(0.5, 0.3, 1.0), 3, None, 1, ok_cl, 2)),
            ("onset threshold NaN", (p, p, None, ok, 2, arr(np.nan), 1, None, 1, ok_cl, 2)),
            ("offset threshold 0", (p, p, p, ok, 2, ok, 2, arr(0.0, 0.5), 2, ok_cl, 2)),
            ("offset threshold 1", (p, p, p, ok, 2, ok, 2, arr(0.5, 1.0), 2, ok_cl, 2)),
            ("offset threshold NaN", (p, p, p, ok, 2, ok, 2, arr(0.5, np.nan), 2, ok_cl, 2)),
            ("offset logits without onset logits", (p, None, p, ok, 2, None, 1, ok, 2, ok_cl, 2)),
            ("Kk = 2 without offset logits", (p, p, None, ok, 2, ok, 2, ok, 2, ok_cl, 2)),
            ("Ko = 2 without onset logits", (p, None, None, ok, 2, ok, 2, None, 1, ok_cl, 2)),
            ("null thr_frame", (p, p, p, None, 2, ok, 2, ok, 2, ok_cl, 2)),
            ("null thr_onset with onset logits", (p, p, None, ok, 2, None, 2, None, 1, ok_cl, 2)),
            ("null thr_offset with offset logits", (p, p, p, ok, 2, ok, 2, None, 2, ok_cl, 2)),
            ("null cleanups with Kc = 2", (p, p, p, ok, 2, ok, 2, ok, 2, None, 2)),
            ("min_frames 0", (p, p, p, ok, 2, ok, 2, ok, 2, cl((1, 0), (0, 0)), 2)),
            ("min_frames 65", (p, p, p, ok, 2, ok, 2, ok, 2, cl((65, 0)), 1)),
            ("bridge_frames -1", (p, None, None, ok, 2, None, 1, None, 1, cl((1, -1)), 1)),
            ("bridge_frames 64", (p, p, None, ok, 2, ok, 2, None, 1, cl((1, 0), (2, 2), (1, 64)), 3)),
            ("null frame logits", (None, p, p, ok, 2, ok, 2, ok, 2, ok_cl, 2)),
            ("B = 0", (p, p, p, ok, 2, ok, 2, ok, 2, ok_cl, 2, (0, 88, 10))),
            ("T = 0", (p, p, p, ok, 2, ok, 2, ok, 2, ok_cl, 2, (1, 88, 0))),
            ("T = 2^30", (p, p, p, ok, 2, ok, 2, ok, 2, ok_cl, 2, (1, 88, 1 << 30))),
        ]
        for what, args in bad:
            assert call(*args) == einval, (name, what)
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and len(msg) > len(name) + 5, (name, what, msg)
    assert listed(p, None, None, ok, 1, None, 1, None, 1, None, 1, (1, 88, 7_000_000)) == einval       # 320 T past 31 bits
    assert _lib.last_error().startswith("mt_note_grid_list:")
    assert lib.mt_note_grid_counts(p, p, p, ok.ctypes.data, 2, ok.ctypes.data, 2, ok.ctypes.data, 2, ok_cl.ctypes.data, 2, None, None, p, 1, 88, 10,
                                   None) == einval                                                    # null reference
    assert lib.mt_note_grid_list(p, p, p, ok.ctypes.data, 2, ok.ctypes.data, 2, ok.ctypes.data, 2, ok_cl.ctypes.data, 2, p, p, None, None, p, 1, 88,
                                 10, None) == einval


# ------------------------------------------------------------------ the kernels' scratch
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_grid_kernels_use_no_scratch(tmp_path):
    """A configuration's state -- matcher and cleanup pipeline -- is parked in LDS between slabs and lives in registers inside one:
    nothing of it may end up in scratch (private_seg_size 0 in the compiler's metadata, for the roll and the list variant with and
    without the offset head), and the threshold sweep's two kernels are still there."""
    out = tmp_path / "notes.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    os.path.join(CSRC, "notes.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (\S+)\.private_seg_size, (\d+)", out.read_text())}
    grid = [k for k in scratch if "note_grid_kernel" in k]
    assert len(grid) == 4, sorted(scratch)
    for k in grid:
        assert scratch[k] == 0, (k, scratch[k])
    assert len([k for k in scratch if "note_sweep_kernel" in k]) == 2, sorted(scratch)


# ------------------------------------------------------------------ the command line
def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), *args], capture_output=True, text=True, timeout=300)


def test_command_line_of_the_decoder_tuner():
    r = _run("--help")
    assert r.returncode == 0
    for flag in ("--tune_note_decoder", "--tune_min_note_ms", "--tune_bridge_gap_ms"):
        assert flag in r.stdout, flag
    base = ("--model", "none.pth", "--note_metrics", "--tune_note_decoder")
    for extra, word in ((("--tune_note_thresholds",), "--tune_note_thresholds"), (("--min_note_ms", "64"), "--min_note_ms"),
                        (("--bridge_gap_ms", "32"), "--bridge_gap_ms")):
        r = _run(*base, *extra)
        assert r.returncode == 2 and "--tune_note_decoder" in r.stderr and word in r.stderr, (extra, r.stderr)
    r = _run("--model", "none.pth", "--note_metrics", "--tune_min_note_ms", "32")
    assert r.returncode == 2 and "--tune_note_decoder" in r.stderr, r.stderr
    r = _run(*base, "--tune_min_note_ms", "4096")
    assert r.returncode == 2 and "min_note_ms" in r.stderr, r.stderr
