"""CPU tests of the overlapping-window plan (windows.plan_windows): every frame of the recording's grid is owned by exactly one
window, and only by an interior frame of it."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP, W, TW = 512, 480000, 938
OVERLAPS = [0.256, 0.5, 2.0, 7.3, 15.0]


@pytest.fixture(scope="module")
def win():
    from music_transcription_amd import windows
    return windows


def _lengths():
    ns = set(range(1, 4000, 97)) | set(range(0, 3 * W + 20 * HOP, 1543))
    for c in (W, 2 * W, 3 * W, W + 937 * HOP // 2):
        ns |= {c + d for d in (-257, -256, -255, -1, 0, 1, 255, 256, 257, 511, 512, 513)}
    ns |= {1, 2, 511, 512, 513}
    return sorted(n for n in ns if n >= 1)


@pytest.mark.parametrize("overlap", OVERLAPS)
def test_plan_tiles_the_grid_with_interior_frames(win, overlap):
    for n in _lengths():
        p = win.plan_windows(n, overlap)
        O = int(round(overlap * 16000 / HOP))
        assert (p.Tw, p.Tg, p.O, p.S) == (TW, 1 + n // HOP, O, TW - O)
        K = len(p.start)
        L = max(0, math.ceil((n - W) / HOP))
        assert K == math.ceil(L / p.S) + 1 and p.start[-1] == L, (n, overlap)
        assert np.all(np.diff(p.start) > 0) and p.start[0] == 0
        # starts are frames of the hop grid: window k reads samples from HOP * start[k]
        if n > W:
            end = HOP * int(p.start[-1]) + W
            assert n <= end < n + HOP, (n, overlap)
        else:
            assert K == 1
        # ownership tiles [0, Tg) exactly once
        owned = np.zeros(p.Tg, np.int64)
        for a, lo, hi in zip(p.start, p.lo, p.hi):
            assert 0 <= lo < hi <= TW, (n, overlap, a, lo, hi)
            owned[a + lo:a + hi] += 1
        assert np.all(owned == 1), (n, overlap)
        assert p.start[0] + p.lo[0] == 0 and p.start[-1] + p.hi[-1] == p.Tg
        # every kept frame is interior: [O // 2, Tw - ceil(O / 2)), window 0's left edge and the last window's right edge excepted
        for k, (lo, hi) in enumerate(zip(p.lo, p.hi)):
            if k > 0:
                assert lo >= O // 2, (n, overlap, k, lo)
            if k < K - 1:
                assert hi <= TW - (O + 1) // 2, (n, overlap, k, hi)


def test_one_window_up_to_30_s(win):
    for n in (0, 1, 16000, W - 1, W):
        p = win.plan_windows(n, 2.0)
        assert list(p.start) == [0] and p.lo[0] == 0 and p.hi[0] == 1 + n // HOP
    p = win.plan_windows(W + 1, 2.0)
    assert list(p.start) == [0, 1] and p.hi[-1] == 1 + (W + 1) // HOP - 1


def test_window_count_at_2_s(win):
    n = 20 * 60 * 16000
    p = win.plan_windows(n, 2.0)
    chunks = -(-n // W)
    assert chunks == 40 and len(p.start) == 43


@pytest.mark.parametrize("overlap", [0.0, 0.2, 0.23, -1.0, 15.1, 30.0, float("nan"), float("inf")])
def test_overlap_out_of_range_refused(win, overlap):
    with pytest.raises(ValueError, match=r"between 0\.256 s and 15\.008 s"):
        win.plan_windows(W * 2, overlap)
    with pytest.raises(ValueError):
        win.overlap_frames(overlap)


def test_overlap_bounds_accepted(win):
    assert win.plan_windows(W * 3, 0.25).O == 8          # round(7.8125)
    assert win.plan_windows(W * 3, 15.008).O == 469
    with pytest.raises(ValueError):
        win.plan_windows(-1, 2.0)


def test_evaluate_script_refuses_window_overlap_with_cache(tmp_path):
    import pickle
    import subprocess
    cache = tmp_path / "cache"
    cache.mkdir()
    with open(cache / "test_metadata.pkl", "wb") as f:
        pickle.dump({"n_mels": 64, "chunks": []}, f)
    ckpt = tmp_path / "m.pth"
    ckpt.write_bytes(b"")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", str(ckpt), "--cache_dir", str(cache),
                        "--window_overlap", "2", "--headless"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--window_overlap" in r.stdout and "--data_source full" in r.stdout, r.stdout + r.stderr
