"""Frame smoothing in the corpus paths, without a GPU: the command line's flags and early refusals, the refusals of the two corpus
functions before they touch the model or the data, the header's new exports, and the segment arithmetic of the split kernel
(csrc/smooth.hip, DESIGN.md 6c "Long rows: segments per wave") restated and checked for coverage."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "transcribe_corpus.py")


def _run(*args):
    return subprocess.run([sys.executable, SCRIPT, *args], capture_output=True, text=True, cwd=ROOT, timeout=300)


def test_help_lists_both_flags():
    r = _run("--help")
    assert r.returncode == 0 and "--smooth-on" in r.stdout and "--smooth-off" in r.stdout


def test_bad_penalties_exit_2_before_any_checkpoint_is_opened():
    """argparse's error exit; neither the directory nor the checkpoint exists, so anything later would have complained about them."""
    for flag, value in (("--smooth-on", "64.5"), ("--smooth-off", "-1"), ("--smooth-on", "-0.001"), ("--smooth-off", "nan"), ("--smooth-on", "1e9")):
        for more in ((), ("--overlap", "2"), ("--decoder", "onset", "--min-note-ms", "64")):
            r = _run("--wav-dir", "none", "--model", "none.pth", flag, value, *more)
            assert r.returncode == 2 and flag[2:].replace("-", "_") in r.stderr and "penalty" in r.stderr, (flag, value, r.stderr[-500:])
            assert "none.pth" not in r.stderr and "Traceback" not in r.stderr


def test_corpus_functions_refuse_bad_penalties_before_any_work():
    from music_transcription_amd import corpus
    model = types.SimpleNamespace(model=None)

    def never(*a, **k):
        raise AssertionError("the refusal comes before any audio is asked for")
    for kw in (dict(smooth_on=-1.0), dict(smooth_off=64.5), dict(smooth_on=float("nan")), dict(smooth_off="1"), dict(smooth_on=True)):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=name + " must be a penalty"):
            corpus.transcribe_shard(model, [0], never, n_mels=32, device="cuda", reference_roll_of=never, midi_path_of=never, **kw)
        with pytest.raises(ValueError, match=name + " must be a penalty"):
            corpus.transcribe_shard_windows(model, [0], never, overlap_s=1.0, n_mels=32, device="cuda", reference_roll_of=never,
                                            midi_path_of=never, **kw)


def test_header_declares_the_split_exports():
    hdr = open(os.path.join(ROOT, "include", "mt_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    one = re.search(r"int\s+mt_frame_smooth_split\(([^;]*)\);", hdr)
    two = re.search(r"int\s+mt_frame_smooth_chunks_split\(([^;]*)\);", hdr)
    assert one and two
    assert re.search(r"long long T,\s*int waves,\s*mt_stream_t stream", one.group(1)) and "const long long* lengths" in one.group(1)
    assert re.search(r"int T,\s*int waves,\s*mt_stream_t stream", two.group(1)) and "lengths" not in two.group(1)
    from music_transcription_amd import _lib
    assert {"mt_frame_smooth_split", "mt_frame_smooth_chunks_split"} <= set(_lib.EXPORTS)


def segments(L, waves):
    """The split kernel's cut of a row of L frames: per wave the half-open range of frames it owns."""
    W = -(-L // 64)
    seg = -(-W // waves)
    return seg, [(min(L, min(W, s * seg) * 64), min(L, min(W, (s + 1) * seg) * 64)) for s in range(waves)]


def test_segments_own_every_window_exactly_once():
    rng = np.random.default_rng(31)
    cases = [(0, 2), (1, 16), (64, 2), (65, 2), (130, 16), (1024, 16), (1025, 16), (4200, 5), (120064, 16)]
    cases += [(int(rng.integers(0, 200000)), int(rng.integers(2, 17))) for _ in range(200)]
    for L, S in cases:
        W = -(-L // 64)
        seg, cut = segments(L, S)
        assert seg * S >= W and (seg - 1) * S < W or W == 0 and seg == 0                 # the smallest seg that covers the row
        owner = np.zeros(W, int)
        for lo, end in cut:
            assert (lo % 64 == 0 or lo == end == L) and 0 <= lo <= end <= L and end - lo <= seg * 64
            if end > lo:
                owner[lo // 64:-(-end // 64)] += 1
        assert (owner == 1).all(), (L, S)
        assert [lo for lo, end in cut if end > lo] == sorted(lo for lo, end in cut if end > lo)     # in order, wave by wave
        assert sum(end - lo for lo, end in cut) == L
        empty = [s for s, (lo, end) in enumerate(cut) if lo == end]
        used = -(-W // seg) if seg else 0
        assert empty == list(range(used, S)), (L, S)                                     # the empty segments are the last ones
        if L:
            assert cut[used - 1][1] == L                                                 # and the row's last frame lies in the last used one
    assert sum(1 for lo, end in segments(130, 16)[1] if lo == end) == 13
