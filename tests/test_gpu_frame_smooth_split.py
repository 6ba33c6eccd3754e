"""Frame smoothing with several waves per row (csrc/smooth.hip, mt_frame_smooth_split / mt_frame_smooth_chunks_split; DESIGN.md 6c "Long
rows: segments per wave") against the literal specification of frame_smooth_ref.py and against the one-wave kernel on the same input:
lengths on, one before and one after every boundary the kernel knows (window, slab, segment), rows whose carries cross whole segments
in either direction, ties and a NaN at a segment boundary, the chunk layout, in place, (0, 0), the refusals and the forced dispatch.
Integer arithmetic on quantised evidence: every comparison is array_equal on the whole output buffer, pre-filled with a sentinel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frame_smooth_ref as FR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, P, T = 2, 3, 4200                                # 66 windows: five slabs of 16, the last one short
THRESHOLDS = (0.3, 0.5, 0.8)
PENALTIES = [(0.0, 0.0), (1.0, 1.0), (1.5, 0.25), (64.0, 64.0)]
WAVES = (2, 3, 5, 16)
SENTINEL = -7.0
EINVAL = -1


def seg_of(L, waves):
    """Windows per segment of a row of L frames cut over `waves` waves."""
    return -(-(-(-L // 64)) // waves)


def _lengths():
    """Every L the issue names, in pairs (one per recording of the batch)."""
    ls = [63, 64, 65, 1023, 1024, 1025, 0, 1, T]
    for S in WAVES:
        edge = seg_of(T, S) * 64                     # the first segment boundary of a full row
        full = (T // 64 // S) * S * 64               # the longest L whose windows fill all S segments evenly: one more frame re-cuts them
        ls += [edge - 1, edge, edge + 1, full - 1, full, full + 1]
    ls = sorted(set(ls))
    assert all(0 <= v <= T for v in ls)
    if len(ls) % 2:
        ls.append(T)
    return [(ls[i], ls[-1 - i]) for i in range(len(ls) // 2)]


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(autouse=True)
def one_wave_twins(monkeypatch):
    """mt_frame_smooth / mt_frame_smooth_chunks are the one-wave kernel in this file, whatever the dispatch rule would pick."""
    monkeypatch.setenv("MT_SMOOTH_SPLIT", "0")


def _raw():
    from music_transcription_amd import _lib
    return _lib.lib, _lib.ptr, _lib.stream_ptr


def raw(x, thr, on, off, lengths=None, waves=None, out=None, chunks=False):
    """The C entry point for (chunks, waves) called directly -> rc, out (sentinels wherever the kernel writes nothing)."""
    lib, ptr, stream = _raw()
    n0, Pn, Tn = x.shape
    out = torch.full_like(x, SENTINEL) if out is None else out
    more = () if waves is None else (waves,)
    if chunks:
        fn = lib.mt_frame_smooth_chunks if waves is None else lib.mt_frame_smooth_chunks_split
        rc = fn(ptr(x), ptr(out), thr, on, off, n0, Pn, Tn, *more, stream())
    else:
        ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
        fn = lib.mt_frame_smooth if waves is None else lib.mt_frame_smooth_split
        rc = fn(ptr(x), ptr(out), thr, on, off, ptr(ln), n0, Pn, Tn, *more, stream())
    torch.cuda.synchronize()
    return rc, out


def _activity(x, thr):
    from music_transcription_amd import ops
    return ops.predict_from_logits(x.contiguous().float(), thr).cpu().numpy() > 0


def _expect(x, thr, on, off, lengths=None):
    """x (B, P, T) on the device -> what a call leaves in a buffer of sentinels: the specification on the valid frames."""
    want = FR.smooth_ref(x.cpu().numpy(), thr, on, off, lengths, _activity(x, thr))
    if lengths is not None:
        for b, L in enumerate(lengths):
            want[b, :, max(0, min(L, x.shape[2])):] = SENTINEL
    return want


def _all_agree(x, thr, on, off, lengths, waves_list, what):
    """One-wave and every wave count against the specification -> the expected buffer."""
    want = _expect(x, thr, on, off, lengths)
    rc, one = raw(x, thr, on, off, lengths)
    assert rc == 0 and np.array_equal(one.cpu().numpy(), want), (what, "one wave")
    for S in waves_list:
        rc, got = raw(x, thr, on, off, lengths, waves=S)
        assert rc == 0 and np.array_equal(got.cpu().numpy(), want), (what, S)
        assert torch.equal(got, one)
    return want


_CASE = {}


def _random_case():
    """Noisy evidence around Markov runs (tests/test_gpu_frame_smooth.py's recipe); the first pitch on the 1/64 grid."""
    if not _CASE:
        from offset_decode_ref import markov
        rng = np.random.default_rng(21)
        runs = markov(rng, (B, P, T), 0.05, 0.08)
        x = (rng.normal(0, 1.0, (B, P, T)) + np.where(runs, 1.0, -1.0) * rng.choice([0.3, 1.5], (B, P, 1))).astype(np.float32)
        x[:, 0] = np.round(x[:, 0] * 64) / 64
        x[1, 1, 40], x[1, 1, 2700], x[0, 2, 64], x[0, 2, 4100] = np.inf, -np.inf, 80.0, -80.0
        _CASE.update(dev=torch.from_numpy(x).cuda())
    return _CASE


def _padded(x, lengths):
    """Frames at or past a length must never be read: +50, -50 and NaN in turn."""
    pad = torch.tensor([50.0, -50.0, float("nan")], device="cuda").repeat(T // 3 + 1)[:T]
    y = x.clone()
    for b, L in enumerate(lengths):
        y[b, :, L:] = pad[L:]
    return y


@pytest.mark.parametrize("on,off", PENALTIES)
def test_random_rows_equal_the_specification_and_the_one_wave_kernel(mta, on, off):
    x = _random_case()["dev"]
    changed = 0
    for thr in THRESHOLDS:
        for lengths in _lengths():
            want = _all_agree(_padded(x, lengths), thr, on, off, list(lengths), WAVES, (thr, lengths))
        want = _all_agree(x, thr, on, off, None, WAVES, (thr, "no lengths"))
        changed += int(((want > 0) != _activity(x, thr)).sum())
    assert (changed > 100) == ((on, off) != (0.0, 0.0))


def test_the_length_list_holds_every_boundary():
    ls = {v for pair in _lengths() for v in pair}
    assert {0, 1, 63, 64, 65, 1023, 1024, 1025, T} <= ls
    for S in WAVES:
        e = seg_of(T, S) * 64
        assert {e - 1, e, e + 1} <= ls
        full = [L for L in ls if L % 64 == 0 and L and (L // 64) % S == 0 and L + 1 in ls and L - 1 in ls]
        assert full and all(seg_of(L + 1, S) == seg_of(L, S) + 1 for L in full)
    assert (seg_of(T, 16), seg_of(T, 5), seg_of(T, 3), seg_of(T, 2)) == (5, 14, 22, 33)          # 16 waves: 66 windows, two empty segments


def test_fewer_windows_than_waves(mta):
    x = _random_case()["dev"]
    for on, off in PENALTIES[1:]:
        _all_agree(_padded(x, (130, 130)), 0.5, on, off, [130, 130], (16,), (on, off))            # 3 windows: 13 empty segments
    assert seg_of(130, 16) == 1


# ------------------------------------------------------------------------------------------------ carries across whole segments
CARRY_T, CARRY_S = 4096, 8                          # segments of 8 windows = 512 frames


def _carry_rows():
    """Penalties (2, 2): a = b = 128.  +-0.1 logits are 6 grid steps, so alternating them keeps d inside the band; +-5 is decisive on
    its own; a logit of exactly 0 at threshold 0.5 is no evidence at all."""
    wiggle = np.where(np.arange(CARRY_T) % 2 == 0, 0.1, -0.1).astype(np.float32)
    rows, names = [], []
    for sign in (1.0, -1.0):
        r = wiggle.copy()                            # backward: decided in the first segment, then nothing until frame 4000
        r[5], r[6], r[4000] = -5.0 * sign, 1.0 * sign, 5.0 * sign
        rows.append(r), names.append(f"back{sign:+.0f}")
        r = wiggle.copy() * sign                     # backward: nothing decisive above frame 5 but the row's last frame, on iff d > 0
        r[5], r[6] = -5.0 * sign, 1.0 * sign
        rows.append(r), names.append(f"last{sign:+.0f}")
        for early in (1.5, 0.0):                     # forward: decided at frame 0 (d clamps to -128), 96 steps back at frame 3 or not, six
            r = np.zeros(CARRY_T, np.float32)        # segments of zero evidence, then 166 steps: -32 + 166 crosses b = 128, -128 + 166
            r[0], r[3] = -5.0 * sign, early * sign   # does not; 64 steps against at frame 4090 then leave the row's end at +64 or -26
            r[3600], r[4090] = 2.6 * sign, -1.0 * sign
            rows.append(r), names.append(f"fwd{sign:+.0f}/{early}")
    return np.stack(rows)[:, None, :], names


def test_carries_cross_whole_segments_in_both_directions(mta):
    x, names = _carry_rows()
    dev = torch.from_numpy(x).cuda()
    want = _all_agree(dev, 0.5, 2.0, 2.0, None, (CARRY_S, 2, 16), "carry rows")
    path = {name: want[n, 0] > 0 for n, name in enumerate(names)}
    seg = seg_of(CARRY_T, CARRY_S) * 64
    assert seg == 512
    for sign, name in ((1.0, "back+1"), (-1.0, "back-1")):                   # the rows do what they are named for
        d = FR.forward_d(FR.quantise(x[names.index(name), 0], 0.5), 128, 128)
        assert (np.abs(d[7:4000]) < 128).all() and abs(d[5]) > 128 and abs(d[4000]) > 128        # six middle segments undecided throughout
        assert (path[name][7:4001] == (sign > 0)).all() and path[name][5] == (sign < 0)
    for name in ("last+1", "last-1"):
        d = FR.forward_d(FR.quantise(x[names.index(name), 0], 0.5), 128, 128)
        assert (np.abs(d[7:]) < 128).all()
        assert (path[name][7:] == (d[-1] > 0)).all()
    assert path["last+1"][-1] != path["last-1"][-1]                           # once resolving on, once off
    q = FR.quantise(x[names.index("fwd+1/1.5"), 0], 0.5)
    assert (q[seg:7 * seg] == 0).all() and q[3] == 96 and q[3600] == 166
    d = FR.forward_d(q, 128, 128)
    assert d[3599] == -32 and d[3600] == 134                                   # frame 3600 is decisive only because d_in came through
    assert not path["fwd+1/1.5"][:3].any() and path["fwd+1/1.5"][3:].all() and not path["fwd+1/0.0"].any()        # (d = -a is decisive)
    assert path["fwd-1/1.5"][0] and not path["fwd-1/1.5"][1:].any() and path["fwd-1/0.0"].all()       # and a positive d_in as well


def test_ties_at_a_segment_boundary(mta):
    L, S = 256, 2                                    # 4 windows, segments of 2: the boundary is frame 128
    assert seg_of(L, S) * 64 == 128
    x = np.full((1, 1, L), -5.0, np.float32)
    x[0, 0, 127:129] = 1.0                           # 128 grid steps of evidence, one frame on either side of the boundary
    dev = torch.from_numpy(x).cuda()
    g = 63.0 / 64.0
    for (on, off), stays in (((1.0, 1.0), False), ((g, 1.0), True), ((1.0, g), True), ((1.5, 1.5), False)):
        want = _all_agree(dev, 0.5, on, off, None, (S, 4), (on, off))
        assert (want[0, 0, 127:129] > 0).all() == stays and not (want[0, 0, :127] > 0).any() and not (want[0, 0, 129:] > 0).any()


def test_a_nan_in_a_later_segment(mta):
    L, S = 600, 4                                    # 10 windows, segments of 3: frame 400 lies in segment 2
    assert 2 * seg_of(L, S) * 64 <= 400 < 3 * seg_of(L, S) * 64
    x = torch.full((1, 1, L), 1.0, device="cuda")
    x[0, 0, 400] = float("nan")
    want = _all_agree(x, 0.5, 64.0, 64.0, None, (S,), "bridged")
    assert (want > 0).all()
    want = _all_agree(x, 0.5, 20.0, 20.0, None, (S,), "left for one frame")
    assert not want[0, 0, 400] > 0 and (np.delete(want[0, 0], 400) > 0).all()


# ------------------------------------------------------------------------------------------------ the chunk layout
def _cat(x):
    """(NB, P, T) chunks -> (1, P, NB * T): the recording they are."""
    return x.permute(1, 0, 2).reshape(1, x.shape[1], -1).contiguous()


def test_chunks_are_one_recording(mta):
    rng = np.random.default_rng(22)
    NB, Pn, Tn = 5, 2, 938                           # 4 690 frames, chunk boundaries inside windows
    x = torch.from_numpy(rng.normal(0, 1.2, (NB, Pn, Tn)).astype(np.float32)).cuda()
    for on, off in PENALTIES[1:]:
        want = _expect(_cat(x), 0.5, on, off)
        rc, one = raw(x, 0.5, on, off, chunks=True)
        assert rc == 0 and np.array_equal(_cat(one).cpu().numpy(), want)
        for S in (2, 7):
            rc, got = raw(x, 0.5, on, off, waves=S, chunks=True)
            assert rc == 0 and np.array_equal(_cat(got).cpu().numpy(), want) and torch.equal(got, one), (on, off, S)
            buf = x.clone()
            rc, _ = raw(buf, 0.5, on, off, waves=S, out=buf, chunks=True)         # in place
            assert rc == 0 and torch.equal(buf, one)


def test_in_place(mta):
    x = _random_case()["dev"]
    lengths = [3071, T]
    want = _expect(x, 0.3, 1.5, 0.25, lengths)
    for b, L in enumerate(lengths):
        want[b, :, L:] = x[b, :, L:].cpu().numpy()                               # frames past L are not written: they keep the input
    for S in WAVES:
        buf = x.clone()
        rc, same = raw(buf, 0.3, 1.5, 0.25, lengths, waves=S, out=buf)
        assert rc == 0 and same is buf and np.array_equal(buf.cpu().numpy(), want), S


def test_no_penalty_through_the_kernel_is_the_threshold(mta):
    rng = np.random.default_rng(23)
    x = rng.normal(0, 0.05, (2, 3, 1100)).astype(np.float32)                     # crowded around the thresholds' logits
    for i, thr in enumerate(THRESHOLDS):
        x[1, i] += FR.centre(thr)
    dev = torch.from_numpy(x).cuda()
    for thr in THRESHOLDS:
        act = _activity(dev, thr)
        for S in WAVES:
            rc, got = raw(dev, thr, 0.0, 0.0, waves=S)
            assert rc == 0 and np.array_equal(got.cpu().numpy() > 0, act) and (got.abs() == 64.0).all() and 0 < act.mean() < 1


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_c_abi_refusals_leave_the_output_alone(mta):
    from music_transcription_amd import _lib
    lib, ptr, stream = _raw()
    x = _random_case()["dev"]
    for waves in (0, 1, 17, -1):
        rc, got = raw(x, 0.5, 1.0, 1.0, [5, 5], waves=waves)
        assert rc == EINVAL and (got == SENTINEL).all() and "waves" in _lib.last_error(), waves
        rc, got = raw(x, 0.5, 1.0, 1.0, waves=waves, chunks=True)
        assert rc == EINVAL and (got == SENTINEL).all() and "waves" in _lib.last_error(), waves
    nan = float("nan")
    for thr, on, off in [(0.5, -0.5, 0.0), (0.5, 0.0, 64.5), (0.5, nan, 0.0), (0.5, 0.0, nan), (0.0, 1.0, 1.0), (1.0, 1.0, 1.0), (nan, 1.0, 1.0)]:
        rc, got = raw(x, thr, on, off, [5, 5], waves=4)
        assert rc == EINVAL and (got == SENTINEL).all(), (thr, on, off)
        rc, got = raw(x, thr, on, off, waves=4, chunks=True)
        assert rc == EINVAL and (got == SENTINEL).all(), (thr, on, off)
    assert "penalty" in _lib.last_error() or "threshold" in _lib.last_error()
    out = torch.full_like(x, SENTINEL)
    for xp, op in ((None, ptr(out)), (ptr(x), None)):
        assert lib.mt_frame_smooth_split(xp, op, 0.5, 1.0, 1.0, None, B, P, T, 4, stream()) == EINVAL
        assert lib.mt_frame_smooth_chunks_split(xp, op, 0.5, 1.0, 1.0, B, P, T, 4, stream()) == EINVAL
    for dims in ((0, P, T), (B, 0, T), (B, P, 0), (B, -1, T)):
        assert lib.mt_frame_smooth_split(ptr(x), ptr(out), 0.5, 1.0, 1.0, None, *dims, 4, stream()) == EINVAL
        assert lib.mt_frame_smooth_chunks_split(ptr(x), ptr(out), 0.5, 1.0, 1.0, *dims, 4, stream()) == EINVAL
    both = torch.full((2 * x.numel(),), SENTINEL, device="cuda")                  # out overlaps the input without being it
    assert lib.mt_frame_smooth_split(both.data_ptr(), both.data_ptr() + 4 * T, 0.5, 1.0, 1.0, None, B, P, T, 4, stream()) == EINVAL
    assert lib.mt_frame_smooth_chunks_split(both.data_ptr() + 4, both.data_ptr(), 0.5, 1.0, 1.0, B, P, T, 4, stream()) == EINVAL
    assert "overlap" in _lib.last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (both == SENTINEL).all()


def test_smooth_frame_logits_takes_waves(mta):
    x = _random_case()["dev"]
    lengths = [T, 1025]
    want = mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, lengths)
    assert np.array_equal(want.cpu().numpy(), FR.smooth_ref(x.cpu().numpy(), 0.3, 1.0, 0.5, lengths, _activity(x, 0.3)))
    assert torch.equal(mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, lengths, waves=5), want)
    assert torch.equal(mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, chunks=True, waves=16), mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, chunks=True))
    assert mta.smooth_frame_logits(x, waves=4) is x
    for bad in (0, 1, 17, 2.0, True):
        with pytest.raises(ValueError, match="waves"):
            mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, waves=bad)


# ------------------------------------------------------------------------------------------------ the forced dispatch
CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import music_transcription_amd
from music_transcription_amd import _lib
x = torch.from_numpy(np.load(sys.argv[2])).cuda()
out = torch.full_like(x, -7.0)
ln = torch.tensor([int(v) for v in sys.argv[4].split(",")], dtype=torch.int64, device="cuda")
rc = _lib.lib.mt_frame_smooth(_lib.ptr(x), _lib.ptr(out), 0.5, 1.5, 0.25, _lib.ptr(ln), x.shape[0], x.shape[1], x.shape[2], _lib.stream_ptr())
torch.cuda.synchronize()
assert rc == 0, _lib.last_error()
np.save(sys.argv[3], out.cpu().numpy())
"""


def test_forced_dispatch_in_a_fresh_process(mta, tmp_path):
    lengths = (4161, 2689)
    x = _padded(_random_case()["dev"], lengths)
    want = _expect(x, 0.5, 1.5, 0.25, lengths)
    src, dst = str(tmp_path / "x.npy"), str(tmp_path / "y.npy")
    np.save(src, x.cpu().numpy())
    env = dict(os.environ, MT_SMOOTH_SPLIT="4")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, ROOT, src, dst, ",".join(map(str, lengths))], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert np.array_equal(np.load(dst), want)
