"""The offset-gated note decoder on the GPU (csrc/note_decode.h decode_window_off, mt_*_off in csrc/notes.hip, notes.py) against the
literal scan of offset_decode_ref.py, with scipy's maximum matching for the counts; then device against device for what must not
change (starts, note counts, tp_onset), hand-built rows on the window / slab / chunk / length boundaries, and the command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import note_list_ref as LR
import note_metrics_ref as NR
import offset_decode_ref as OR
from oracle import model_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P = 88
FS = 16000 / 512


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _cuda(*arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]                # (a copy: the shared cases are read-only)


def _case(B, T, thr, othr, kthr, seed):
    """The generator of test_gpu_notes with a third head: the activity of the three heads is fixed first, then logits are placed >= 0.01 from
    logit(threshold), far outside the band where host and device expf may disagree.  The offset activity marks the last active frame
    of every run of the frame activity, moved by -1 .. +1 frames; 10 % are dropped, 1 % of all frames fire spuriously, and three in
    ten marks are smeared over 2 or 3 frames."""
    rng = np.random.default_rng(seed)
    shape = (B, P, T)
    ref = OR.markov(rng, shape, 0.06, 0.2)
    shift = rng.integers(-2, 3, size=(B, P, 1))
    est = np.take_along_axis(ref, np.clip(np.arange(T)[None, None, :] - shift, 0, T - 1), axis=2)
    est ^= rng.random(shape) < 0.03
    prev = np.concatenate([np.zeros((B, P, 1), bool), est[..., :-1]], axis=2)
    ons = (est & ~prev) & (rng.random(shape) > 0.1)                         # most note starts, some missed
    ons |= est & (rng.random(shape) < 0.04)                                  # re-strikes inside held notes
    ons |= rng.random(shape) < 0.005                                         # onsets without frame activity
    nxt = np.concatenate([est[..., 1:], np.zeros((B, P, 1), bool)], axis=2)
    b, p, t = np.nonzero(est & ~nxt & (rng.random(shape) > 0.1))             # falling edges: the last active frame, 10 % dropped
    t = np.clip(t + rng.integers(-1, 2, size=t.shape), 0, T - 1)
    width = np.where(rng.random(t.shape) < 0.3, rng.integers(2, 4, size=t.shape), 1)
    offs = rng.random(shape) < 0.01                                          # spurious
    for w in range(3):
        m = width > w
        offs[b[m], p[m], np.clip(t[m] + w, 0, T - 1)] = True
    mag = lambda: rng.uniform(0.01, 4.0, size=shape)
    frame = np.where(est, OR.logit(thr) + mag(), OR.logit(thr) - mag()).astype(np.float32)
    onset = np.where(ons, OR.logit(othr) + mag(), OR.logit(othr) - mag()).astype(np.float32)
    offset = np.where(offs, OR.logit(kthr) + mag(), OR.logit(kthr) - mag()).astype(np.float32)
    assert (NR.sigmoid_active(frame, thr) == est).all() and (NR.sigmoid_active(onset, othr) == ons).all()
    assert (NR.sigmoid_active(offset, kthr) == offs).all()
    return frame, onset, offset, ref.astype(np.float32), (est, ons, offs)


def _note_list(rng, ref):
    """The runs of the roll as a note list in ticks, onsets moved by up to 15 ms and offsets by up to 60 ms (order and on < off kept)."""
    on, off, ptr = LR.notes_from_roll(ref)
    on = np.maximum(0, on.astype(np.int64) + rng.integers(-150, 151, size=on.shape))
    off = np.maximum(on + 1, off.astype(np.int64) + rng.integers(-600, 601, size=off.shape))
    return on.astype(np.int32), off.astype(np.int32), ptr


def _dev_notes(on, off, ptr):
    return {"on": torch.from_numpy(np.asarray(on, np.int32)).cuda(), "off": torch.from_numpy(np.asarray(off, np.int32)).cuda(),
            "ptr": torch.from_numpy(np.asarray(ptr, np.int64)).cuda()}


def _earlier_fraction(est, ons, offs, lengths):
    """Over all rows: (estimated notes that the offset head ends earlier than the onset-gated decoder would, estimated notes)."""
    B, _, T = est.shape
    earlier = total = 0
    for b in range(B):
        L = T if lengths is None else lengths[b]
        for p in range(P):
            a = NR.onset_notes(est[b, p, :L], ons[b, p, :L])
            c = OR.onset_offset_notes(est[b, p, :L], ons[b, p, :L], offs[b, p, :L])
            assert [s for s, _ in a] == [s for s, _ in c] and all(y[1] <= x[1] for x, y in zip(a, c))
            earlier += sum(y[1] < x[1] for x, y in zip(a, c))
            total += len(a)
    return earlier, total


CASES = [(1, 1), (3, 63), (3, 64), (3, 65), (2, 513), (2, 1025), (4, 938)]     # a window is 64 frames, a slab 512


def _thresholds(k):
    return (0.3, 0.5, 0.7)[k % 3], (0.5, 0.7, 0.3)[k % 3], (0.7, 0.3, 0.5)[k % 3]


def _ragged(rng, B, T):
    return ([T, 0] + [int(v) for v in rng.integers(0, T + 1, size=max(0, B - 2))])[:B]


_CASE_CACHE = {}


def _shared_case(B, T):
    """One case per shape, built once and shared by the roll test, the list test and the invariants; nobody writes to it."""
    if (B, T) not in _CASE_CACHE:
        k = CASES.index((B, T))
        thr, othr, kthr = _thresholds(k)
        frame, onset, offset, ref, act = _case(B, T, thr, othr, kthr, seed=700 + k)
        rng = np.random.default_rng(40 + k)
        for a in (frame, onset, offset, ref) + act:
            a.setflags(write=False)
        _CASE_CACHE[(B, T)] = dict(thr=(thr, othr, kthr), frame=frame, onset=onset, offset=offset, ref=ref, act=act,
                                   ragged=_ragged(rng, B, T), notes=_note_list(rng, ref))
    return _CASE_CACHE[(B, T)]


def _inputs_use_the_offset_head(c, lengths, want, want_onset_gated, T):
    """The condition on the inputs, on the reference alone: a kernel that ignores the offset head cannot pass."""
    if T < 63:
        return
    earlier, total = _earlier_fraction(*c["act"], lengths)
    print(f"offset head ends {earlier} of {total} estimated notes earlier ({earlier / max(total, 1):.3f})")
    assert total > 0 and 10 * earlier >= total
    assert (want[:, 3] != want_onset_gated[:, 3]).any()


@pytest.mark.parametrize("B,T", CASES)
def test_roll_counts_equal_the_reference(mta, B, T):
    from music_transcription_amd.notes import note_match_counts
    c = _shared_case(B, T)
    thr, othr, kthr = c["thr"]
    est, ons, offs = c["act"]
    x, o, k, r = _cuda(c["frame"], c["onset"], c["offset"], c["ref"])
    for lengths in (None, c["ragged"]):
        want = OR.match_counts_active(est, ons, offs, c["ref"], lengths)
        _inputs_use_the_offset_head(c, lengths, want, NR.match_counts_active(est, c["ref"], ons, lengths), T)
        got = note_match_counts(x, r, thr, o, othr, lengths, offset_logits=k, offset_threshold=kthr).cpu().numpy()
        assert got.dtype == np.int64 and got.shape == (B, 4)
        np.testing.assert_array_equal(got, want, err_msg=f"lengths={'ragged' if lengths else None}")


@pytest.mark.parametrize("B,T", CASES)
def test_list_counts_equal_the_reference(mta, B, T):
    from music_transcription_amd.notes import note_match_list
    c = _shared_case(B, T)
    thr, othr, kthr = c["thr"]
    est, ons, offs = c["act"]
    r_on, r_off, r_ptr = c["notes"]
    x, o, k = _cuda(c["frame"], c["onset"], c["offset"])
    ref = _dev_notes(r_on, r_off, r_ptr)
    for lengths in (None, c["ragged"]):
        want = OR.match_list_counts_active(est, ons, offs, r_on, r_off, r_ptr, lengths)
        _inputs_use_the_offset_head(c, lengths, want, LR.match_list_counts_active(est, r_on, r_off, r_ptr, ons, lengths), T)
        got = note_match_list(x, ref, thr, o, othr, lengths, offset_logits=k, offset_threshold=kthr).cpu().numpy()
        assert got.dtype == np.int64 and got.shape == (B, 4)
        np.testing.assert_array_equal(got, want, err_msg=f"lengths={'ragged' if lengths else None}")


@pytest.mark.parametrize("B,T", CASES)
def test_note_lists_equal_the_reference(mta, B, T):
    """The B samples as B chunks of one recording: the carries cross every chunk boundary."""
    from music_transcription_amd.notes import heads_to_notes_device
    c = _shared_case(B, T)
    thr, othr, kthr = c["thr"]
    x, o, k = _cuda(c["frame"], c["onset"], c["offset"])
    got = heads_to_notes_device(x, o, thr, othr, fs=FS, min_midi=0, offset_logits=k, offset_threshold=kthr)
    assert [(p, int(round(s * FS)), int(round(e * FS))) for p, s, e in got] == OR.heads_notes_active(*c["act"])


# ------------------------------------------------------------------------------------------------ device against device
@pytest.mark.parametrize("B,T", CASES)
def test_only_the_offset_column_changes(mta, B, T):
    from music_transcription_amd.notes import note_match_counts, note_match_list
    c = _shared_case(B, T)
    thr, othr, kthr = c["thr"]
    x, o, k, r = _cuda(c["frame"], c["onset"], c["offset"], c["ref"])
    ref = _dev_notes(*c["notes"])
    for lengths in (None, c["ragged"]):
        a = note_match_counts(x, r, thr, o, othr, lengths)
        b = note_match_counts(x, r, thr, o, othr, lengths, offset_logits=k, offset_threshold=kthr)
        assert torch.equal(a[:, :3], b[:, :3])
        a = note_match_list(x, ref, thr, o, othr, lengths)
        b = note_match_list(x, ref, thr, o, othr, lengths, offset_logits=k, offset_threshold=kthr)
        assert torch.equal(a[:, :3], b[:, :3])


@pytest.mark.parametrize("B,T", CASES)
def test_a_silent_offset_head_gives_the_onset_gated_decoder(mta, B, T):
    from music_transcription_amd.notes import heads_to_notes_device, note_match_counts, note_match_list
    c = _shared_case(B, T)
    thr, othr, _ = c["thr"]
    x, o, r = _cuda(c["frame"], c["onset"], c["ref"])
    k = torch.full_like(x, -30.0)
    ref = _dev_notes(*c["notes"])
    for lengths in (None, c["ragged"]):
        assert torch.equal(note_match_counts(x, r, thr, o, othr, lengths), note_match_counts(x, r, thr, o, othr, lengths, offset_logits=k))
        assert torch.equal(note_match_list(x, ref, thr, o, othr, lengths), note_match_list(x, ref, thr, o, othr, lengths, offset_logits=k))
    assert heads_to_notes_device(x, o, thr, othr) == heads_to_notes_device(x, o, thr, othr, offset_logits=k)


# ------------------------------------------------------------------------------------------------ boundaries, hand-built
def _rows_to_logits(rows, T):
    """[(frame runs, onset frames, offset frames)] -> (1, len(rows), T) activities and logits at +-3."""
    act = np.zeros((3, 1, len(rows), T), bool)
    for i, (runs, ons, offs) in enumerate(rows):
        for s, e in runs:
            act[0, 0, i, s:e] = True
        act[1, 0, i, list(ons)] = True
        act[2, 0, i, list(offs)] = True
    return act, [np.where(a, 3.0, -3.0).astype(np.float32) for a in act]


def _device_notes(logits, lengths=None):
    """Per row [(start, end)] through mt_heads_to_notes_off (rows as pitches of one chunk); with lengths, each row cut to its length."""
    from music_transcription_amd.notes import heads_to_notes_device
    f, o, k = logits
    n_rows = f.shape[1]
    out = [[] for _ in range(n_rows)]
    if lengths is None:
        for p, s, e in heads_to_notes_device(*_cuda(f, o), 0.5, 0.5, fs=1.0, min_midi=0, offset_logits=_cuda(k)[0]):
            out[p].append((int(s), int(e)))
        return out
    for i, L in enumerate(lengths):
        cut = [np.ascontiguousarray(a[:, i:i + 1, :L]) for a in (f, o, k)]
        out[i] = [(int(s), int(e)) for _, s, e in heads_to_notes_device(*_cuda(*cut[:2]), 0.5, 0.5, fs=1.0, min_midi=0,
                                                                           offset_logits=_cuda(cut[2])[0])]
    return out


def test_edges_on_the_window_and_slab_boundaries(mta):
    from music_transcription_amd.notes import note_match_counts, note_match_list
    T = 600
    rows = [([(10, 600)], [10], [at]) for at in (63, 64, 511, 512)]                  # an edge on each side of a window / slab boundary
    rows.append(([(10, 600)], [64], [63, 64]))                                        # active on 63 and 64: no edge at 64, no cut
    rows.append(([(10, 600)], [512], [510, 511, 512]))                                # the same across the slab boundary
    rows.append(([(10, 600)], [10, 64], [63]))                                        # cut at 63, struck again on the window's first frame
    rows.append(([(10, 600)], [10, 513], [510, 511]))                                 # cut at 510; the frame run opens nothing until 513
    want = [[(10, 64)], [(10, 65)], [(10, 512)], [(10, 513)], [(64, 600)], [(512, 600)], [(10, 64), (64, 600)], [(10, 511), (513, 600)]]
    act, logits = _rows_to_logits(rows, T)
    assert [OR.onset_offset_notes(act[0, 0, i], act[1, 0, i], act[2, 0, i]) for i in range(len(rows))] == want
    assert _device_notes(logits) == want
    # the matchers decode the same notes: each row a sample of its own against a reference that ends where the offset head fires
    ref = np.zeros((len(rows), 1, T), np.float32)
    for i, notes in enumerate(want):
        ref[i, 0, notes[0][0]:notes[0][1]] = 1.0
    f, o, k = [t.permute(1, 0, 2).contiguous() for t in _cuda(*logits)]
    a = [x[0][:, None] for x in act]
    want_counts = OR.match_counts_active(*a, ref)
    assert want_counts[:, 3].sum() == len(rows) > NR.match_counts_active(a[0], ref, a[1])[:, 3].sum()
    np.testing.assert_array_equal(note_match_counts(f, _cuda(ref)[0], 0.5, o, 0.5, offset_logits=k).cpu().numpy(), want_counts)
    r_on, r_off, r_ptr = LR.notes_from_roll(ref)
    got = note_match_list(f, _dev_notes(r_on, r_off, r_ptr), 0.5, o, 0.5, offset_logits=k).cpu().numpy()
    np.testing.assert_array_equal(got, OR.match_list_counts_active(*a, r_on, r_off, r_ptr))


def test_edges_at_the_valid_length(mta):
    from music_transcription_amd.notes import note_match_counts, note_match_list
    T, L = 200, 130
    rows = [([(100, 200)], [100], [L - 1]),                                           # an edge on the last valid frame: the note ends at L
            ([(100, 200)], [100], [L]),                                               # an edge on the first invalid frame: not seen
            ([(100, 200)], [100], [L - 2])]                                           # and one before: the note ends at L - 1
    want = [[(100, L)], [(100, L)], [(100, L - 1)]]
    act, logits = _rows_to_logits(rows, T)
    assert [OR.onset_offset_notes(act[0, 0, i, :L], act[1, 0, i, :L], act[2, 0, i, :L]) for i in range(3)] == want
    assert _device_notes(logits, [L] * 3) == want
    # the matchers under `lengths`, each row a sample of its own, against the reference [100, L) (its run goes on past L)
    f, o, k = [t.permute(1, 0, 2).contiguous() for t in _cuda(*logits)]
    ref = np.zeros((3, 1, T), np.float32)
    ref[:, 0, 100:140] = 1.0
    want_counts = OR.match_counts_active(act[0, 0][:, None], act[1, 0][:, None], act[2, 0][:, None], ref, [L] * 3)
    np.testing.assert_array_equal(want_counts, [[1, 1, 1, 1]] * 3)
    got = note_match_counts(f, _cuda(ref)[0], 0.5, o, 0.5, [L] * 3, offset_logits=k).cpu().numpy()
    np.testing.assert_array_equal(got, want_counts)
    r_on, r_off, r_ptr = LR.notes_from_roll(ref)
    got = note_match_list(f, _dev_notes(r_on, r_off, r_ptr), 0.5, o, 0.5, [L] * 3, offset_logits=k).cpu().numpy()
    np.testing.assert_array_equal(got, OR.match_list_counts_active(act[0, 0][:, None], act[1, 0][:, None], act[2, 0][:, None], r_on, r_off,
                                                                   r_ptr, [L] * 3))


def test_edges_on_chunk_boundaries_and_the_capacity_protocol(mta):
    from music_transcription_amd import _lib
    NB, T = 3, 50
    f = np.full((NB, P, T), -3.0, np.float32)
    o, k = f.copy(), f.copy()
    f[:, 3] = f[:, 4] = f[:, 5] = 3.0                      # three keys held through all 150 frames
    o[0, 3, 5] = o[0, 4, 5] = o[0, 5, 5] = 3.0
    k[0, 3, T - 1] = 3.0                                   # an edge on the last frame of chunk 0: ends at 50
    k[1, 4, 0] = 3.0                                       # an edge on the first frame of chunk 1: ends at 51
    k[0, 5, T - 1] = k[1, 5, 0] = 3.0                      # active across the boundary: one edge, on frame 49
    o[1, 5, 0] = 3.0                                       # struck again on the first frame of chunk 1, under the smeared offset
    want = [(3, 5, 50), (4, 5, 51), (5, 5, 50), (5, 50, 150)]
    assert OR.heads_notes_active(f > 0, o > 0, k > 0) == want
    x, on, off = _cuda(f, o, k)
    counts = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    call = lambda s, e, cap: _lib.lib.mt_heads_to_notes_off(_lib.ptr(x), _lib.ptr(on), _lib.ptr(off), 0.5, 0.5, 0.5, NB, P, T, _lib.ptr(counts),
                                                            _lib.ptr(s), _lib.ptr(e), cap, _lib.stream_ptr())
    s = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    e = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    assert call(s, e, 1) == 0                              # capacity 1: the total is reported, nothing is written past the capacity
    assert int(counts.sum()) == len(want) and counts.cpu().tolist()[3:6] == [1, 1, 2]
    assert (s[1:] == -7).all() and (e[1:] == -7).all()
    assert (int(s[0]), int(e[0])) == (5, 50)               # pitch 3's note fits; the pitches after it do not
    assert call(s, e, int(counts.sum())) == 0
    pitches = np.repeat(np.arange(P), counts.cpu().numpy())
    assert list(zip(pitches.tolist(), s[:4].cpu().tolist(), e[:4].cpu().tolist())) == want
    assert (s[4:] == -7).all() and (e[4:] == -7).all()


# ------------------------------------------------------------------------------------------------ thresholds, arguments
def test_offset_activity_at_the_threshold_equals_predict_threshold(mta):
    """Offset logits at logit(thr), one ulp either side and densely around it (the candidates of test_gpu_notes'
    test_activity_at_the_threshold_equals_predict_threshold): the kernel's offset activity is mt_predict_threshold's bit for bit
    (device vs device).  Every candidate is a one-frame offset mark between strongly inactive frames on the second frame of a
    12-frame note of its own, which is 2 frames long if the mark is active: 10 frames apart is outside the offset tolerance, so
    tp_onset_offset against the long and against the short reference counts the inactive and the active candidates."""
    from music_transcription_amd.notes import note_match_counts
    from music_transcription_amd import ops
    for thr in (0.3, 0.5, 0.7):
        x0 = np.float32(OR.logit(thr))
        near = [x0, np.nextafter(x0, np.float32(np.inf)), np.nextafter(x0, np.float32(-np.inf))]
        cand = np.concatenate([np.array(near, np.float32), (x0 + np.linspace(-3e-4, 3e-4, 2001)).astype(np.float32)])
        n, S = len(cand), 16
        T = S * n
        frow, orow, krow = (np.full(T, -30.0, np.float32) for _ in range(3))
        for w in range(12):
            frow[w::S] = 30.0                                      # block i: frames [16 i, 16 i + 12) are active
        orow[0::S] = 30.0
        krow[1::S] = cand                                          # an active candidate ends the note at 16 i + 2
        f, o, k = (torch.from_numpy(a).cuda().view(1, 1, -1) for a in (frow, orow, krow))
        active = ops.predict_from_logits(k, thr).cpu().numpy().reshape(-1)[1::S] > 0
        n_active = int(active.sum())
        assert 0 < n_active < n
        long_ref = torch.from_numpy((frow > 0).astype(np.float32)).cuda().view(1, 1, -1)
        short = np.zeros(T, np.float32)
        short[0::S] = short[1::S] = 1.0
        short_ref = torch.from_numpy(short).cuda().view(1, 1, -1)
        got_long = note_match_counts(f, long_ref, 0.5, o, 0.5, offset_logits=k, offset_threshold=thr).cpu().numpy()[0]
        got_short = note_match_counts(f, short_ref, 0.5, o, 0.5, offset_logits=k, offset_threshold=thr).cpu().numpy()[0]
        np.testing.assert_array_equal(got_long, [n, n, n, n - n_active], err_msg=str(thr))
        np.testing.assert_array_equal(got_short, [n, n, n, n_active], err_msg=str(thr))


def test_bad_arguments_are_refused_and_write_nothing(mta):
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import heads_to_notes_device, note_match_counts, note_match_list
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_ptr()
    B, T = 2, 10
    x = torch.zeros(B, P, T, device="cuda")
    c = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    on = torch.zeros(4, dtype=torch.int32, device="cuda")
    rp = torch.zeros(B * P + 1, dtype=torch.int64, device="cuda")
    cnt = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    s, e = torch.full((8,), -7, dtype=torch.int32, device="cuda"), torch.full((8,), -7, dtype=torch.int32, device="cuda")
    EINVAL = -1                                                             # MT_EINVAL
    bad = [(None, 0.5)] + [(x, t) for t in (0.0, 1.0, -0.5, 1.5, float("nan"))]
    for k, kthr in bad:
        assert lib.mt_note_match_counts_off(ptr(x), ptr(x), ptr(k), 0.5, 0.5, kthr, ptr(x), None, ptr(c), B, P, T, st) == EINVAL
        assert lib.mt_note_match_list_off(ptr(x), ptr(x), ptr(k), 0.5, 0.5, kthr, ptr(on), ptr(on), ptr(rp), None, ptr(c), B, P, T, st) == EINVAL
        assert lib.mt_heads_to_notes_off(ptr(x), ptr(x), ptr(k), 0.5, 0.5, kthr, B, P, T, ptr(cnt), ptr(s), ptr(e), 8, st) == EINVAL
    # a NULL onset pointer and the other two thresholds are refused as well
    assert lib.mt_note_match_counts_off(ptr(x), None, ptr(x), 0.5, 0.5, 0.5, ptr(x), None, ptr(c), B, P, T, st) == EINVAL
    assert lib.mt_note_match_list_off(ptr(x), None, ptr(x), 0.5, 0.5, 0.5, ptr(on), ptr(on), ptr(rp), None, ptr(c), B, P, T, st) == EINVAL
    assert lib.mt_heads_to_notes_off(ptr(x), None, ptr(x), 0.5, 0.5, 0.5, B, P, T, ptr(cnt), ptr(s), ptr(e), 8, st) == EINVAL
    assert lib.mt_note_match_counts_off(ptr(x), ptr(x), ptr(x), 1.0, 0.5, 0.5, ptr(x), None, ptr(c), B, P, T, st) == EINVAL
    assert lib.mt_note_match_counts_off(ptr(x), ptr(x), ptr(x), 0.5, 0.0, 0.5, ptr(x), None, ptr(c), B, P, T, st) == EINVAL
    torch.cuda.synchronize()
    assert (c == -7).all() and (cnt == -7).all() and (s == -7).all() and (e == -7).all()
    # the Python layer: thresholds, shapes, and the onset head that the decoder cannot do without
    with pytest.raises(ValueError):
        note_match_counts(x, x, 0.5, x, 0.5, offset_logits=x, offset_threshold=1.0)
    with pytest.raises(ValueError):
        note_match_counts(x, x, 0.5, x, 0.5, offset_logits=x[:, :, :5])
    with pytest.raises(ValueError):
        note_match_counts(x, x, 0.5, offset_logits=x)
    with pytest.raises(ValueError):
        note_match_list(x, {"on": on, "off": on, "ptr": rp}, 0.5, offset_logits=x)
    with pytest.raises(ValueError):
        heads_to_notes_device(x, None, offset_logits=x)


# ------------------------------------------------------------------------------------------------ end to end
NM, H, L = 32, 16, 2


def _large(mta, n_mels=NM, seed=3):
    m = mta.TranscriptionModel(model_type="cnn_rnn_large", n_mels=n_mels, hidden_size=H, num_layers=L, dropout=0.0, device="cuda")
    m.load_state_dict(R.make_state_dict("cnn_rnn_large", n_mels, H, L, seed), strict=True)
    m.eval()
    return m


def _mid_threshold(logits):
    """A threshold near the median activation, so that a seeded random model yields plenty of notes; 4 decimals, as the CLIs print."""
    return round(float(np.clip(torch.sigmoid(logits.float().median()).item(), 0.05, 0.95)), 4)


def _midi_notes(path):
    """[(pitch, start tick, end tick)] of the one instrument track transcribe.write_midi writes, in its pitch-major input order."""
    data = open(path, "rb").read()
    at = data.index(b"MTrk", data.index(b"MTrk") + 4) + 8
    tick, open_at, notes = 0, {}, []
    at += 3                                                                 # delta 0 + program change (2 bytes)
    while True:
        d = 0
        while True:
            byte = data[at]
            at += 1
            d = (d << 7) | (byte & 0x7F)
            if not byte & 0x80:
                break
        tick += d
        status, a, b = data[at], data[at + 1], data[at + 2]
        at += 3
        if status == 0xFF:
            break
        if status == 0x90:
            open_at[a] = tick
        else:
            notes.append((a, open_at.pop(a), tick))
    return sorted(notes)


def test_main_writes_the_offset_gated_notes(mta, tmp_path):
    from scipy.io import wavfile
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    from music_transcription_amd.notes import heads_to_notes_device
    rng = np.random.default_rng(4)
    wav, ckpt, mid = str(tmp_path / "a.wav"), str(tmp_path / "m.pth"), str(tmp_path / "a.mid")
    wavfile.write(wav, 16000, (0.2 * rng.standard_normal(16000 * 40)).clip(-1, 1).astype(np.float32))
    sd = R.make_state_dict("cnn_rnn_large", NM, H, L, 9)
    torch.save(sd, ckpt)
    model = _large(mta, seed=9)
    chunks, _ = tr.split_into_chunks_device(tr.load_audio_device(wav, 16000, "cuda"))
    with torch.no_grad():
        mel, cmax = get_frontend(16000, NM, 512, "cuda")(chunks, clamp=False)
        heads = model.model(mel, chunk_max_power=cmax, return_all_heads=True)
    thr, othr, kthr = (_mid_threshold(heads[h]) for h in ("frame", "onset", "offset"))
    want = heads_to_notes_device(heads["frame"], heads["onset"], thr, othr, FS, offset_logits=heads["offset"], offset_threshold=kthr)
    gated = heads_to_notes_device(heads["frame"], heads["onset"], thr, othr, FS)
    assert len(want) == len(gated) > 0 and want != gated                    # the offset head does cut notes of this model
    assert tr.transcribe_chunks_to_notes(model, chunks, thr, n_mels=NM, decoder="onset_offset", onset_threshold=othr,
                                         offset_threshold=kthr) == want
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), wav, ckpt, "-o", mid, "-d", "cuda", "-t", str(thr), "--decoder",
                        "onset_offset", "--onset-threshold", str(othr), "--offset-threshold", str(kthr), "--n-mels", str(NM),
                        "--hidden-size", str(H), "--num-layers", str(L)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tick = lambda t: int(round(t * 220 * 120.0 / 60.0))
    assert _midi_notes(mid) == sorted((p, tick(s), tick(e)) for p, s, e in want)


def test_evaluate_script_with_the_offset_gated_decoder(mta, tmp_path):
    from music_transcription_amd import evaluate as E
    from music_transcription_amd.notes import note_match_counts, note_prf
    cache = os.path.join(GOLDEN, "cache_fixture")
    n_mels = 16
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", n_mels, H, L, 5), ckpt)
    model = _large(mta, n_mels=n_mels, seed=5)
    ds = mta.CachedMaestroDataset(cache, "train")
    with torch.no_grad():
        heads = model(ds[0][0][None].cuda(), return_all_heads=True)
    thr, othr, kthr = (_mid_threshold(heads[h]) for h in ("frame", "onset", "offset"))
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--cache_dir", cache, "--split", "train",
            "--model_type", "cnn_rnn_large", "--hidden_size", str(H), "--num_layers", str(L), "--headless", "--threshold", str(thr),
            "--onset_threshold", str(othr), "--note_metrics", "--decoder", "onset_offset"]
    gated = E.note_metrics_dataset(model, ds, thr, othr)
    for k in (0.5, kthr):                                                   # the default, and a threshold at which this head does fire
        got = E.note_metrics_dataset(model, ds, thr, othr, offset_threshold=k)
        want = got["mean"]
        r = subprocess.run(base + ["--offset_threshold", str(k)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = dict(l.split("=") for l in r.stdout.strip().splitlines())
        assert list(out) == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1"], r.stdout
        assert out["EVAL_NOTE_ONSET_F1"] == f"{want['onset_f1']:.6f}" and out["EVAL_NOTE_ONSET_OFFSET_F1"] == f"{want['onset_offset_f1']:.6f}"
        # the onset criterion is the onset-gated decoder's
        assert all(got["per_sample"][m] == gated["per_sample"][m] for m in ("onset_precision", "onset_recall", "onset_f1"))
    # at kthr the offset logits did reach the kernel: the onset+offset figures are not the onset-gated decoder's, and they are
    # those of the counts on the collected heads
    assert got["per_sample"]["onset_offset_f1"] != gated["per_sample"]["onset_offset_f1"]
    lr = E.collect_logits(model, ds, range(len(ds)), all_heads=True, with_offset=True)
    assert [len(x) for x in lr] == [5] * len(ds)
    for n, (_, frame, roll, onset, offset) in enumerate(lr):
        c = note_match_counts(frame, roll, thr, onset, othr, offset_logits=offset, offset_threshold=kthr)
        assert note_prf(c)[0]["onset_offset"][2] == got["per_sample"]["onset_offset_f1"][n]
    with pytest.raises(ValueError, match="onset_offset"):
        E.tune_note_thresholds(model, ds, "cuda", decoder="onset_offset", log=None)
    with pytest.raises(ValueError):
        E.note_metrics_dataset(model, ds, thr, None, offset_threshold=0.5)


def test_windows_carry_the_stitched_offset_head(mta):
    """transcribe_windows(all_heads=True, with_offset=True) -> (frame, onset, offset) in that order: the first two are what
    all_heads=True alone returns, the third is the offset head of every window through the chunk path, stitched by hand with the
    plan; and the window transcription with decoder="onset_offset" decodes exactly these three."""
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    from music_transcription_amd.notes import heads_to_notes_device
    from music_transcription_amd.windows import plan_windows, transcribe_windows
    model = _large(mta, seed=7)
    n, W, HOP = 16000 * 45, 480000, 512
    g = torch.Generator(device="cuda").manual_seed(6)
    y = 0.2 * torch.randn(n, device="cuda", generator=g)
    got = transcribe_windows(model, [y], 2.0, all_heads=True, with_offset=True)[0]
    two = transcribe_windows(model, [y], 2.0, all_heads=True)[0]
    assert len(got) == 3 and len(two) == 2 and torch.equal(got[0], two[0]) and torch.equal(got[1], two[1])
    plan = plan_windows(n, 2.0)
    assert len(plan.start) == 2                                              # the stitch has a seam
    chunks = torch.zeros(len(plan.start), W, device="cuda")
    for b, a in enumerate(plan.start):
        seg = y[HOP * int(a):HOP * int(a) + W]
        chunks[b, :seg.numel()] = seg
    with torch.no_grad():
        mel, cmax = get_frontend(16000, NM, HOP, "cuda")(chunks, clamp=False)
        heads = model.model(mel, chunk_max_power=cmax, return_all_heads=True)
    for at, name in enumerate(("frame", "onset", "offset")):
        lg = heads[name].cpu().numpy()
        want = np.full((P, plan.Tg), np.nan, np.float32)
        for b, (a, lo, hi) in enumerate(zip(plan.start, plan.lo, plan.hi)):
            want[:, a + lo:a + hi] = lg[b, :, lo:hi]
        assert np.array_equal(got[at].cpu().numpy(), want), name
    assert not torch.equal(got[2], got[1]) and not torch.equal(got[2], got[0])
    thr, othr, kthr = (_mid_threshold(h) for h in got)
    want = heads_to_notes_device(got[0][None], got[1][None], thr, othr, FS, offset_logits=got[2][None], offset_threshold=kthr)
    assert want != heads_to_notes_device(got[0][None], got[1][None], thr, othr, FS)
    assert tr.transcribe_windows_to_notes(model, y, 2.0, thr, n_mels=NM, decoder="onset_offset", onset_threshold=othr,
                                          offset_threshold=kthr) == want
    with pytest.raises(ValueError, match="all_heads"):
        transcribe_windows(model, [y], 2.0, with_offset=True)
