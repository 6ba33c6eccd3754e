"""mt_notes_batch / notes.notes_batch_device (csrc/notes_batch.hip): the notes of a padded batch of whole recordings with lengths,
integer-exact against the single-recording kernels (mt_roll_to_notes, mt_heads_to_notes) on contiguous trimmed copies, against the
numpy decoders of note_metrics_ref.py on the device's activity bits, and against the matcher's n_est."""
import numpy as np
import pytest
import torch

import note_metrics_ref as NR

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 64


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def _markov(rng, shape, p_on, p_off, p0):
    u = rng.random(shape)
    out = np.zeros(shape, bool)
    state = rng.random(shape[:-1]) < p0
    for t in range(shape[-1]):
        out[..., t] = state
        state = np.where(state, u[..., t] >= p_off, u[..., t] < p_on)
    return out


def _case(B, P, T, thr, othr, seed):
    """Frame / onset logits: runs of frame activity, onsets at most run starts, re-strikes and stray onsets, and about 3 % of the
    cells exactly at logit(threshold) or one ulp either side of it."""
    rng = np.random.default_rng(seed)
    est = _markov(rng, (B, P, T), 0.12, 0.15, 0.7)
    prev = np.concatenate([np.zeros((B, P, 1), bool), est[..., :-1]], axis=2)
    ons = (est & ~prev) & (rng.random((B, P, T)) > 0.1)
    ons |= est & (rng.random((B, P, T)) < 0.05)
    ons |= rng.random((B, P, T)) < 0.01
    mag = lambda: rng.uniform(0.01, 4.0, size=(B, P, T))
    frame = np.where(est, _logit(thr) + mag(), _logit(thr) - mag()).astype(np.float32)
    onset = np.where(ons, _logit(othr) + mag(), _logit(othr) - mag()).astype(np.float32)
    for x, t in ((frame, thr), (onset, othr)):
        x0 = np.float32(_logit(t))
        near = np.array([x0, np.nextafter(x0, np.float32(np.inf)), np.nextafter(x0, np.float32(-np.inf))], np.float32)
        tie = rng.random((B, P, T)) < 0.03
        x[tie] = near[rng.integers(0, 3, size=int(tie.sum()))]
    return frame, onset


def _length_values(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 7]


def _lengths(T, B, k):
    v = _length_values(T)
    return [v[(k + j) % len(v)] for j in range(B)]


def _clamp(lengths, B, T):
    return [T] * B if lengths is None else [min(max(int(v), 0), T) for v in lengths]


def _batch(x, on, thr, othr, lengths, capacity=None):
    """mt_notes_batch -> (counts, row_off, starts, ends) as numpy; starts / ends are the whole buffers, GUARD elements behind capacity."""
    from music_transcription_amd import _lib
    B, P, T = x.shape
    rows = B * P
    dev = x.device
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=dev)
    counts = torch.full((rows,), SENTINEL, dtype=torch.int32, device=dev)
    row_off = torch.full((rows + 1,), SENTINEL, dtype=torch.int64, device=dev)
    cap = B * P * (T // 2 + 1) if capacity is None else capacity          # no row holds more than ceil(T / 2) notes
    s = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    e = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.mt_notes_batch(_lib.ptr(x), _lib.ptr(on), thr, othr, _lib.ptr(ln), B, P, T, _lib.ptr(counts), _lib.ptr(row_off),
                                       _lib.ptr(s), _lib.ptr(e), cap, _lib.stream_ptr()), "mt_notes_batch")
    return counts.cpu().numpy(), row_off.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()


def _single(xb, ob, thr, othr):
    """The single-recording kernel on a contiguous (P, L) copy -> (counts (P,), starts, ends)."""
    from music_transcription_amd import _lib
    P, L = xb.shape
    dev = xb.device
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    cap = P * (L // 2 + 1)
    s, e = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    if ob is None:
        _lib.check(_lib.lib.mt_roll_to_notes(_lib.ptr(xb), 0, thr, 1, P, L, _lib.ptr(counts), _lib.ptr(s), _lib.ptr(e), cap, _lib.stream_ptr()),
                   "mt_roll_to_notes")
    else:
        _lib.check(_lib.lib.mt_heads_to_notes(_lib.ptr(xb), _lib.ptr(ob), thr, othr, 1, P, L, _lib.ptr(counts), _lib.ptr(s), _lib.ptr(e), cap,
                                              _lib.stream_ptr()), "mt_heads_to_notes")
    c = counts.cpu().numpy()
    n = int(c.sum())
    return c, s[:n].cpu().numpy(), e[:n].cpu().numpy()


def _numpy_notes(xb, ob, thr, othr):
    """note_metrics_ref's decoders on the device's activity bits (mt_predict_threshold: the kernels' expression) -> per row [(s, e)]."""
    from music_transcription_amd import ops
    f = ops.predict_from_logits(xb, thr).cpu().numpy() > 0
    if ob is None:
        return [NR.frame_notes(r) for r in f]
    o = ops.predict_from_logits(ob, othr).cpu().numpy() > 0
    return [NR.onset_notes(fr, orow) for fr, orow in zip(f, o)]


SHAPES = [(P, T) for P in (3, 88) for T in (1, 63, 64, 65, 130, 1100)]
THRESHOLDS = [(0.3, 0.5), (0.5, 0.7), (0.7, 0.3)]


# ------------------------------------------------------------------ 1. against the single-recording kernels and numpy
@pytest.mark.parametrize("decoder", ["frame", "onset"])
@pytest.mark.parametrize("P,T", SHAPES)
def test_equals_the_single_recording_kernels(mta, P, T, decoder):
    B = 5
    k = SHAPES.index((P, T))
    rows_with_note = rows_all = ends_at_L = 0
    for j, (thr, othr) in enumerate(THRESHOLDS):
        frame, onset = _case(B, P, T, thr, othr, seed=1000 + 10 * k + j)
        x = torch.from_numpy(frame).cuda()
        on = torch.from_numpy(onset).cuda() if decoder == "onset" else None
        for lengths in (None, _lengths(T, B, 3 * k + 5 * j), _lengths(T, B, 3 * k + 5 * j + 4)):
            counts, row_off, s, e = _batch(x, on, thr, othr, lengths)
            assert row_off[0] == 0 and np.array_equal(row_off[1:], np.cumsum(counts.astype(np.int64)))
            Ls = _clamp(lengths, B, T)
            for b, L in enumerate(Ls):
                got_c = counts[b * P:(b + 1) * P]
                lo, hi = int(row_off[b * P]), int(row_off[(b + 1) * P])
                if L == 0:
                    assert not got_c.any() and lo == hi
                    continue
                xb = x[b, :, :L].contiguous()
                ob = None if on is None else on[b, :, :L].contiguous()
                want_c, want_s, want_e = _single(xb, ob, thr, othr)
                assert np.array_equal(got_c, want_c), (lengths, b)
                assert np.array_equal(s[lo:hi], want_s) and np.array_equal(e[lo:hi], want_e), (lengths, b)
                ref = _numpy_notes(xb, ob, thr, othr)
                assert [len(r) for r in ref] == got_c.tolist()
                assert [n for r in ref for n in r] == list(zip(s[lo:hi].tolist(), e[lo:hi].tolist())), (lengths, b)
                ends_at_L += int((e[lo:hi] == L).sum())
            rows_with_note += int((counts > 0).sum())
            rows_all += B * P
    assert rows_with_note >= 0.3 * rows_all, (rows_with_note, rows_all)
    assert ends_at_L > 0


# ------------------------------------------------------------------ 2. padding is never read as data
@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_padding_is_never_read(mta, decoder):
    B = 5
    for k, (P, T) in enumerate(SHAPES):
        thr, othr = THRESHOLDS[k % 3]
        frame, onset = _case(B, P, T, thr, othr, seed=2000 + k)
        lengths = _lengths(T, B, k)
        Ls = _clamp(lengths, B, T)
        want = None
        for fill in (None, 50.0, -50.0, float("nan")):
            f, o = frame.copy(), onset.copy()
            if fill is not None:
                for b, L in enumerate(Ls):
                    f[b, :, L:] = fill
                    o[b, :, L:] = fill
            got = _batch(torch.from_numpy(f).cuda(), torch.from_numpy(o).cuda() if decoder == "onset" else None, thr, othr, lengths)
            if want is None:
                want = got
                assert want[1][-1] > 0 or T == 1
            else:
                assert all(np.array_equal(a, b) for a, b in zip(got, want)), (P, T, fill)


# ------------------------------------------------------------------ 3. capacity protocol
@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_capacity_protocol(mta, decoder):
    B, P, T = 5, 88, 130
    thr, othr = 0.5, 0.3
    frame, onset = _case(B, P, T, thr, othr, seed=31)
    x = torch.from_numpy(frame).cuda()
    on = torch.from_numpy(onset).cuda() if decoder == "onset" else None
    lengths = [130, 64, 0, 137, 65]
    counts, row_off, s_full, e_full = _batch(x, on, thr, othr, lengths)
    total = int(row_off[-1])
    first = int(counts[np.nonzero(counts)[0][0]])
    assert total > first > 0
    for cap in (total, total - 1, first, 0):
        c, off, s, e = _batch(x, on, thr, othr, lengths, capacity=cap)
        assert np.array_equal(c, counts) and np.array_equal(off, row_off)
        assert s.size == cap + GUARD
        written = np.zeros(cap + GUARD, bool)
        for r in range(B * P):
            lo, hi = int(off[r]), int(off[r]) + int(c[r])
            if hi <= cap:
                written[lo:hi] = True
        at = np.nonzero(written)[0]                            # rows that fit: the full result, at the same places
        assert np.array_equal(s[at], s_full[at]) and np.array_equal(e[at], e_full[at])
        assert (s[~written] == SENTINEL).all() and (e[~written] == SENTINEL).all()
        assert int(written.sum()) == (total if cap == total else int(sum(c[r] for r in range(B * P) if off[r] + c[r] <= cap)))
        if cap == total - 1:
            assert 0 < written.sum() < total


# ------------------------------------------------------------------ 4. agreement with the matcher
@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_counts_agree_with_the_matcher(mta, decoder):
    from music_transcription_amd.notes import note_match_counts
    B, P, T = 5, 88, 1100
    thr, othr = 0.7, 0.3
    frame, onset = _case(B, P, T, thr, othr, seed=41)
    x = torch.from_numpy(frame).cuda()
    on = torch.from_numpy(onset).cuda() if decoder == "onset" else None
    for lengths in (None, [1100, 0, 65, 1107, 700]):
        counts, _, _, _ = _batch(x, on, thr, othr, lengths)
        m = note_match_counts(x, torch.zeros_like(x), thr, on, othr, lengths).cpu().numpy()
        assert np.array_equal(counts.reshape(B, P).sum(1), m[:, 1]) and m[:, 1].sum() > 0


# ------------------------------------------------------------------ 5. 64-bit indexing
def test_rows_past_2g_floats(mta):
    """(2, 1, 2^30 + 64) logits: row 1 starts 4 GiB into the buffer.  Three runs in its last 200 frames, the last one running into
    lengths[1] = T - 5 (the five padding frames behind it are active and must not be read)."""
    T = (1 << 30) + 64
    x = torch.full((2, 1, T), -1.0, device="cuda")
    x[1, 0, T - 190:T - 180] = 2.0
    x[1, 0, T - 100:T - 99] = 2.0
    x[1, 0, T - 20:] = 2.0
    x[0, 0, 100:110] = 2.0                                   # past lengths[0]: not a note
    counts, row_off, s, e = _batch(x, None, 0.5, 0.5, [100, T - 5], capacity=16)
    assert counts.tolist() == [0, 3] and row_off.tolist() == [0, 0, 3]
    assert s[:3].tolist() == [T - 190, T - 100, T - 20] and e[:3].tolist() == [T - 180, T - 99, T - 5]
    assert (s[3:] == SENTINEL).all() and (e[3:] == SENTINEL).all()
    del x
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. notes_batch_device
@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_notes_batch_device_equals_the_per_recording_functions(mta, decoder, monkeypatch):
    from music_transcription_amd import notes as N, transcribe as tr
    B, P, T = 4, 88, 700
    thr, othr = 0.5, 0.7
    frame, onset = _case(B, P, T, thr, othr, seed=61)
    x = torch.from_numpy(frame).cuda()
    on = torch.from_numpy(onset).cuda() if decoder == "onset" else None
    lengths = [700, 1, 333, 64]
    fs = 16000 / 512

    def per_recording(b, L):
        if on is None:
            return tr.notes_from_logits_device(x[b:b + 1, :, :L].contiguous(), thr, fs)
        return N.heads_to_notes_device(x[b:b + 1, :, :L].contiguous(), on[b:b + 1, :, :L].contiguous(), thr, othr, fs)

    for ln in (None, lengths, torch.tensor(lengths)):
        got = mta.notes_batch_device(x, on, thr, othr, ln, fs)
        want = [per_recording(b, L) for b, L in enumerate(_clamp(None if ln is None else lengths, B, T))]
        assert got == want and sum(len(w) for w in want) > 100

    # many short notes: the first capacity guess (B * T / 16) is too small -> exactly one more launch, same notes
    x2 = torch.full((2, 88, 600), -3.0, device="cuda")
    x2[:, :, ::2] = 3.0
    on2 = x2.clone() if decoder == "onset" else None
    calls = []
    real = N.lib.mt_notes_batch
    monkeypatch.setattr(N.lib, "mt_notes_batch", lambda *a: (calls.append(a[12]), real(*a))[1])
    got = N.notes_batch_device(x2, on2, 0.5, 0.5, [600, 599], fs, min_midi=0)
    assert len(calls) == 2 and calls[0] < calls[1] == 88 * 600
    assert [len(g) for g in got] == [88 * 300, 88 * 300]
    assert got[1][:3] == [(0, 0.0, 1 / fs), (0, 2 / fs, 3 / fs), (0, 4 / fs, 5 / fs)] and got[1][-1] == (87, 598 / fs, 599 / fs)


def test_bad_arguments_are_refused(mta):
    from music_transcription_amd import _lib
    x = torch.zeros(1, 88, 10, device="cuda")
    c = torch.zeros(88, dtype=torch.int32, device="cuda")
    off = torch.zeros(89, dtype=torch.int64, device="cuda")
    s = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    good = [p(x), None, 0.5, 0.5, None, 1, 88, 10, p(c), p(off), p(s), p(s), 8, _lib.stream_ptr()]
    assert _lib.lib.mt_notes_batch(*good) == 0
    for k, bad in [(2, 0.0), (2, 1.0), (5, 0), (6, 0), (7, 0), (7, -3), (12, -1), (0, None), (8, None), (9, None), (10, None)]:
        args = list(good)
        args[k] = bad
        assert _lib.lib.mt_notes_batch(*args) != 0, (k, bad)
        assert "mt_notes_batch" in _lib.last_error()
    args = list(good)
    args[1], args[3] = p(x), 1.5                             # the onset threshold counts once there are onset logits
    assert _lib.lib.mt_notes_batch(*args) != 0
    with pytest.raises(ValueError):
        mta.notes_batch_device(x, None, 1.0)
    torch.cuda.synchronize()
