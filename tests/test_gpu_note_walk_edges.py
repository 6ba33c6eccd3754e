"""The edges that the shared row walk of csrc/note_decode.h (walk_slabs) owns for every note kernel, on one padded batch: the
512-frame slab edge of notes.hip, the 1024-frame slab edge of notes_batch.hip and each recording's last valid frame, with notes
planted to start, end, be re-struck and be cut by the offset head exactly there, and a padding of strongly active logits that
must have no effect.  Every entry point is compared exactly with the pure-Python references of this directory; a test without
the gpu mark checks that the references' own note lists do sit on those edges."""
import numpy as np
import pytest
import torch

import note_list_ref as LR
import note_metrics_ref as NR
import offset_decode_ref as OR

B, P, T = 6, 3, 1025                                           # P = 3: the last workgroup of four waves is half empty
LENGTHS = [511, 512, 513, 1023, 1024, 1025]
EDGES = (512, 1024)
THR, OTHR, KTHR = 0.3, 0.5, 0.7


def _plant(act, b, p, lo, hi, frame=(), onset=(), offset=()):
    """Rows (b, p) of the three heads: inactive on [lo - 2, hi + 2), then active on the listed frames (all clipped to the row)."""
    for a, on in zip(act, (frame, onset, offset)):
        a[b, p, max(lo - 2, 0):min(hi + 2, T)] = False
        a[b, p, [t for t in on if 0 <= t < T]] = True


def _build():
    rng = np.random.default_rng(2024)
    shape = (B, P, T)
    ref = OR.markov(rng, shape, 0.06, 0.2)
    est = np.roll(ref, 1, axis=2) ^ (rng.random(shape) < 0.03)
    prev = np.concatenate([np.zeros((B, P, 1), bool), est[..., :-1]], axis=2)
    ons = ((est & ~prev) & (rng.random(shape) > 0.1)) | (est & (rng.random(shape) < 0.04)) | (rng.random(shape) < 0.005)
    nxt = np.concatenate([est[..., 1:], np.zeros((B, P, 1), bool)], axis=2)
    offs = (est & ~nxt & (rng.random(shape) > 0.1)) | (rng.random(shape) < 0.01)
    act = (est, ons, offs)
    for b, L in enumerate(LENGTHS):
        for p in range(P):
            # a note that starts 6 frames before the row's last valid frame and runs into the padding: it ends at L
            _plant(act, b, p, L - 6, L, frame=range(L - 6, L), onset=[L - 6])
        for X in EDGES:
            if X >= L:
                continue
            # pitch 0: a frame run across X - 1 | X, struck at X - 7 and struck again exactly at X (a note ends and one starts at X)
            _plant(act, b, 0, X - 7, X + 8, frame=range(X - 7, X + 8), onset=[X - 7, X])
            # pitch 1: the same run, struck once, and an offset edge at X - 1: its cut lands on X, the next slab's first frame (e_prev)
            _plant(act, b, 1, X - 7, X + 8, frame=range(X - 7, X + 8), onset=[X - 7], offset=[X - 1])
    mag = lambda: rng.uniform(0.01, 4.0, size=shape)
    frame = np.where(est, OR.logit(THR) + mag(), OR.logit(THR) - mag()).astype(np.float32)
    onset = np.where(ons, OR.logit(OTHR) + mag(), OR.logit(OTHR) - mag()).astype(np.float32)
    offset = np.where(offs, OR.logit(KTHR) + mag(), OR.logit(KTHR) - mag()).astype(np.float32)
    for b, L in enumerate(LENGTHS):                            # the padding: strongly active on all heads and in the roll
        for a in act + (ref, frame, onset, offset):
            a[b, :, L:] = 8.0 if a.dtype == np.float32 else True
    assert (NR.sigmoid_active(frame, THR) == est).all() and (NR.sigmoid_active(onset, OTHR) == ons).all()
    assert (NR.sigmoid_active(offset, KTHR) == offs).all()
    c = dict(frame=frame, onset=onset, offset=offset, ref=ref.astype(np.float32), act=act, notes=LR.notes_from_roll(ref))
    for a in (c["frame"], c["onset"], c["offset"], c["ref"]) + act + c["notes"]:
        a.setflags(write=False)
    return c


_CASE = {}


def _case():
    """Built once, shared by every test here; nobody writes to it."""
    if not _CASE:
        _CASE.update(_build())
    return _CASE


def _row_notes(c, b, decoder):
    """[(pitch, start, end)] of recording b trimmed to its length, pitch-major: the reference's note list."""
    est, ons, offs = c["act"]
    L = LENGTHS[b]
    out = []
    for p in range(P):
        f, o, k = est[b, p, :L], ons[b, p, :L], offs[b, p, :L]
        notes = NR.frame_notes(f) if decoder == "frame" else NR.onset_notes(f, o) if decoder == "onset" else OR.onset_offset_notes(f, o, k)
        out += [(p, int(s), int(e)) for s, e in notes]
    return out


def test_the_references_sit_on_the_edges():
    """Non-vacuity, on the references alone: notes start at 512 and 1024, offset-gated notes have 511 and 1023 as their last frame
    where the onset-gated note runs on, and in every recording and decoder a note ends at exactly lengths[b]."""
    c = _case()
    lists = {d: [_row_notes(c, b, d) for b in range(B)] for d in ("frame", "onset", "onset_offset")}
    for d in ("onset", "onset_offset"):
        starts = {s for rec in lists[d] for _, s, _ in rec}
        assert set(EDGES) <= starts, (d, sorted(starts))
    for X in EDGES:
        cut = [(b, n) for b in range(B) for n in lists["onset_offset"][b] if n[0] == 1 and n[2] == X]
        assert cut and all((1, n[1], min(X + 8, LENGTHS[b])) in lists["onset"][b] for b, n in cut), (X, cut)
        assert any((p, s, e) for rec in lists["frame"] for p, s, e in rec if s < X < e)                  # frame runs across X - 1 | X
    for d, recs in lists.items():
        for b, rec in enumerate(recs):
            assert any(e == LENGTHS[b] for _, _, e in rec), (d, b)
            assert all(e <= LENGTHS[b] for _, _, e in rec), (d, b)


@pytest.fixture(scope="module")
def dev():
    import music_transcription_amd  # noqa: F401  (loads the library)
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = _case()
    t = {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("frame", "onset", "offset", "ref")}
    t["notes"] = {k: torch.from_numpy(np.array(v)).cuda() for k, v in zip(("on", "off", "ptr"), c["notes"])}
    return t


@pytest.mark.gpu
def test_roll_counts(dev):
    from music_transcription_amd.notes import note_match_counts
    c = _case()
    est, ons, offs = c["act"]
    x, o, k, r = dev["frame"], dev["onset"], dev["offset"], dev["ref"]
    np.testing.assert_array_equal(note_match_counts(x, r, THR, None, 0.5, LENGTHS).cpu().numpy(), NR.match_counts_active(est, c["ref"], None, LENGTHS))
    np.testing.assert_array_equal(note_match_counts(x, r, THR, o, OTHR, LENGTHS).cpu().numpy(), NR.match_counts_active(est, c["ref"], ons, LENGTHS))
    np.testing.assert_array_equal(note_match_counts(x, r, THR, o, OTHR, LENGTHS, offset_logits=k, offset_threshold=KTHR).cpu().numpy(),
                                  OR.match_counts_active(est, ons, offs, c["ref"], LENGTHS))


@pytest.mark.gpu
def test_list_counts(dev):
    from music_transcription_amd.notes import note_match_list
    c = _case()
    est, ons, offs = c["act"]
    x, o, k, notes = dev["frame"], dev["onset"], dev["offset"], dev["notes"]
    np.testing.assert_array_equal(note_match_list(x, notes, THR, None, 0.5, LENGTHS).cpu().numpy(),
                                  LR.match_list_counts_active(est, *c["notes"], None, LENGTHS))
    np.testing.assert_array_equal(note_match_list(x, notes, THR, o, OTHR, LENGTHS).cpu().numpy(),
                                  LR.match_list_counts_active(est, *c["notes"], ons, LENGTHS))
    np.testing.assert_array_equal(note_match_list(x, notes, THR, o, OTHR, LENGTHS, offset_logits=k, offset_threshold=KTHR).cpu().numpy(),
                                  OR.match_list_counts_active(est, ons, offs, *c["notes"], LENGTHS))


@pytest.mark.gpu
def test_note_lists_per_recording(dev):
    """mt_heads_to_notes and _off on each recording's trimmed rows as one chunk (NB = 1)."""
    from music_transcription_amd.notes import heads_to_notes_device
    c = _case()
    for b, L in enumerate(LENGTHS):
        x, o, k = (dev[h][b:b + 1, :, :L].contiguous() for h in ("frame", "onset", "offset"))
        assert heads_to_notes_device(x, o, THR, OTHR, fs=1.0, min_midi=0) == _row_notes(c, b, "onset")
        assert heads_to_notes_device(x, o, THR, OTHR, fs=1.0, min_midi=0, offset_logits=k, offset_threshold=KTHR) == _row_notes(c, b, "onset_offset")


@pytest.mark.gpu
def test_note_lists_with_a_chunk_boundary_inside_a_slab(dev):
    """NB = 2, T = 513: the chunks concatenated in time put their boundary at frame 513, inside the second slab."""
    from music_transcription_amd.notes import heads_to_notes_device
    est, ons, offs = (a[4:6, :, :513] for a in _case()["act"])
    x, o, k = (dev[h][4:6, :, :513].contiguous() for h in ("frame", "onset", "offset"))
    want = [(p, s, e) for p in range(P) for s, e in NR.onset_notes(est[:, p].reshape(-1), ons[:, p].reshape(-1))]
    assert heads_to_notes_device(x, o, THR, OTHR, fs=1.0, min_midi=0) == want
    assert heads_to_notes_device(x, o, THR, OTHR, fs=1.0, min_midi=0, offset_logits=k, offset_threshold=KTHR) == OR.heads_notes_active(est, ons, offs)


@pytest.mark.gpu
def test_notes_batch(dev):
    from music_transcription_amd.notes import notes_batch_device
    c = _case()
    assert notes_batch_device(dev["frame"], None, THR, 0.5, LENGTHS, fs=1.0, min_midi=0) == [_row_notes(c, b, "frame") for b in range(B)]
    assert notes_batch_device(dev["frame"], dev["onset"], THR, OTHR, LENGTHS, fs=1.0, min_midi=0) == [_row_notes(c, b, "onset") for b in range(B)]
