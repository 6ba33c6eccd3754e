"""Note cleanup in the decoders on the GPU (csrc/note_decode.h clean_step, the mt_*_clean entry points, notes.py; DESIGN.md 6c "Note cleanup") against
the literal scan of note_clean_ref.py, with scipy's maximum matching for the counts: hand-built rows on the window / slab / length
boundaries, random rows for the three decoders, the cleaning kernels against the old ones at (1, 0), the C ABI's refusals and the
command lines.  Everything is integer logic on thresholded activity, so every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import note_clean_ref as CR
import offset_decode_ref as OR
from oracle import model_ref as R
from test_gpu_note_list import _random_list
from test_gpu_offset_decoder import _midi_notes, _mid_threshold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FS = 16000 / 512
P, T = 5, 1100                                      # 5 rows: no multiple of the 4 per workgroup; 1100 frames: past both slabs (512, 1024)
LENGTHS = [1100, 1025, 1024, 1023, 513, 512, 511, 65, 64, 63, 1, 0]
HI, LO = OR.logit(0.5 + 0.2), OR.logit(0.5 - 0.2)   # logits of active / inactive cells at threshold 0.5
PAIRS = [(1, 0), (2, 0), (1, 1), (3, 2), (64, 63)]
DECODERS = ["frame", "onset", "onset_offset"]


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _logits(act):
    return torch.from_numpy(np.where(np.asarray(act, bool), HI, LO).astype(np.float32)).cuda()


def _dev_notes(on, off, ptr):
    return {"on": torch.from_numpy(np.asarray(on, np.int32)).cuda(), "off": torch.from_numpy(np.asarray(off, np.int32)).cuda(),
            "ptr": torch.from_numpy(np.asarray(ptr, np.int64)).cuda()}


def _heads_of(decoder, f, o, k):
    return f, (o if decoder != "frame" else None), (k if decoder == "onset_offset" else None)


# ------------------------------------------------------------------------------------------------ the entry points, called directly
def _raw():
    from music_transcription_amd import _lib
    return _lib.lib, _lib.ptr, _lib.stream_ptr


def raw_match(x, on, off, ref, lengths, M, G):
    lib, ptr, stream = _raw()
    B, Pn, Tn = x.shape
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    rc = lib.mt_note_match_counts_clean(ptr(x), ptr(on), ptr(off), 0.5, 0.5, 0.5, ptr(ref), ptr(ln), ptr(counts), B, Pn, Tn, M, G, stream())
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy()


def raw_list(x, on, off, notes, lengths, M, G):
    lib, ptr, stream = _raw()
    B, Pn, Tn = x.shape
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
    rc = lib.mt_note_match_list_clean(ptr(x), ptr(on), ptr(off), 0.5, 0.5, 0.5, ptr(notes["on"]), ptr(notes["off"]), ptr(notes["ptr"]), ptr(ln),
                                      ptr(counts), B, Pn, Tn, M, G, stream())
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy()


def raw_heads(x, on, off, M, G, cap=1 << 16):
    """-> rc, [(pitch index, start, end)], and the raw buffers (for the refusals)."""
    lib, ptr, stream = _raw()
    NB, Pn, Tn = x.shape
    counts = torch.full((Pn,), -7, dtype=torch.int32, device="cuda")
    starts, ends = torch.full((cap,), -7, dtype=torch.int32, device="cuda"), torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    rc = lib.mt_heads_to_notes_clean(ptr(x), ptr(on), ptr(off), 0.5, 0.5, 0.5, NB, Pn, Tn, ptr(counts), ptr(starts), ptr(ends), cap, M, G, stream())
    torch.cuda.synchronize()
    c, s, e = counts.cpu().numpy(), starts.cpu().numpy(), ends.cpu().numpy()
    notes = []
    if rc == 0:
        assert c.sum() <= cap
        notes = [(int(p), int(a), int(b)) for p, a, b in zip(np.repeat(np.arange(Pn), c), s[:c.sum()], e[:c.sum()])]
        assert (s[c.sum():] == -7).all() and (e[c.sum():] == -7).all()          # nothing written past the notes
    return rc, notes, (c, s, e)


def raw_batch(x, on, lengths, M, G, cap=1 << 17):
    lib, ptr, stream = _raw()
    B, Pn, Tn = x.shape
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
    counts = torch.full((B * Pn,), -7, dtype=torch.int32, device="cuda")
    row_off = torch.full((B * Pn + 1,), -7, dtype=torch.int64, device="cuda")
    se = torch.full((2, cap), -7, dtype=torch.int32, device="cuda")
    rc = lib.mt_notes_batch_clean(ptr(x), ptr(on), 0.5, 0.5, ptr(ln), B, Pn, Tn, ptr(counts), ptr(row_off), ptr(se[0]), ptr(se[1]), cap, M, G,
                                  stream())
    torch.cuda.synchronize()
    c, ro, s, e = counts.cpu().numpy(), row_off.cpu().numpy(), se[0].cpu().numpy(), se[1].cpu().numpy()
    out = []
    if rc == 0:
        assert ro[-1] <= cap and (np.diff(ro) == c).all()
        assert (s[ro[-1]:] == -7).all() and (e[ro[-1]:] == -7).all()
        for b in range(B):
            out.append([(p, int(s[i]), int(e[i])) for p in range(Pn) for i in range(ro[b * Pn + p], ro[b * Pn + p + 1])])
    return rc, out, (c, ro, s, e)


# ------------------------------------------------------------------------------------------------ random rows
_RANDOM = {}


def _random_case():
    """Markov rows with short runs, so that every 64-frame window carries events; built once, nobody writes to it."""
    if not _RANDOM:
        rng = np.random.default_rng(2024)
        B = len(LENGTHS)
        f = OR.markov(rng, (B, P, T), 0.25, 0.3)
        o = OR.markov(rng, (B, P, T), 0.08, 0.6)
        k = OR.markov(rng, (B, P, T), 0.06, 0.6)
        ref = OR.markov(rng, (B, P, T), 0.1, 0.2)
        f[0, 0] = OR.markov(rng, (T,), 0.01, 0.01)                               # and a row of long runs and long gaps
        o[:2, 0], k[:2, 0] = OR.markov(rng, (2, T), 0.004, 0.6), OR.markov(rng, (2, T), 0.003, 0.6)     # few onsets: notes past 64 frames
        r_on, r_off, r_ptr = _random_list(rng, f, o, T)                          # with re-struck keys, equal onsets, empty and crowded rows
        for a in (f, o, k, ref):
            a.setflags(write=False)
        _RANDOM.update(f=f, o=o, k=k, ref=ref, list=(r_on, r_off, r_ptr),
                       dev=dict(f=_logits(f), o=_logits(o), k=_logits(k), ref=torch.from_numpy(ref.astype(np.float32)).cuda(),
                                list=_dev_notes(r_on, r_off, r_ptr)))
    return _RANDOM


@pytest.mark.parametrize("M,G", PAIRS)
@pytest.mark.parametrize("decoder", DECODERS)
def test_random_rows_equal_the_reference(mta, decoder, M, G):
    c = _random_case()
    d = c["dev"]
    f, o, k = _heads_of(decoder, c["f"], c["o"], c["k"])
    x, on, off = _heads_of(decoder, d["f"], d["o"], d["k"])
    for lengths in (LENGTHS, None):
        rc, got = raw_match(x, on, off, d["ref"], lengths, M, G)
        want = CR.match_counts_active(f, c["ref"], o, k, lengths, M, G)
        assert rc == 0 and np.array_equal(got, want), (lengths, got, want)
        rc, got = raw_list(x, on, off, d["list"], lengths, M, G)
        want_l = CR.match_list_counts_active(f, *c["list"], o, k, lengths, M, G)
        assert rc == 0 and np.array_equal(got, want_l), (lengths, got, want_l)
    assert want[:, 1].sum() > 0 and (M == 64 or (want[:, 2].sum() > 0 and want_l[:, 2].sum() > 0))      # notes survive, and match
    for sl in (slice(0, T), slice(0, 1024)):                                     # chunks of 1100 and of 1024 frames, concatenated
        cut = lambda a: None if a is None else a[:2, :, sl]
        dcut = lambda a: None if a is None else a[:2, :, sl].contiguous()
        rc, got, _ = raw_heads(dcut(x), dcut(on), dcut(off), M, G)
        assert rc == 0 and got == CR.heads_notes_active(cut(f), cut(o), cut(k), M, G)
    if decoder != "onset_offset":
        for lengths in (LENGTHS, None):
            rc, got, _ = raw_batch(x, on, lengths, M, G)
            assert rc == 0 and got == CR.batch_notes_active(f, o, lengths, M, G)
    if (M, G) != (1, 0):                                                         # the inputs do exercise the stage
        assert not np.array_equal(want, CR.match_counts_active(f, c["ref"], o, k, None, 1, 0))


# ------------------------------------------------------------------------------------------------ constructed rows
BOUNDARIES = (64, 512, 1024)


def _scene(L=T, runs=(), onsets=None, offsets=(), beyond=True):
    """One row: f active on the runs [s, e); o active on one frame at each of `onsets` (None: at the start of every run); k active on
    one frame at each of `offsets`.  With `beyond`, all three heads are active from L on: frames that must never be read."""
    f, o, k = np.zeros(T, bool), np.zeros(T, bool), np.zeros(T, bool)
    for s, e in runs:
        f[max(0, s):e] = True
    for t in ([max(0, s) for s, _ in runs] if onsets is None else onsets):
        o[min(t, T - 1)] = True
    for t in offsets:
        k[min(t, T - 1)] = True
    if beyond:
        f[L:] = o[L:] = k[L:] = True
    return dict(L=L, f=f, o=o, k=k)


def _scenes(M, G):
    """The rows for one (M, G), at each of the three boundaries."""
    out = []
    for bd in BOUNDARIES:
        for n in (G, G + 1):                                                    # a gap of exactly G and of G + 1 frames ...
            if n == 0:
                continue
            for gs in (bd - n, bd - max(1, n // 2), bd):                        # ... ending on, straddling and starting on the boundary
                if gs < 1:
                    continue
                runs = [(gs - 5, gs), (gs + n, gs + n + 5)]
                out.append(_scene(runs=runs))
                out.append(_scene(runs=runs, onsets=[max(0, gs - 5)]))           # one onset: the bridged note carries on
        for n in (M - 1, M):                                                    # a note of M - 1 and of M frames from the last frame before
            if n >= 1:
                out.append(_scene(runs=[(bd - 1, bd - 1 + n)]))
                out.append(_scene(runs=[(bd - 1, bd - 1 + n), (bd + n + 2, bd + n + 4)]))
        n = max(1, M - 1)
        out.append(_scene(runs=[(bd - n, bd + 10)], onsets=[bd - n, bd]))       # a short note closed by a re-strike
        out.append(_scene(runs=[(bd - 1, bd + 10)], offsets=[bd - 2 + n]))      # a short note cut by an offset edge
        out.append(_scene(runs=[(bd - 1, bd + 10)], offsets=[bd - 1 + n]))      # (and one frame longer)
        for L in (bd, bd + 1):                                                  # a note still open at L, short and just long enough
            out.append(_scene(L=L, runs=[(L - n, L)]))
            out.append(_scene(L=L, runs=[(L - n - 1, L)]))
        g = max(1, G)
        out.append(_scene(L=bd, runs=[(bd - 10 - g, bd - g)]))                  # a gap that reaches L
        out.append(_scene(L=bd + 1, runs=[(bd - 10 - g, bd + 1 - g)]))
        out.append(_scene(runs=[(g, bd + 3)]))                                  # a leading gap
        out.append(_scene(runs=[(bd - 6, bd - 1), (bd - 1 + g + 1, bd + g + 6)], onsets=[bd - 6, bd]))        # an onset edge inside the gap
        out.append(_scene(runs=[(bd - 6, bd - 1), (bd - 1 + g, bd + g + 6)], onsets=[bd - 6], offsets=[bd - 2]))   # an offset edge before it
        out.append(_scene(runs=[(bd - n, bd), (bd + g + 1, bd + g + 1 + n), (bd + g + n + 5, bd + g + n + 5 + 70)]))   # two short notes
        out.append(_scene(runs=[(bd - n, bd), (bd + g, bd + g + n)]))           # a bridge that makes one note of two short ones
    return out


CONSTRUCTED = [(1, 1), (1, 2), (1, 63), (2, 0), (3, 0), (64, 0), (3, 2), (5, 1), (64, 63)]


@pytest.mark.parametrize("M,G", CONSTRUCTED)
def test_constructed_rows(mta, M, G):
    sc = _scenes(M, G)
    lengths = [s["L"] for s in sc]
    stack = lambda key: np.repeat(np.stack([s[key] for s in sc])[:, None, :], P, axis=1)          # the same row on all five pitches,
    f, o, k = stack("f"), stack("o"), stack("k")                                                 # so the reference scans one of them
    ref = np.roll(f, 1, axis=2)
    one = lambda v: None if v is None else v[:, :1]
    on_all = lambda notes: [(p, s, e) for p in range(P) for _, s, e in notes]
    xf, xo, xk, xr = _logits(f), _logits(o), _logits(k), torch.from_numpy(ref.astype(np.float32)).cuda()
    changed = 0
    for decoder in DECODERS:
        a, b, c = _heads_of(decoder, f, o, k)
        x, on, off = _heads_of(decoder, xf, xo, xk)
        rc, got = raw_match(x, on, off, xr, lengths, M, G)
        want = P * CR.match_counts_active(one(a), one(ref), one(b), one(c), lengths, M, G)
        assert rc == 0 and np.array_equal(got, want), (decoder, np.nonzero((got != want).any(1))[0])
        changed += int(not np.array_equal(want, P * CR.match_counts_active(one(a), one(ref), one(b), one(c), lengths, 1, 0)))
        if decoder != "onset_offset":
            rc, got, _ = raw_batch(x, on, lengths, M, G)
            want = [on_all(rec) for rec in CR.batch_notes_active(one(a), one(b), lengths, M, G)]
            assert rc == 0 and got == want, (decoder, [n for n in range(len(sc)) if got[n] != want[n]])
        for n, s in enumerate(sc):                                              # every row alone, trimmed to its length: the note list
            cut = lambda v: None if v is None else v[n:n + 1, :, :s["L"]].contiguous()
            rc, got, _ = raw_heads(cut(x), cut(on), cut(off), M, G, cap=4096)
            want = on_all(CR.heads_notes_active(*(None if v is None else v[n:n + 1, :1, :s["L"]] for v in (a, b, c)), M, G))
            assert rc == 0 and got == want, (decoder, n, got[:6], want[:6])
    assert changed == 3


def test_constructed_rows_do_what_they_are_named_for():
    """On the reference alone: the rows above do bridge, drop and keep what their comments say."""
    bd = 512
    notes = lambda s, dec, M, G: CR.clean_notes(*_heads_of(dec, s["f"][:s["L"]], s["o"][:s["L"]], s["k"][:s["L"]]), M, G)
    gap = _scene(runs=[(bd - 7, bd - 2), (bd, bd + 5)])
    assert notes(gap, "frame", 1, 2) == [(bd - 7, bd + 5)] and notes(gap, "frame", 1, 1) == [(bd - 7, bd - 2), (bd, bd + 5)]
    assert notes(gap, "onset", 1, 2) == [(bd - 7, bd), (bd, bd + 5)]             # the onset edge still splits
    one = _scene(runs=[(bd - 7, bd - 2), (bd, bd + 5)], onsets=[bd - 7])
    assert notes(one, "onset", 1, 2) == [(bd - 7, bd + 5)] and notes(one, "onset", 1, 0) == [(bd - 7, bd - 2)]
    re = _scene(runs=[(bd - 2, bd + 10)], onsets=[bd - 2, bd])
    assert notes(re, "onset", 3, 0) == [(bd, bd + 10)]                           # the survivor is not extended
    cut = _scene(runs=[(bd - 1, bd + 10)], offsets=[bd])
    assert notes(cut, "onset_offset", 3, 0) == [] and notes(cut, "onset_offset", 2, 0) == [(bd - 1, bd + 1)]
    for L in (bd, bd + 1):
        end = _scene(L=L, runs=[(L - 2, L)])
        assert notes(end, "frame", 3, 0) == [] and notes(end, "frame", 2, 0) == [(L - 2, L)]
    assert notes(_scene(L=bd, runs=[(bd - 12, bd - 2)]), "frame", 1, 2) == [(bd - 12, bd - 2)]
    assert notes(_scene(runs=[(2, bd)]), "frame", 1, 2) == [(2, bd)]
    before = _scene(runs=[(bd - 6, bd - 1), (bd + 1, bd + 8)], onsets=[bd - 6], offsets=[bd - 2])
    assert notes(before, "onset_offset", 1, 2) == [(bd - 6, bd - 1)]             # the offset edge cuts through the bridged gap
    two = _scene(runs=[(bd - 2, bd), (bd + 1, bd + 3)])
    assert notes(two, "frame", 3, 0) == [] and notes(two, "frame", 3, 1) == [(bd - 2, bd + 3)]


# ------------------------------------------------------------------------------------------------ old against new at (1, 0)
@pytest.mark.parametrize("decoder", DECODERS)
def test_the_cleaning_kernels_at_1_0_return_what_the_old_ones_return(mta, decoder):
    from music_transcription_amd.notes import heads_to_notes_device, note_match_counts, note_match_list, notes_batch_device
    from music_transcription_amd.transcribe import notes_from_logits_device
    d = _random_case()["dev"]
    x, on, off = _heads_of(decoder, d["f"], d["o"], d["k"])
    for lengths in (LENGTHS, None):
        rc, got = raw_match(x, on, off, d["ref"], lengths, 1, 0)
        assert rc == 0 and np.array_equal(got, note_match_counts(x, d["ref"], 0.5, on, 0.5, lengths, off, 0.5).cpu().numpy())
        rc, got = raw_list(x, on, off, d["list"], lengths, 1, 0)
        assert rc == 0 and np.array_equal(got, note_match_list(x, d["list"], 0.5, on, 0.5, lengths, off, 0.5).cpu().numpy())
    rc, got, _ = raw_heads(x[:2].contiguous(), None if on is None else on[:2].contiguous(), None if off is None else off[:2].contiguous(), 1, 0)
    old = notes_from_logits_device(x[:2], 0.5, 1.0, 0) if on is None else heads_to_notes_device(x[:2], on[:2], 0.5, 0.5, 1.0, 0, off if off is None else off[:2])
    assert rc == 0 and len(got) > 0 and got == [(p, int(s), int(e)) for p, s, e in old]
    if decoder != "onset_offset":
        rc, got, _ = raw_batch(x, on, LENGTHS, 1, 0)
        assert rc == 0 and got == [[(p, int(s), int(e)) for p, s, e in rec] for rec in notes_batch_device(x, on, 0.5, 0.5, LENGTHS, 1.0, 0)]


class _Spy:
    """Stands in for the loaded library: passes every call on and keeps the names (once for a call repeated with larger buffers)."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        if self.calls[-1:] != [name]:
            self.calls.append(name)
        return getattr(self.lib, name)


def test_python_calls_the_old_entry_points_at_the_defaults_and_the_cleaning_ones_otherwise(mta, monkeypatch):
    from music_transcription_amd import notes as N, transcribe as tr
    c = _random_case()
    d = c["dev"]
    spy = _Spy(N.lib)
    monkeypatch.setattr(N, "lib", spy)
    monkeypatch.setattr(tr, "lib", spy)
    x, on, off = d["f"], d["o"], d["k"]
    N.note_match_counts(x, d["ref"], 0.5, on, 0.5, LENGTHS)
    N.note_match_counts(x, d["ref"], 0.5, on, 0.5, LENGTHS, off, 0.5, min_note_frames=1, bridge_frames=0)
    N.note_match_list(x, d["list"], 0.5)
    N.note_match_list(x, d["list"], 0.5, on, 0.5, None, off)
    N.heads_to_notes_device(x[:2], on[:2])
    N.heads_to_notes_device(x[:2], on[:2], offset_logits=off[:2])
    N.notes_batch_device(x, None, lengths=LENGTHS)
    tr.notes_from_logits_device(x[:2])
    assert spy.calls == ["mt_note_match_counts", "mt_note_match_counts_off", "mt_note_match_list", "mt_note_match_list_off", "mt_heads_to_notes",
                         "mt_heads_to_notes_off", "mt_notes_batch", "mt_roll_to_notes"]
    del spy.calls[:]
    f, o, k = c["f"], c["o"], c["k"]
    got = N.note_match_counts(x, d["ref"], 0.5, on, 0.5, LENGTHS, off, 0.5, min_note_frames=3, bridge_frames=2).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, CR.match_counts_active(f, c["ref"], o, k, LENGTHS, 3, 2))
    got = N.note_match_list(x, d["list"], 0.5, None, 0.5, LENGTHS, min_note_frames=2).cpu().numpy()
    assert np.array_equal(got, CR.match_list_counts_active(f, *c["list"], None, None, LENGTHS, 2, 0))
    got = N.heads_to_notes_device(x[:2], on[:2], 0.5, 0.5, 1.0, 0, bridge_frames=1)
    assert got == [(p, float(s), float(e)) for p, s, e in CR.heads_notes_active(f[:2], o[:2], None, 1, 1)]
    assert spy.calls[-1] == "mt_heads_to_notes_clean" and "mt_roll_to_notes" not in spy.calls
    got = tr.notes_from_logits_device(x[:2], 0.5, 1.0, 0, min_note_frames=3, bridge_frames=2)
    assert got == [(p, float(s), float(e)) for p, s, e in CR.heads_notes_active(f[:2], None, None, 3, 2)]
    got = N.notes_batch_device(x, on, 0.5, 0.5, LENGTHS, 1.0, 0, min_note_frames=64, bridge_frames=63)
    assert got == [[(p, float(s), float(e)) for p, s, e in rec] for rec in CR.batch_notes_active(f, o, LENGTHS, 64, 63)]
    assert spy.calls == ["mt_note_match_counts_clean", "mt_note_match_list_clean", "mt_heads_to_notes_clean", "mt_notes_batch_clean"]
    del spy.calls[:]
    for kw in (dict(min_note_frames=0), dict(min_note_frames=65), dict(bridge_frames=-1), dict(bridge_frames=64), dict(min_note_frames=2.0)):
        for call in (lambda: N.note_match_counts(x, d["ref"], **kw), lambda: N.note_match_list(x, d["list"], **kw),
                     lambda: N.heads_to_notes_device(x[:2], on[:2], **kw), lambda: N.notes_batch_device(x, **kw),
                     lambda: tr.notes_from_logits_device(x[:2], **kw)):
            with pytest.raises(ValueError, match="min_note_frames|bridge_frames"):
                call()
    assert spy.calls == []                                                       # refused before any GPU work


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_c_abi_refusals_leave_the_outputs_alone(mta):
    d = _random_case()["dev"]
    x, on, off = d["f"], d["o"], d["k"]
    bad = [(0, 0), (65, 0), (1, -1), (1, 64)]
    for heads in ((x, on, off), (x, on, None), (x, None, None)):
        for M, G in bad:
            rc, got = raw_match(*heads, d["ref"], LENGTHS, M, G)
            assert rc != 0 and (got == -7).all()
            rc, got = raw_list(*heads, d["list"], LENGTHS, M, G)
            assert rc != 0 and (got == -7).all()
            rc, _, bufs = raw_heads(*(None if h is None else h[:2].contiguous() for h in heads), M, G, cap=4096)
            assert rc != 0 and all((b == -7).all() for b in bufs)
            if heads[2] is None:
                rc, _, bufs = raw_batch(heads[0], heads[1], LENGTHS, M, G, cap=4096)
                assert rc != 0 and all((b == -7).all() for b in bufs)
    rc, got = raw_match(x, None, off, d["ref"], LENGTHS, 2, 1)                   # an offset head without an onset head
    assert rc != 0 and (got == -7).all()
    rc, got = raw_list(x, None, off, d["list"], LENGTHS, 2, 1)
    assert rc != 0 and (got == -7).all()
    rc, _, bufs = raw_heads(x[:2].contiguous(), None, off[:2].contiguous(), 2, 1, cap=4096)
    assert rc != 0 and all((b == -7).all() for b in bufs)
    from music_transcription_amd import _lib
    assert "min_frames" in _lib.last_error() or "bad arguments" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ end to end
NM, H, NL = 32, 16, 2
MODEL_FLAGS = ["--model-type", "cnn_rnn_large", "--n-mels", str(NM), "--hidden-size", str(H), "--num-layers", str(NL)]
TICK = lambda t: int(round(t * 220 * 120.0 / 60.0))                               # transcribe.write_midi's ticks


def _large(mta, n_mels=NM, seed=3):
    m = mta.TranscriptionModel(model_type="cnn_rnn_large", n_mels=n_mels, hidden_size=H, num_layers=NL, dropout=0.0, device="cuda")
    m.load_state_dict(R.make_state_dict("cnn_rnn_large", n_mels, H, NL, seed), strict=True)
    m.eval()
    return m


def _wav(path, seconds, seed):
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    wavfile.write(path, 16000, (0.2 * rng.standard_normal(int(16000 * seconds))).clip(-1, 1).astype(np.float32))


def _rule_on_the_library_s_activity(logits, thr, M, G):
    """(NB, 88, T) device logits -> [(midi pitch, start tick, end tick)]: the reference rule on the activity the library thresholds."""
    from music_transcription_amd import ops
    act = ops.predict_from_logits(logits.contiguous().float(), thr).cpu().numpy() > 0
    return sorted((21 + p, TICK(s / FS), TICK(e / FS)) for p, s, e in CR.heads_notes_active(act, None, None, M, G))


def _main(wav, ckpt, mid, thr, *more):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), wav, ckpt, "-o", mid, "-d", "cuda", "-t", str(thr), "--decoder", "frame",
                        "--n-mels", str(NM), "--hidden-size", str(H), "--num-layers", str(NL), *more], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return _midi_notes(mid)


def test_main_writes_the_cleaned_notes(mta, tmp_path):
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    from music_transcription_amd.windows import transcribe_windows
    wav, ckpt, mid = str(tmp_path / "a.wav"), str(tmp_path / "m.pth"), str(tmp_path / "a.mid")
    _wav(wav, 40, 4)
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, NL, 9), ckpt)
    model = _large(mta, seed=9)
    y = tr.load_audio_device(wav, 16000, "cuda")
    chunks, _ = tr.split_into_chunks_device(y)
    with torch.no_grad():
        mel, cmax = get_frontend(16000, NM, 512, "cuda")(chunks, clamp=False)
        logits = model.model(mel, chunk_max_power=cmax)
    stitched = transcribe_windows(model, [y], 2.0)[0][None]
    thr = _mid_threshold(logits)
    flags = ["--min-note-ms", "64", "--bridge-gap-ms", "32"]                      # M = 2, G = 1
    for lg, more in ((logits, []), (stitched, ["--overlap", "2"])):
        want, plain = _rule_on_the_library_s_activity(lg, thr, 2, 1), _rule_on_the_library_s_activity(lg, thr, 1, 0)
        assert 0 < len(want) < len(plain)                                       # this model does give short notes and short gaps
        assert _main(wav, ckpt, mid, thr, *more, *flags) == want


def test_evaluate_script_prints_the_cleaned_figures(mta, tmp_path):
    from music_transcription_amd import evaluate as E
    cache = os.path.join(GOLDEN, "cache_fixture")
    n_mels = 16
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", n_mels, H, NL, 5), ckpt)
    model = _large(mta, n_mels=n_mels, seed=5)
    ds = mta.CachedMaestroDataset(cache, "train")
    with torch.no_grad():
        thr = _mid_threshold(model(ds[0][0][None].cuda()))
    want = E.note_metrics_dataset(model, ds, thr, min_note_frames=2)
    plain = E.note_metrics_dataset(model, ds, thr)
    assert (want["min_note_frames"], want["bridge_frames"]) == (2, 0) and "min_note_frames" not in plain
    assert want["per_sample"] != plain["per_sample"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--cache_dir", cache, "--split", "train",
                        "--model_type", "cnn_rnn_large", "--hidden_size", str(H), "--num_layers", str(NL), "--headless", "--threshold", str(thr),
                        "--note_metrics", "--min_note_ms", "64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict(l.split("=") for l in r.stdout.strip().splitlines())
    assert out["EVAL_NOTE_ONSET_F1"] == f"{want['mean']['onset_f1']:.6f}"
    assert out["EVAL_NOTE_ONSET_OFFSET_F1"] == f"{want['mean']['onset_offset_f1']:.6f}"
    with pytest.raises(ValueError, match="do not clean"):
        E.tune_note_thresholds(model, ds, "cuda", decoder="frame", log=None, min_note_frames=2)


def test_corpus_script_writes_the_notes_main_writes(mta, tmp_path):
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.windows import transcribe_windows
    wavs, out, ckpt = tmp_path / "wav", str(tmp_path / "mid"), str(tmp_path / "m.pth")
    wavs.mkdir()
    for name, seconds, seed in (("a", 35, 11), ("b", 12, 12)):
        _wav(str(wavs / f"{name}.wav"), seconds, seed)
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, NL, 9), ckpt)
    thr = _mid_threshold(transcribe_windows(_large(mta, seed=9), [tr.load_audio_device(str(wavs / "a.wav"), 16000, "cuda")], 2.0)[0])
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "scripts", "transcribe_corpus.py"), "--wav-dir", str(wavs),
                        "--model", ckpt, *MODEL_FLAGS, "--batch", "4", "--threshold", str(thr), "--overlap", "2", "--min-note-ms", "64", "--out-dir", out],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    for name in ("a", "b"):
        got = _midi_notes(os.path.join(out, f"{name}.mid"))
        mid = str(tmp_path / f"{name}_main.mid")
        assert len(got) > 0 and got == _main(str(wavs / f"{name}.wav"), ckpt, mid, thr, "--overlap", "2", "--min-note-ms", "64")
    assert got != _main(str(wavs / "b.wav"), ckpt, mid, thr, "--overlap", "2")       # and the flag did drop notes
