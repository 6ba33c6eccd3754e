"""GPU tests of the decoder grid in ticks (DESIGN.md 6c "Decoder grid in ticks"): mt_notes_grid_ticks, mt_note_match_ticks_cells and
notes.note_grid_ticks_counts against the single-configuration path they replace -- notes.notes_ticks_tables_device followed by
notes.note_match_ticks_device, cell by cell -- and against the host matcher, on the case whose coverage test_note_grid_ticks_cpu.py
asserts; the tuner built on them against a brute-force loop; edge inputs; and independence of what fresh buffers held."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_grid_ticks_case as C  # noqa: E402
import note_ticks_case as TC  # noqa: E402
from alloc_fill import assert_fill_independent, run_under_fills  # noqa: E402

pytestmark = pytest.mark.gpu
BIT63 = -(1 << 63)                        # bit 63 of a uint64 count, read as int64


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _dev(notes):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in notes.items()}


class Dev:
    """The case on the device and the single-configuration path, every cell computed once."""

    def __init__(self):
        self.case = C.Case()
        self.frame, self.onset, self.offset = (torch.from_numpy(x).cuda() for x in (self.case.frame, self.case.onset, self.case.offset))
        self.ref = _dev(self.case.ref)
        self._cells = {}

    def cell(self, cell, offset_gated, rr=2):
        """(tables, counts) of notes_ticks_tables_device / note_match_ticks_device at one cell."""
        from music_transcription_amd.notes import note_match_ticks_device, notes_ticks_tables_device
        key = (cell, offset_gated, rr)
        if key not in self._cells:
            tf, to, tk, (M, G), R = cell
            est = notes_ticks_tables_device(self.frame, self.onset, tf, to, C.LENGTHS, offset_logits=self.offset if offset_gated else None,
                                            offset_threshold=tk, min_note_frames=M, bridge_frames=G, refine_reach=rr,
                                            onset_detect="peak" if R else "edge", peak_reach=R or 1)
            self._cells[key] = (est, note_match_ticks_device(est, self.ref))
        return self._cells[key]

    def grid(self, g, offset_gated, rr=2, reaches=True):
        from music_transcription_amd.notes import note_grid_ticks_counts
        return note_grid_ticks_counts(self.frame, self.onset, self.ref, g["tf"], g["to"], self.offset if offset_gated else None,
                                      g["tk"] if offset_gated else None, g["cleanups"], g["reaches"] if reaches else None, C.LENGTHS, rr)


@pytest.fixture(scope="module")
def dev(mta):
    return Dev()


def _check_grid(dev, g, offset_gated, got):
    cells = C.cells(g, offset_gated)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (C.B, *(n + 1 for n in cells[-1][0]), 4)
    got = got.cpu().numpy()
    bad = [(idx, cell) for idx, cell in cells if not np.array_equal(got[(slice(None), *idx)], dev.cell(cell, offset_gated)[1].cpu().numpy())]
    assert not bad, bad[:4]
    return got


@pytest.mark.parametrize("offset_gated", [True, False], ids=["offset-gated", "onset-gated"])
def test_grid_equals_the_single_configuration_path(dev, offset_gated):
    """Every cell of the main grid (32 offset-gated, 16 onset-gated with Kk = 1): note_match_ticks_device(notes_ticks_tables_device(cell),
    ref) exactly, and the host matcher on the extractor's own slices."""
    from music_transcription_amd.notes import note_match_ticks, notes_grid_ticks_tables_device
    got = _check_grid(dev, C.GRID, offset_gated, dev.grid(C.GRID, offset_gated))
    assert len({tuple(got[(slice(None), *idx)].reshape(-1)) for idx, _ in C.cells(C.GRID, offset_gated)}) >= (24 if offset_gated else 12)
    g = C.GRID
    tab = notes_grid_ticks_tables_device(dev.frame, dev.onset, g["tf"], g["to"], dev.offset if offset_gated else None,
                                         g["tk"] if offset_gated else None, g["cleanups"], g["reaches"], C.LENGTHS, 2)
    rows = C.B * C.P
    on, off, ptr = (tab[k].cpu().numpy() for k in ("on", "off", "ptr"))
    for n, (idx, cell) in enumerate(C.cells(g, offset_gated)):
        lo, hi = ptr[n * rows], ptr[(n + 1) * rows]
        one = {"on": on[lo:hi], "off": off[lo:hi], "ptr": ptr[n * rows:(n + 1) * rows + 1] - lo}
        assert np.array_equal(note_match_ticks(one, dev.case.ref).astype(np.int64), got[(slice(None), *idx)]), (idx, cell)


def test_without_a_reach_axis(dev):
    """peak_reaches=None: no such axis, the edge rule."""
    g = dict(C.GRID, reaches=[0])
    got = dev.grid(g, False, reaches=False)
    assert tuple(got.shape) == (C.B, 2, 2, 1, 2, 4)
    _check_grid(dev, g, False, got[..., None, :])


@pytest.mark.parametrize("rr", [0, 2, 8])
@pytest.mark.parametrize("offset_gated", [True, False], ids=["offset-gated", "onset-gated"])
def test_slices_equal_the_tables(dev, offset_gated, rr):
    """The extractor's per-cell slices equal notes_ticks_tables_device's tables element for element (ptr, on, off)."""
    from music_transcription_amd.notes import notes_grid_ticks_tables_device
    g = C.GRID if rr == 2 else dict(C.GRID, tf=[0.4], tk=[0.6])
    tab = notes_grid_ticks_tables_device(dev.frame, dev.onset, g["tf"], g["to"], dev.offset if offset_gated else None,
                                         g["tk"] if offset_gated else None, g["cleanups"], g["reaches"], C.LENGTHS, rr)
    cells = C.cells(g, offset_gated)
    rows = C.B * C.P
    assert tab["cells"] == len(cells) and tab["ptr"].numel() == len(cells) * rows + 1 and int(tab["ptr"][0]) == 0
    ptr = tab["ptr"].cpu().numpy()
    assert ptr[-1] == tab["on"].numel() == tab["off"].numel() > 1000
    for n, (idx, cell) in enumerate(cells):
        want = dev.cell(cell, offset_gated, rr)[0]
        lo, hi = int(ptr[n * rows]), int(ptr[(n + 1) * rows])
        assert np.array_equal(ptr[n * rows:(n + 1) * rows + 1] - lo, want["ptr"].cpu().numpy()), (idx, cell, "ptr")
        assert torch.equal(tab["on"][lo:hi], want["on"]), (idx, cell, "on")
        assert torch.equal(tab["off"][lo:hi], want["off"]), (idx, cell, "off")
    if rr == 2:                                             # the refinement is at work: onsets off the frame grid
        assert int((tab["on"] % 320 != 0).sum()) > 1000


@pytest.mark.parametrize("offset_gated", [True, False], ids=["offset-gated", "onset-gated"])
def test_slices_against_the_host_composition(dev, offset_gated):
    """The extractor against the host decode -> refine composition of the case (no device decoder in between): ptr and off exactly,
    and on within one tick.  The tick bound: the kernel evaluates the sigmoids in f32 (a few 1e-7 off the f64 values), the shift's
    denominator is at least the margin 2^-10, so the shift moves by less than 1e-3 and rint(320 shift) by at most one.  That holds
    where f32 and f64 take the same decisions; notes whose margin lies within 1e-5 of 2^-10, or with two neighbouring probabilities
    on the peak walk closer than 1e-6, are left out of the tick comparison (and must stay below 1 % of the notes)."""
    import onset_regress_ref as OG
    from music_transcription_amd.notes import notes_grid_ticks_tables_device
    rr, case = 2, dev.case
    g = dict(C.GRID, tf=[0.4], tk=[0.6])
    tab = notes_grid_ticks_tables_device(dev.frame, dev.onset, g["tf"], g["to"], dev.offset if offset_gated else None,
                                         g["tk"] if offset_gated else None, g["cleanups"], g["reaches"], C.LENGTHS, rr)
    on, off, ptr = (tab[k].cpu().numpy().astype(np.int64) for k in ("on", "off", "ptr"))
    rows, compared, skipped = C.B * C.P, 0, 0
    for n, (idx, cell) in enumerate(C.cells(g, offset_gated)):
        want = case.host_tables(cell, rr, offset_gated)
        lo, hi = ptr[n * rows], ptr[(n + 1) * rows]
        assert np.array_equal(ptr[n * rows:(n + 1) * rows + 1] - lo, want["ptr"]), (idx, cell, "ptr")
        assert np.array_equal(off[lo:hi], want["off"]), (idx, cell, "off")
        i = 0
        for b, p in itertools.product(range(C.B), range(C.P)):
            for s, e in case.row_notes(b, p, cell, offset_gated):
                q = case._q[b, p]
                tick, _, margin = OG.refine_one(q, s, e, rr)
                walk = q[s:min(s + rr, e - 1, len(q) - 1) + 1]
                if abs(margin - 2.0 ** -10) < 1e-5 or (len(walk) > 1 and np.abs(np.diff(walk)).min() < 1e-6):
                    skipped += 1
                else:
                    assert abs(int(on[lo + i]) - tick) <= 1, (idx, cell, b, p, s, e, int(on[lo + i]), tick)
                    compared += 1
                i += 1
        assert i == hi - lo
    print("notes compared", compared, "left out", skipped)
    assert compared > 1000 and skipped * 100 < compared


def test_a_grid_past_64_cells_tiles(dev):
    """3 x 3 x 2 x 2 x 3 = 108 cells with repeated and unsorted axis values: the same grid cell by cell."""
    got = _check_grid(dev, C.GRID_108, True, dev.grid(C.GRID_108, True))
    assert np.array_equal(got[:, :, 0], got[:, :, 2]) and not np.array_equal(got[:, :, 0], got[:, :, 1])      # to = [0.5, 0.35, 0.5]


def test_cells_matcher(mta):
    """mt_note_match_ticks_cells with K = 1 equals mt_note_match_ticks on the same tables; stacked three times, an unsorted estimate row in
    one cell sets bit 63 for that (cell, recording) alone -- a bad-input status, nothing is read through the row -- and the other counts
    stay those of the clean tables."""
    from music_transcription_amd.notes import note_match_ticks_cells_device, note_match_ticks_device
    est, ref = TC.tables()
    d_ref = _dev(ref)
    want = note_match_ticks_device(_dev(est), d_ref)
    for lengths in (None, [40, 10, 0]):
        one = note_match_ticks_cells_device(_dev(est), d_ref, 1, lengths)
        assert torch.equal(one, note_match_ticks_device(_dev(est), d_ref, lengths)[None])
    K, rows, n = 3, TC.B * TC.P, len(est["on"])
    stacked = {"on": np.tile(est["on"], K), "off": np.tile(est["off"], K),
               "ptr": np.concatenate([est["ptr"][:-1] + k * n for k in range(K)] + [[K * n]]).astype(np.int64)}
    clean = note_match_ticks_cells_device(_dev(stacked), d_ref, K)
    assert torch.equal(clean, want[None].expand(K, -1, -1))
    row = next(r for r in range(TC.P, 2 * TC.P) if est["ptr"][r + 1] - est["ptr"][r] >= 2 and est["on"][est["ptr"][r]] < est["on"][est["ptr"][r + 1] - 1])
    a, b = n + est["ptr"][row], n + est["ptr"][row + 1] - 1               # cell 1, recording 1
    stacked["on"][[a, b]] = stacked["on"][[b, a]]
    with pytest.raises(ValueError, match="non-decreasing"):
        note_match_ticks_cells_device(_dev(stacked), d_ref, K)
    got = note_match_ticks_cells_device(_dev(stacked), d_ref, K, checked=False)
    flagged = (got & BIT63) != 0
    assert flagged[1, 1].all() and int(flagged.sum()) == 4
    keep = torch.ones_like(flagged)
    keep[1, 1] = False
    assert torch.equal(got[keep], clean[keep])
    with pytest.raises(ValueError):
        note_match_ticks_cells_device(_dev(stacked), d_ref, 2)


def test_edge_inputs(dev):
    from music_transcription_amd.notes import note_grid_ticks_counts, notes_grid_ticks_tables_device
    n_ref = np.diff(dev.case.ref["ptr"][::C.P])
    # all lengths 0: nothing is read (the logits are NaN there), no estimate, every reference note counted
    nan = torch.full_like(dev.frame, float("nan"))
    got = note_grid_ticks_counts(nan, nan, dev.ref, [0.4, 0.6], [0.5], nan, [0.5], [(1, 0), (2, 1)], [0, 1], [0, 0, 0]).cpu().numpy()
    assert got.shape == (C.B, 2, 1, 1, 2, 2, 4)
    assert (got[..., 0] == n_ref[:, None, None, None, None, None]).all() and (got[..., 1:] == 0).all()
    # a cell that decodes no note beside cells that do
    g = dict(C.GRID, to=[0.35, 0.9999999])
    got = dev.grid(g, True).cpu().numpy()
    assert (got[:, :, 1, ..., 1:] == 0).all() and (got[:, :, 0, ..., 1] > 0)[:2].all() and (got[..., 0] == n_ref[:, None, None, None, None, None]).all()
    tab = notes_grid_ticks_tables_device(dev.frame, dev.onset, [0.5], [0.9999999], lengths=C.LENGTHS)
    assert tab["on"].numel() == 0 and int(tab["ptr"].abs().sum()) == 0
    # T = 1
    x = torch.tensor([3.0, -3.0], device="cuda").repeat(44).reshape(1, 88, 1)
    ref = {"on": torch.zeros(88, dtype=torch.int32, device="cuda"), "off": torch.full((88,), 320, dtype=torch.int32, device="cuda"),
           "ptr": torch.arange(89, dtype=torch.int64, device="cuda")}
    got = note_grid_ticks_counts(x, x, ref, [0.5], [0.5], x, [0.5], [(1, 0), (2, 0)], [0, 1]).cpu().numpy()
    assert (got[0, 0, 0, 0, 0] == [88, 44, 44, 44]).all() and (got[0, 0, 0, 0, 1] == [88, 0, 0, 0]).all()


class _Recordings:
    """Two whole recordings with a MIDI note list: recordings 0 and 1 of the case."""
    onset_labels, chunk_length = "midi", None

    def __init__(self, dev):
        self.dev = dev

    def __len__(self):
        return 2

    def ref_notes(self, indices):
        ref, on, off, ptr = self.dev.case.ref, [], [], [0]
        for i in indices:
            lo, hi = ref["ptr"][i * C.P], ref["ptr"][(i + 1) * C.P]
            on.append(ref["on"][lo:hi])
            off.append(ref["off"][lo:hi])
            ptr += (ref["ptr"][i * C.P + 1:(i + 1) * C.P + 1] - lo + ptr[-1]).tolist()
        return _dev({"on": np.concatenate(on), "off": np.concatenate(off), "ptr": np.array(ptr, np.int64)})


def test_tuner_picks_the_brute_force_cell(dev, monkeypatch):
    """tune_note_decoder(refine_onsets=True) on two groups of one recording each: every round is one note_grid_ticks_counts call per
    group, and the chosen cell is the best of a loop over note_metrics_dataset(refine_onsets=True) at the candidates it scored."""
    from music_transcription_amd import evaluate as E, notes as N
    ds = _Recordings(dev)

    def fake(model, dataset, indices, device="cuda", max_batch=128, all_heads=False, with_offset=False):
        assert all_heads and with_offset
        return [(i, dev.frame[i, :, :C.LENGTHS[i]], torch.zeros_like(dev.frame[i, :, :C.LENGTHS[i]]), dev.onset[i, :, :C.LENGTHS[i]],
                 dev.offset[i, :, :C.LENGTHS[i]]) for i in indices]
    monkeypatch.setattr(E, "collect_logits", fake)
    calls, axes = [], set()
    real = N.note_grid_ticks_counts

    def spy(frame, on, ref, tf, to, off=None, tk=None, cleanups=None, reaches=None, lengths=None, rr=2):
        calls.append(frame.shape[0])
        axes.update(itertools.product(np.float32(tf).tolist(), np.float32(to).tolist(), np.float32(tk).tolist()))
        return real(frame, on, ref, tf, to, off, tk, cleanups, reaches, lengths, rr)
    monkeypatch.setattr(N, "note_grid_ticks_counts", spy)
    monkeypatch.setattr(N, "note_grid_counts", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the frame-grid kernel was called")))
    cleanups, reaches = [(1, 0), (3, 1)], [0, 1]
    got = E.tune_note_decoder(None, ds, "cuda", decoder="onset_offset", note_reference="midi", objective="onset", cleanups=cleanups,
                              tune_range=(0.4, 0.6), tune_step=0.2, tune_rounds=1, log=None, max_batch=1, peak_reaches=reaches,
                              refine_onsets=True, refine_reach=3)
    thr, othr, kthr, clean, (detect, reach), best = got
    assert calls and len(calls) % 2 == 0 and set(calls) == {1}          # one call per group (of one recording) and round
    monkeypatch.setattr(N, "note_grid_ticks_counts", real)
    brute = {}
    for (a, o, k), cl, R in itertools.product(sorted(axes), cleanups, reaches):
        m = E.note_metrics_dataset(None, ds, a, o, offset_threshold=k, note_reference="midi", max_batch=1, min_note_frames=cl[0],
                                   bridge_frames=cl[1], refine_onsets=True, refine_reach=3,
                                   **(dict(onset_detect="peak", peak_reach=R) if R else {}))
        brute[a, o, k, cl, R] = m["mean"]["onset_f1"]
    top = max(brute.values())
    key = (float(np.float32(thr)), float(np.float32(othr)), float(np.float32(kthr)), tuple(clean), reach)
    assert detect == ("peak" if reach else "edge") and key in brute, (got, sorted(brute)[:3])
    assert best == pytest.approx(top, abs=1e-12) and brute[key] == pytest.approx(top, abs=1e-12), (got, top)
    assert 0.0 < top < 1.0 and len(set(brute.values())) > len(brute) // 2


def test_counts_do_not_depend_on_what_fresh_buffers_held(dev):
    """The main grid, a tiled grid and the stacked tables under alloc_fill's 0x00 twice, 0xFF and 0x47: outputs and workspaces are fully
    written before they are read; integers only, so the comparison is bitwise."""
    from music_transcription_amd.notes import notes_grid_ticks_tables_device
    small = dict(C.GRID_108, tf=[0.6, 0.4], to=[0.5])

    def fn():
        g = C.GRID
        tab = notes_grid_ticks_tables_device(dev.frame, dev.onset, g["tf"], g["to"], None, None, g["cleanups"], g["reaches"], C.LENGTHS, 2)
        return {"offset": dev.grid(C.GRID, True), "onset": dev.grid(C.GRID, False), "tiled": dev.grid(dict(small, reaches=list(range(9))), True),
                "on": tab["on"], "off": tab["off"], "ptr": tab["ptr"]}
    spreads = assert_fill_independent(run_under_fills(fn))
    assert all(s == 0.0 for s in spreads.values()), spreads
