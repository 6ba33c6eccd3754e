"""GPU tests of the tick matcher mt_note_match_ticks and its Python surface (DESIGN.md 6c "Sub-frame onsets", Scoring): the device counts
against the host matcher notes.note_match_ticks on the rows of note_ticks_case (whose coverage test_note_ticks_cpu.py asserts), against
the independent frame-grid kernel mt_note_match_list, on empty lists, under filled allocations, the wrapper's refusals, and the device
note tables and the evaluation built on them against the host path."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_fill as AF  # noqa: E402
import note_ticks_case as TC  # noqa: E402
from offset_decode_ref import markov  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


@pytest.fixture(scope="module")
def case(mta):
    """(est, ref) host tables, the same on the device, and the host matcher's counts -- computed once."""
    from music_transcription_amd.notes import note_match_ticks
    est, ref = TC.tables()
    return est, ref, _dev(est), _dev(ref), note_match_ticks(est, ref).astype(np.int64)


def _dev(notes):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in notes.items()}


def _host(notes):
    return {k: v.cpu().numpy() for k, v in notes.items()}


def test_counts_equal_the_host_matcher(mta, case):
    from music_transcription_amd.notes import note_match_ticks_device
    est, ref, d_est, d_ref, want = case
    got = note_match_ticks_device(d_est, d_ref)
    assert got.dtype == torch.int64 and got.shape == (TC.B, 4) and got.is_cuda
    got = got.cpu().numpy()
    if not np.array_equal(got, want):                                       # name the rows: every row alone, the others emptied
        bad = []
        for r in range(TC.B * TC.P):
            one = [{"on": d["on"][d["ptr"][r]:d["ptr"][r + 1]], "off": d["off"][d["ptr"][r]:d["ptr"][r + 1]],
                    "ptr": np.concatenate([np.zeros(r + 1, np.int64), np.full(TC.B * TC.P - r, d["ptr"][r + 1] - d["ptr"][r])])} for d in (est, ref)]
            g = note_match_ticks_device(_dev(one[0]), _dev(one[1])).cpu().numpy()[r // TC.P]
            c = TC.row_counts(one[0]["on"], one[0]["off"], one[1]["on"], one[1]["off"])
            if g.tolist() != [c["n_ref"], c["n_est"], c["tp_onset"], c["tp_onset_offset"]]:
                bad.append((r, TC.SPECIAL.get(r, ("random",))[0], g.tolist(), c["tp_onset"], c["tp_onset_offset"]))
        raise AssertionError((got, want, bad[:10]))


def test_counts_with_lengths_equal_the_model(mta, case):
    """The length rule on the same rows: recording 0 cut inside its notes, recording 1 at nothing, recording 2 past the random rows but
    inside the chained one.  The reference is the numpy model, which test_note_ticks_cpu.py holds against scipy under this rule too."""
    from music_transcription_amd.notes import note_match_ticks_device
    est, ref, d_est, d_ref, _ = case
    for lengths in ([20, 0, 300], [1 << 40, -5, 1]):
        want, _ = TC.model_counts(est, ref, lengths)
        got = note_match_ticks_device(d_est, d_ref, lengths=lengths).cpu().numpy()
        assert np.array_equal(got, want), (lengths, got, want)


def test_on_the_frame_grid_equals_note_match_list(mta):
    """Estimates on the frame grid are what mt_note_match_list scores: an independent kernel with the same criteria and length rule."""
    from music_transcription_amd.notes import note_match_list, note_match_ticks_device, notes_batch_device
    rng = np.random.default_rng(4)
    B, P, T, lengths = 2, 88, 40, [40, 27]
    act = markov(rng, (B, P, T), 0.15, 0.3)
    edge = act & ~np.concatenate([np.zeros((B, P, 1), bool), act[..., :-1]], -1)
    frame = torch.from_numpy(np.where(act, 3.0, -3.0).astype(np.float32)).cuda()
    onset = torch.from_numpy(np.where(edge | (rng.random((B, P, T)) < 0.05), 3.0, -3.0).astype(np.float32)).cuda()
    r_on, r_off, r_ptr = [], [], [0]                                         # reference notes around the runs, off the grid, some past the lengths
    for b in range(B):
        for p in range(P):
            s = np.flatnonzero(edge[b, p])
            on = np.sort(np.clip(320 * s + rng.integers(-600, 601, size=s.size), 0, None))
            r_on += on.tolist()
            r_off += (on + rng.integers(100, 3000, size=s.size)).tolist()
            r_ptr.append(len(r_on))
    ref = _dev({"on": np.array(r_on, np.int32), "off": np.array(r_off, np.int32), "ptr": np.array(r_ptr, np.int64)})
    want = note_match_list(frame, ref, 0.5, onset, 0.5, lengths).cpu().numpy()
    notes = notes_batch_device(frame, onset, 0.5, 0.5, lengths, fs=1.0, min_midi=0)          # (pitch row, start frame, end frame)
    e_on, e_off, e_ptr = [], [], [0]
    for b in range(B):
        for p in range(P):
            row = [(int(s), int(e)) for q, s, e in notes[b] if q == p]
            assert row == sorted(row)
            e_on += [320 * s for s, _ in row]
            e_off += [320 * e for _, e in row]
            e_ptr.append(len(e_on))
    est = _dev({"on": np.array(e_on, np.int32), "off": np.array(e_off, np.int32), "ptr": np.array(e_ptr, np.int64)})
    got = note_match_ticks_device(est, ref, lengths).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert (want[:, 2] > 10).all() and (want[:, 3] < want[:, 2]).all() and want[1, 0] < (np.diff(r_ptr)[P:]).sum()   # matches, pruned; notes cut by lengths


@pytest.mark.parametrize("empty", ["both", "est", "ref"])
def test_empty_lists(mta, case, empty):
    """The raw entry point with no notes at all, no estimates, no reference notes: the counts are written, and neither the words around
    them nor the workspace past its size."""
    from music_transcription_amd import _lib
    _, _, d_est, d_ref, want = case
    rows = TC.B * TC.P
    none = {"on": None, "off": None, "ptr": torch.zeros(rows + 1, dtype=torch.int64, device="cuda")}
    est = none if empty in ("both", "est") else d_est
    ref = none if empty in ("both", "ref") else d_ref
    n_est, n_ref = (0 if d["on"] is None else d["on"].numel() for d in (est, ref))
    counts = torch.full((TC.B * 4 + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    size = int(_lib.lib.mt_note_match_ticks_workspace(n_est, n_ref))
    ws = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.mt_note_match_ticks(_lib.ptr(est["on"]), _lib.ptr(est["off"]), _lib.ptr(est["ptr"]), _lib.ptr(ref["on"]),
                                            _lib.ptr(ref["off"]), _lib.ptr(ref["ptr"]), None, _lib.ptr(counts[4:]), TC.B, TC.P, _lib.ptr(ws), size,
                                            _lib.stream_ptr()), "mt_note_match_ticks")
    c = counts.cpu().numpy()
    assert (c[:4] == SENTINEL).all() and (c[-4:] == SENTINEL).all()
    expect = np.zeros((TC.B, 4), np.int64)
    if empty == "est":
        expect[:, 0] = want[:, 0]
    if empty == "ref":
        expect[:, 1] = want[:, 1]
    assert np.array_equal(c[4:-4].reshape(TC.B, 4), expect), (c, expect)
    assert bool((ws[size:] == 0x5A).all())
    if empty == "both":
        assert bool((ws == 0x5A).all())                                     # nothing to match: the workspace is not touched


def test_counts_do_not_depend_on_what_the_buffers_held(mta, case):
    from music_transcription_amd.notes import note_match_ticks_device
    _, _, d_est, d_ref, want = case
    results = AF.run_under_fills(lambda: {"counts": note_match_ticks_device(d_est, d_ref), "cut": note_match_ticks_device(d_est, d_ref, [20, 0, 300])})
    AF.assert_fill_independent(results, tag="note_match_ticks_device")
    for r in results:
        assert np.array_equal(r["counts"].numpy(), want)


def test_wrapper_refuses_bad_tables_before_any_launch(mta, case, monkeypatch):
    from music_transcription_amd import _lib, notes as N
    est, ref, d_est, d_ref, _ = case

    def launched(*a):
        raise AssertionError("mt_note_match_ticks was launched")
    monkeypatch.setattr(_lib.lib, "mt_note_match_ticks", launched)
    row = next(r for r in range(TC.B * TC.P) if est["ptr"][r + 1] - est["ptr"][r] >= 2 and est["on"][est["ptr"][r]] < est["on"][est["ptr"][r + 1] - 1])
    swapped = est["on"].copy()
    a, b = est["ptr"][row], est["ptr"][row + 1] - 1
    swapped[[a, b]] = swapped[[b, a]]
    with pytest.raises(ValueError, match="non-decreasing"):
        N.note_match_ticks_device(_dev({**est, "on": swapped}), d_ref)
    with pytest.raises(ValueError, match="non-decreasing"):
        N.note_match_ticks_device(d_ref, _dev({**est, "on": swapped}))
    # a row's first note before its predecessor's last is no disorder; the last two notes of the tables out of order are
    last = ref["on"].copy()
    last[-2:] = last[-2:][::-1] + [1, 0]
    assert last[-2] > last[-1]
    with pytest.raises(ValueError, match="non-decreasing"):
        N.note_match_ticks_device(d_est, _dev({**ref, "on": last}))
    for bad in (np.concatenate([est["ptr"][:-1], [est["ptr"][-1] + 1]]), np.concatenate([[1], est["ptr"][1:]]),
                np.concatenate([est["ptr"][:5], [est["ptr"][-1]], est["ptr"][6:]])):
        with pytest.raises(ValueError, match="ptr must rise"):
            N.note_match_ticks_device(_dev({**est, "ptr": bad}), d_ref)
    with pytest.raises(ValueError):
        N.note_match_ticks_device(_dev({**est, "ptr": est["ptr"][:-1]}), d_ref)
    with pytest.raises(ValueError, match="CUDA"):
        N.note_match_ticks_device({k: torch.from_numpy(v) for k, v in est.items()}, d_ref)
    with pytest.raises(ValueError, match="CUDA"):
        N.note_match_ticks_device(d_est, {**d_ref, "off": d_ref["off"].cpu()})
    with pytest.raises(ValueError):
        N.note_match_ticks_device({**d_est, "on": d_est["on"].long()}, d_ref)
    with pytest.raises(ValueError, match="lengths"):
        N.note_match_ticks_device(d_est, d_ref, lengths=[1, 2])


# ------------------------------------------------------------------ the tables and the evaluation
def _heads(seed, B=3, P=88, T=130):
    rng = np.random.default_rng(seed)
    logit = lambda run, hi, lo: torch.from_numpy(np.where(run, rng.uniform(0.2, hi, run.shape), -rng.uniform(0.2, lo, run.shape)).astype(np.float32)).cuda()
    act = markov(rng, (B, P, T), 0.08, 0.2)
    edge = act & ~np.concatenate([np.zeros((B, P, 1), bool), act[..., :-1]], -1)
    return logit(act, 4.0, 4.0), logit(edge | markov(rng, (B, P, T), 0.04, 0.6), 4.0, 4.0), logit(markov(rng, (B, P, T), 0.05, 0.7), 4.0, 4.0)


@pytest.mark.parametrize("kw", [dict(), dict(offset=True), dict(min_note_frames=2, bridge_frames=1), dict(offset=True, min_note_frames=3, bridge_frames=2),
                                dict(onset_detect="peak", peak_reach=2), dict(offset=True, onset_detect="peak", peak_reach=1, refine_reach=0)],
                         ids=["onset", "offset", "onset-clean", "offset-clean", "onset-peak", "offset-peak"])
def test_device_tables_equal_the_host_tables(mta, kw):
    from music_transcription_amd.notes import notes_ticks_device, notes_ticks_tables_device
    frame, onset, offset = _heads(7)
    kw = dict(kw)
    off = offset if kw.pop("offset", False) else None
    for lengths in ([130, 97, 0], None):
        want = notes_ticks_device(frame, onset, 0.5, 0.5, lengths, offset_logits=off, **kw)
        got = notes_ticks_tables_device(frame, onset, 0.5, 0.5, lengths, offset_logits=off, **kw)
        assert all(got[k].is_cuda and got[k].is_contiguous() for k in got)
        assert got["on"].dtype == got["off"].dtype == torch.int32 and got["ptr"].dtype == torch.int64
        for k in ("on", "off", "ptr"):
            assert np.array_equal(got[k].cpu().numpy(), want[k]), (k, lengths)
        assert len(want["on"]) > 200


def test_evaluation_scores_refined_notes_on_the_device(mta, tmp_path_factory, monkeypatch):
    """note_metrics_dataset(refine_onsets=True) on the two-recording tree of test_gpu_onset_regress.py: the dict of the host scoring of
    the same lists, with the host matcher out of reach."""
    from test_gpu_onset_regress import _small_tree
    from music_transcription_amd import evaluate as E, notes as N
    tree = str(tmp_path_factory.mktemp("maestro_ticks"))
    _small_tree(tree, {"a": (12.0, "train"), "b": (9.5, "train"), "v": (7.0, "validation")})
    src = mta.MaestroDataset(tree, split="train", n_mels=64, onset_labels="midi", onset_target="regress", onset_width=4)
    rng = np.random.default_rng(2)

    def fake(model, dataset, indices, device="cuda", max_batch=128, all_heads=False, with_offset=False):
        out = []
        for i in indices:
            _, lab, _ = src.get_batch([i])
            on = torch.logit(lab["onset"][0], eps=1e-6)
            on = on + torch.from_numpy(rng.normal(0.0, 1.5, tuple(on.shape)).astype(np.float32)).to(on.device)      # misses and extras
            item = (i, (lab["frame"][0] * 20.0 - 10.0).contiguous(), lab["frame"][0].contiguous())
            out.append(item + ((on, torch.full_like(on, -20.0)) if with_offset else (on,)) if all_heads else item)
        return out
    monkeypatch.setattr(E, "collect_logits", fake)
    for kw in (dict(), dict(offset_threshold=0.5), dict(onset_detect="peak", peak_reach=2, min_note_frames=2)):
        args = dict(threshold=0.5, onset_threshold=0.5, note_reference="midi", refine_onsets=True, refine_reach=4, **kw)
        rng = np.random.default_rng(2)
        lr = fake(None, src, [0, 1], all_heads=True, with_offset="offset_threshold" in kw)
        vals = {k: [] for k in E.NOTE_METRIC_KEYS}                           # the host scoring of the same lists, group by group
        for frame, on, ref, lengths, off in E._note_groups(lr, src, True, "midi", 128, "offset_threshold" in kw):
            est = N.notes_ticks_device(frame, on, 0.5, 0.5, lengths, offset_logits=off, refine_reach=4,
                                       **{k: v for k, v in kw.items() if k != "offset_threshold"})
            for m in N.note_prf(N.note_match_ticks(est, ref)):
                for c in ("onset", "onset_offset"):
                    for k, v in zip(("precision", "recall", "f1"), m[c]):
                        vals[f"{c}_{k}"].append(v)
        rng = np.random.default_rng(2)
        with monkeypatch.context() as mp:
            mp.setattr(N, "note_match_ticks", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the host matcher was called")))
            got = E.note_metrics_dataset(None, src, **args)
        assert got["per_sample"] == vals, (kw, got["per_sample"], vals)
        assert got["refine_reach"] == 4 and got["mean"] == {k: float(np.mean(v)) for k, v in vals.items()}
        assert 0.0 < got["mean"]["onset_f1"] < 1.0, got["mean"]
