"""CPU tests of the tick matcher (DESIGN.md 6c "Sub-frame onsets", Scoring): the numpy restatement of mt_note_match_ticks' algorithm
(note_ticks_case.row_counts) and the host matcher notes.note_match_ticks both equal scipy's maximum bipartite matching on every row of
the generated case -- which pins the convexity claim behind the greedy pass for tp_onset and the component rule before any GPU run --
and the case holds the rows the GPU test relies on.  The argument checks of the entry point that need no GPU are here too."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_ticks_case as TC  # noqa: E402


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


@pytest.fixture(scope="module")
def case():
    pytest.importorskip("scipy")
    est, ref = TC.tables()
    counts, per = TC.model_counts(est, ref)
    want = [TC.scipy_row(eo, ef, ro, rf) for (eo, ef), (ro, rf) in zip(TC.rows_of(est), TC.rows_of(ref))]
    return est, ref, counts, per, want


def test_model_and_host_matcher_are_maximum_matchings(mta, case):
    from music_transcription_amd.notes import note_match_ticks
    est, ref, counts, per, want = case
    for r, (c, (tp_on, tp_onoff)) in enumerate(zip(per, want)):
        assert (c["tp_onset"], c["tp_onset_offset"]) == (tp_on, tp_onoff), (r, TC.SPECIAL.get(r, ("random",))[0], c, tp_on, tp_onoff)
    host = note_match_ticks(est, ref)
    assert host.shape == (TC.B, 4) and np.array_equal(host.astype(np.int64), counts), (host, counts)
    by_b = np.array(want).reshape(TC.B, TC.P, 2).sum(1)
    assert np.array_equal(counts[:, 2:], by_b)


def test_model_applies_the_length_rule(case):
    """With lengths the model is the unclipped model on the reference list cut by hand: notes with on >= 320 L dropped, offsets clipped."""
    est, ref, _, _, _ = case
    lengths = [20, 0, 300]
    got, _ = TC.model_counts(est, ref, lengths)
    on, off, pt = [], [], [0]
    for r, (ro, rf) in enumerate(TC.rows_of(ref)):
        end = 320 * lengths[r // TC.P]
        keep = ro < end
        on += ro[keep].tolist()
        off += np.minimum(rf[keep], end).tolist()
        pt.append(len(on))
    cut = {"on": np.array(on, np.int32), "off": np.array(off, np.int32), "ptr": np.array(pt, np.int64)}
    want, _ = TC.model_counts(est, cut)
    assert np.array_equal(got, want) and got[1, 0] == 0 and 0 < got[0, 0] < TC.model_counts(est, ref)[0][0, 0]
    sc = np.array([TC.scipy_row(eo, ef, ro, rf) for (eo, ef), (ro, rf) in zip(TC.rows_of(est), TC.rows_of(cut))]).reshape(TC.B, TC.P, 2).sum(1)
    assert np.array_equal(got[:, 2:], sc)


def test_case_holds_the_rows_the_gpu_test_relies_on(case):
    est, ref, counts, per, want = case
    name = {v[0]: r for r, v in TC.SPECIAL.items()}
    n_ref = [c["n_ref"] for c in per]
    for n in (0, 1, 63, 64, 65, 129):
        r = name[f"refs_{n}"]
        assert n_ref[r] == n and (n == 0 or per[r]["n_est"] > 0), (n, per[r])
    assert n_ref[name["refs_129_last"]] == 129                                              # the very last row of the tables
    assert per[name["refs_only"]]["n_est"] == 0 and per[name["refs_only"]]["n_ref"] > 0
    assert per[name["ests_only"]]["n_ref"] == 0 and per[name["ests_only"]]["n_est"] > 0
    (eo, _), (ro, _) = TC.rows_of(est)[name["equal_onsets"]], TC.rows_of(ref)[name["equal_onsets"]]
    assert (np.diff(eo) == 0).any() and (np.diff(ro) == 0).any() and want[name["equal_onsets"]][0] > 0
    assert any(a < 64 < b for a, b in per[name["straddle"]]["components"]), per[name["straddle"]]["components"]
    assert any(a < 64 < b or a < 128 < b for r in (name["refs_65"], name["refs_129"]) for a, b in per[r]["components"])
    ch = per[name["chained"]]
    assert ch["components"] == [(0, ch["n_ref"])] and ch["n_ref"] >= 1000                    # one component, the whole row
    assert want[name["chained"]][1] < want[name["chained"]][0] and ch["augmentations"] > 0   # pruned edges, real searches
    deep = per[name["deep_search"]]
    assert deep["failed"] == 1 and deep["max_depth"] == deep["n_ref"] - 1 and want[name["deep_search"]] == (deep["n_ref"], deep["n_ref"] - 1)
    aug = per[name["augmenting"]]
    assert (aug["greedy"], aug["augmentations"]) == (1, 1) and want[name["augmenting"]] == (2, 2)     # the greedy seed 1, the maximum 2
    rnd = np.array([want[r] for r in TC.RANDOM_ROWS])
    assert (rnd[:, 0] > 0).mean() >= 0.3, (rnd[:, 0] > 0).mean()
    assert (rnd[:, 1] < rnd[:, 0]).mean() >= 0.1, (rnd[:, 1] < rnd[:, 0]).mean()
    assert sum(per[r]["augmentations"] > 0 for r in TC.RANDOM_ROWS) >= 1                     # a greedy seed below the maximum, unplanted
    assert sum(len(c["components"]) > 1 for c in per) >= 20


def test_random_tables_agree_with_scipy_at_other_seeds(case):
    for seed in (11, 12):
        est, ref = TC.tables(seed)
        _, per = TC.model_counts(est, ref)
        for r, (c, (eo, ef), (ro, rf)) in enumerate(zip(per, TC.rows_of(est), TC.rows_of(ref))):
            if r in TC.RANDOM_ROWS or r < 8:
                assert (c["tp_onset"], c["tp_onset_offset"]) == TC.scipy_row(eo, ef, ro, rf), (seed, r)


def test_entry_point_refuses_bad_arguments_without_a_gpu(mta):
    from music_transcription_amd import _lib
    lib, EINVAL = _lib.lib, -1
    assert lib.mt_note_match_ticks_workspace(0, 0) == 16
    assert lib.mt_note_match_ticks_workspace(3, 5) == 4 * (2 * 3 + 4 * 5) + 8                # (rounded up to 16 bytes)
    assert lib.mt_note_match_ticks_workspace(1000, 2000) == 4 * (2 * 1000 + 4 * 2000)
    assert lib.mt_note_match_ticks_workspace(-1, 0) == 0
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data                                                                      # never dereferenced: every call is refused
    good = dict(est_on=p, est_off=p, est_ptr=p, ref_on=p, ref_off=p, ref_ptr=p, lengths=None, counts=p, B=1, P=88, ws=p, ws_bytes=64)
    order = list(good)
    for change in (dict(est_ptr=None), dict(ref_ptr=None), dict(counts=None), dict(ws=None), dict(est_on=None), dict(ref_off=None),
                   dict(B=0), dict(P=0), dict(B=-3), dict(ws_bytes=15), dict(ws_bytes=0)):
        args = {**good, **change}
        assert lib.mt_note_match_ticks(*(args[k] for k in order), None) == EINVAL, change
        assert "mt_note_match_ticks" in _lib.last_error()
