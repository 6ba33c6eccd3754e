"""Frame smoothing as an axis of the decoder grid on the GPU: notes.note_grid_counts(smoothings=...) -- one mt_frame_smooth_paths launch per
tile of 16 frame candidates, then mt_note_grid_counts_paths / mt_note_grid_list_paths (csrc/notes.hip; DESIGN.md 6c "Smoothing in the decoder
grid") -- against the numpy restatement of note_grid_case.py given the specification's path (frame_smooth_ref.smooth_ref) as the frame
head's activity, against the single calls with smooth_on / smooth_off cell by cell, the tiling past 16 candidates, smoothings=None, and
evaluate.tune_note_decoder(smoothings=...).  Integer logic throughout: every comparison of counts is exact."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_smooth_ref as FR  # noqa: E402
import note_grid_case as GC  # noqa: E402
from note_grid_case import B, LENGTHS, POOL  # noqa: E402
from note_grid_smooth_case import BLIP_SMOOTHINGS, blip_case, f1_of  # noqa: E402
from test_gpu_note_grid import Dev  # noqa: E402
from test_gpu_note_sweep import _model  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECODERS = ["frame", "onset", "onset_offset"]
TF, TO, TK = [0.5, POOL[5]], [POOL[4], 0.5], [POOL[10], 0.5]
SMOOTHINGS = [(0.0, 0.0), (1.0, 0.5), (2.0, 2.0)]
CLEANUPS = [(1, 0), (3, 2)]


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def dev(mta):
    d = Dev()
    d.paths = {}
    return d


def spec_path(dev, thr, smooth, lengths):
    """The specification's path of the case's frame head, (B, P, T) bool, given the device's own activity; computed once per key."""
    key = (float(np.float32(thr)), smooth, None if lengths is None else tuple(lengths))
    if key not in dev.paths:
        dev.paths[key] = FR.smooth_ref(dev.case.frame, thr, *smooth, lengths, dev.act("frame", thr)) > 0
    return dev.paths[key]


def cpu_grid(dev, kind, decoder, tf, smoothings, to, tk, cleanups, lengths):
    """(B, Kf, Ks, Ko, Kk, Kc, 4): cpu_counts per smoothing, the frame head's activity being the specification's path."""
    per = []
    for s in smoothings:
        act = lambda head, thr, s=s: spec_path(dev, thr, s, lengths) if head == "frame" else dev.act(head, thr)
        per.append(GC.cpu_counts(dev.case, kind, decoder, tf, to, tk, cleanups, lengths, act=act))
    return np.stack(per, axis=2)


def single_calls(dev, kind, decoder, tf, smoothings, to, tk, cleanups, lengths):
    """The same cells through note_match_counts / note_match_list with smooth_on, smooth_off and the cleanup."""
    from music_transcription_amd.notes import note_match_counts, note_match_list
    on, off = dev.heads(decoder)
    to = to if on is not None else [0.5]
    tk = tk if off is not None else [0.5]
    out = torch.empty(B, len(tf), len(smoothings), len(to), len(tk), len(cleanups), 4, dtype=torch.int64, device="cuda")
    call = note_match_counts if kind == "roll" else note_match_list
    for i, a in enumerate(tf):
        for s, (son, soff) in enumerate(smoothings):
            for j, o in enumerate(to):
                for k, kt in enumerate(tk):
                    for c, (M, G) in enumerate(cleanups):
                        out[:, i, s, j, k, c] = call(dev.frame, dev.ref_of(kind), a, on, o, lengths, off, kt, M, G, son, soff)
    return out


def grid(dev, kind, decoder, tf, smoothings, to, tk, cleanups, lengths):
    from music_transcription_amd.notes import note_grid_counts
    on, off = dev.heads(decoder)
    return note_grid_counts(dev.frame, dev.ref_of(kind), tf, on, to if on is not None else None, off, tk if off is not None else None, cleanups,
                            lengths, smoothings=smoothings)


@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("decoder", DECODERS)
def test_every_cell_equals_the_restatement_and_the_single_call(dev, kind, decoder):
    got = grid(dev, kind, decoder, TF, SMOOTHINGS, TO, TK, CLEANUPS, LENGTHS)
    Ko, Kk = (2 if decoder != "frame" else 1), (2 if decoder == "onset_offset" else 1)
    assert got.shape == (B, 2, 3, Ko, Kk, 2, 4) and got.dtype == torch.int64
    want = single_calls(dev, kind, decoder, TF, SMOOTHINGS, TO, TK, CLEANUPS, LENGTHS)
    assert torch.equal(got, want), ((got != want).nonzero()[:5], got[got != want][:5], want[got != want][:5])
    np.testing.assert_array_equal(got.cpu().numpy(), cpu_grid(dev, kind, decoder, TF, SMOOTHINGS, TO, TK, CLEANUPS, LENGTHS))
    tot = got.sum(0)
    assert int(tot[..., 1].max()) > 0 and (tot[:, 0, ..., 1] != tot[:, 2, ..., 1]).any()       # smoothing changes the number of notes
    whole = grid(dev, kind, decoder, TF, SMOOTHINGS, TO, TK, CLEANUPS, None)                  # no lengths: all 1100 frames
    assert torch.equal(whole, single_calls(dev, kind, decoder, TF, SMOOTHINGS, TO, TK, CLEANUPS, None))


@pytest.mark.parametrize("kind", ["roll", "list"])
def test_more_than_sixteen_frame_candidates_are_tiled(dev, kind):
    tf = [POOL[3], 0.5, POOL[11]]
    smoothings = [(0.0, 0.0), (0.5, 0.5), (2.0, 0.0), (0.0, 2.0), (1.0, 1.0), (4.0, 3.0), (64.0, 64.0)]            # 3 x 7 = 21 candidates
    got = grid(dev, kind, "onset", tf, smoothings, [0.5, POOL[4]], None, CLEANUPS, LENGTHS)
    assert got.shape == (B, 3, 7, 2, 1, 2, 4)
    assert torch.equal(got, single_calls(dev, kind, "onset", tf, smoothings, [0.5, POOL[4]], None, CLEANUPS, LENGTHS))
    # and past 64 configurations per path tile: 16 candidates x 2 x 4 cleanups
    cleanups = [(1, 0), (3, 2), (2, 0), (1, 5)]
    got = grid(dev, kind, "onset", tf, smoothings[:6], [0.5, POOL[4]], None, cleanups, LENGTHS)
    assert torch.equal(got, single_calls(dev, kind, "onset", tf, smoothings[:6], [0.5, POOL[4]], None, cleanups, LENGTHS))


@pytest.mark.parametrize("kind", ["roll", "list"])
def test_without_smoothings_nothing_changes_and_no_penalty_is_the_plain_grid(dev, kind):
    from music_transcription_amd.notes import note_grid_counts
    args = (dev.frame, dev.ref_of(kind), TF, dev.onset, TO, dev.offset, TK, CLEANUPS, LENGTHS)
    plain = note_grid_counts(*args)
    assert plain.shape == (B, 2, 2, 2, 2, 4) and torch.equal(note_grid_counts(*args, smoothings=None), plain)
    assert torch.equal(plain, dev.loop(kind, "onset_offset", TF, TO, TK, CLEANUPS, LENGTHS))
    one = note_grid_counts(*args, smoothings=[(0, 0)])
    assert one.shape == (B, 2, 1, 2, 2, 2, 4) and torch.equal(one[:, :, 0], plain)
    for bad in ([], [(0.0,)], [(65.0, 0.0)], [(0.0, -1.0)], 3):
        with pytest.raises(ValueError):
            note_grid_counts(*args, smoothings=bad)


def test_c_abi_of_the_path_grid(dev):
    """The _paths entry points take any words as a frame axis: activity masks packed on the host give the plain grid's counts, and their
    refusals are mt_note_grid_counts' (checked without a GPU in test_note_grid_smooth_cpu.py)."""
    from music_transcription_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    Tn = dev.frame.shape[-1]
    Wn = (Tn + 63) // 64
    acts = np.stack([dev.act("frame", t) for t in TF])                                       # (2, B, P, T)
    ln = torch.tensor(LENGTHS, dtype=torch.int64, device="cuda")
    for b, L in enumerate(LENGTHS):
        acts[:, b, :, L:] = True                                                             # past the length: the kernel masks these bits
    bits = np.zeros(acts.shape[:-1] + (Wn * 64,), bool)
    bits[..., :Tn] = acts
    words = (bits.reshape(acts.shape[:-1] + (Wn, 64)).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    paths = torch.from_numpy(words.view(np.int64)).cuda()
    to, tk = np.float32(TO), np.float32(TK)
    cl = np.asarray(CLEANUPS, np.int32)
    got = torch.empty(B, 2, 2, 2, 2, 4, dtype=torch.int64, device="cuda")
    rc = lib.mt_note_grid_counts_paths(ptr(paths), 2, ptr(dev.onset), ptr(dev.offset), to.ctypes.data, 2, tk.ctypes.data, 2, cl.ctypes.data, 2,
                                       ptr(dev.ref), ptr(ln), ptr(got), B, GC.P, Tn, _lib.stream_ptr())
    assert rc == 0, _lib.last_error()
    assert torch.equal(got, dev.loop("roll", "onset_offset", TF, TO, TK, CLEANUPS, LENGTHS))


# ---------------------------------------------------------------------------------------------------- a batch on which smoothing pays
def test_blips_make_the_smoothed_cell_win_and_the_search_picks_it(mta):
    """note_grid_smooth_case.blip_case: reference runs with strong evidence, distractors of one frame at +0.5 logit.  The cell at (2, 2)
    has strictly higher F1 than the cell at (0, 0) (shown for the specification in test_note_grid_smooth_cpu.py), and a search over
    the two picks it."""
    from music_transcription_amd import evaluate as E
    from music_transcription_amd.notes import note_grid_counts, note_prf
    case = blip_case()
    frame, ref = torch.from_numpy(case.frame).cuda(), torch.from_numpy(case.ref).cuda()
    counts = note_grid_counts(frame, ref, [0.5], smoothings=BLIP_SMOOTHINGS)
    assert counts.shape == (GC.B, 1, 2, 1, 1, 1, 4)
    act = lambda s: (lambda head, thr: FR.smooth_ref(case.frame, thr, *s, None, case.host_act("frame", thr)) > 0)
    for s, smooth in enumerate(BLIP_SMOOTHINGS):
        want = GC.cpu_counts(case, "roll", "frame", [0.5], None, None, [(1, 0)], None, act=act(smooth))
        np.testing.assert_array_equal(counts[:, 0, s, 0, 0, 0].cpu().numpy(), want[:, 0, 0, 0, 0])
    f1 = f1_of(counts.cpu().numpy().reshape(GC.B, 2, 4))
    assert f1[1] > f1[0] and f1[1] == 1.0, f1

    def mean_f1(fts, ots, kts):
        c = note_grid_counts(frame, ref, np.asarray(fts), smoothings=BLIP_SMOOTHINGS)
        v = np.array([m["onset"][2] for m in note_prf(c)]).reshape(GC.B, len(fts), 2, 1, 1, 1)
        return E.fold_smoothings(v).mean(0)
    thr, _, _, d, best = E.search_note_decoder(mean_f1, 1, 2, tune_range=(0.3, 0.7), tune_step=0.2, tune_rounds=1)
    assert E.decoder_candidate(d, [(1, 0)], BLIP_SMOOTHINGS) == ((1, 0), (2.0, 2.0)) and best == pytest.approx(1.0) and thr == pytest.approx(0.5)


# ---------------------------------------------------------------------------------------------------- the tuner
@pytest.mark.parametrize("decoder", ["frame", "onset_offset"])
def test_tuner_with_smoothing_candidates(mta, decoder):
    from music_transcription_amd import evaluate as E
    model = _model(mta, seed=5, nm=16)
    ds = mta.CachedMaestroDataset(os.path.join(GOLDEN, "cache_fixture"), "train")
    smoothings, cleanups = [(0, 0), (1.5, 1.5)], ((1, 0), (3, 1))
    got = E.tune_note_decoder(model, ds, "cuda", decoder=decoder, objective="onset", cleanups=cleanups, smoothings=smoothings, tune_rounds=2,
                              log=None)
    assert len(got) == 6
    thr, othr, kthr, clean, smooth, f1 = got
    assert clean in cleanups and smooth in [(0.0, 0.0), (1.5, 1.5)] and ((othr is None) == (decoder == "frame")) and ((kthr is None) == (othr is None))
    at = E.note_metrics_dataset(model, ds, thr, othr, offset_threshold=kthr, min_note_frames=clean[0], bridge_frames=clean[1],
                                smooth_on=smooth[0], smooth_off=smooth[1])["mean"]["onset_f1"]
    assert f1 == pytest.approx(at, abs=1e-12)
    # one candidate (0, 0): the search of the tuner without the axis, one more entry in the result
    plain = E.tune_note_decoder(model, ds, "cuda", decoder=decoder, objective="onset", cleanups=cleanups, tune_rounds=2, log=None)
    same = E.tune_note_decoder(model, ds, "cuda", decoder=decoder, objective="onset", cleanups=cleanups, smoothings=[(0, 0)], tune_rounds=2, log=None)
    assert len(plain) == 5 and same == plain[:4] + ((0.0, 0.0), plain[4])
