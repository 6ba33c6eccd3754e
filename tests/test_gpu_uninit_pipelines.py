"""The remaining torch.empty callers under poisoned allocations (tests/alloc_fill.py): the front end and the data paths, the decoders
and metrics, and one end-to-end transcription.  Each case is ONE call of a public Python function (on a freshly built object where
it keeps buffers; the cached front-end plans are dropped first) under run_under_fills: 0x00 twice, 0xFF, 0x47.  None of these paths uses float atomics, so every comparison is
bitwise (assert_fill_independent checks that the two control runs agree bitwise before it applies that rule).

Nothing is masked here: the public functions return counts whole, and note lists already cut to their counts -- the entries of
`starts` / `ends` beyond counts[p] (include/mt_hip.h, mt_roll_to_notes: "note k of pitch p is written at [sum of the lower pitches'
counts + k]", nothing beyond the total), the scratch half of smooth_frame_paths' `out` ("The kernel's scratch (as large as the
result) is allocated here") and the pad word of notes_batch_device's `meta` never leave them.

The integer buffers these paths allocate with torch.empty were audited before the first run ("Uninitialised memory"): every
element a kernel uses as an offset, count or loop bound is written by the host (the pinned staging tables of rawdata.py / windows.py)
or by an earlier kernel of the same call (the count pass before the fill pass; the library's own memsets of the metric counts)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import note_grid_case as G
from alloc_fill import BIG_FILL, alloc_fill, assert_fill_independent, run_under_fills
from oracle import frontend_ref, model_ref as R

SR, HOP = 16000, 512


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _check(res, tag):
    spreads = assert_fill_independent(res, tag=tag)
    assert all(s == 0.0 for s in spreads.values()), (tag, "no atomics on these paths: the control runs agree bitwise", spreads)
    return res[0]


def _fresh_frontends():
    """Forget the process-wide front-end plans (frontend.get_frontend caches one per (sr, n_mels, hop, device)), so that the dataset
    and window paths build theirs again, under the fill of the current run."""
    from music_transcription_amd import frontend
    frontend._frontends.clear()


def _notes(lst):
    """[(pitch, start_s, end_s)] -> (n, 3) float64 (a note list is compared whole: it is already cut to its counts)."""
    return torch.tensor([list(n) for n in lst], dtype=torch.float64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("n_mels", [229, 64])
def test_mel_frontend(mta, n_mels):
    wave = torch.from_numpy(frontend_ref.synth_audio(3, 2 * SR, seed=5)).cuda()

    def fn():
        fe = mta.MelFrontend(SR, n_mels, HOP, "cuda")                      # a fresh plan: mt_mel_plan_init writes all the kernel reads
        mel, cmax = fe(wave, clamp=True)
        own = torch.empty(3, dtype=torch.float32, device="cuda")           # the caller's chunk_max buffer: the library clears it
        mel2, cmax2 = fe(wave, clamp=False, chunk_max=own)
        assert cmax2 is own
        return {"mel": mel, "cmax": cmax, "mel_unclamped": mel2, "cmax_own": cmax2}
    ctl = _check(run_under_fills(fn), n_mels)
    assert bool(torch.isfinite(ctl["mel"]).all()) and torch.equal(ctl["cmax"], ctl["cmax_own"]) and float(ctl["cmax"].min()) > 0.0


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from test_gpu_rawdata import _tree
    root = str(tmp_path_factory.mktemp("maestro_uninit"))
    _tree(root, {"a": 7.3, "b": 5.6, "v": 6.2})
    return root


@pytest.mark.parametrize("augmented", [False, True], ids=["plain", "augmented"])
def test_rawdata_window_batches(mta, tree, augmented):
    """MaestroDataset.get_batch: mel, roll and the MIDI onset roll of chunks of unequal length (the last chunk of a recording is
    short: its frames past t_keep are padding the kernels write), plain and with speed jitter + noise."""
    def fn():
        _fresh_frontends()
        aug = mta.Augment(pitch_cents=30.0, snr_db=(5.0, 25.0), generator=torch.Generator().manual_seed(3)) if augmented else None
        ds = mta.MaestroDataset(tree, split="train", n_mels=64, chunk_length=3.0, overlap=0.25, onset_labels="midi", augment=aug)
        assert len(ds) >= 4
        mel, rolls, lengths = ds.get_batch(list(range(len(ds)))[::-1])
        return {"mel": mel, "roll": rolls["frame"], "onset_roll": rolls["onset"], "lengths": lengths}
    ctl = _check(run_under_fills(fn), augmented)
    assert bool(torch.isfinite(ctl["mel"]).all()) and float(ctl["roll"].sum()) > 0.0 and float(ctl["onset_roll"].sum()) > 0.0


def test_full_file_items_and_window_logits(mta, tree):
    """windows.collect_logits_windows over a whole-file dataset: the mel windows, the stitched logits of both heads and the label roll."""
    from music_transcription_amd import windows

    def fn():
        _fresh_frontends()
        ds = mta.MaestroDataset(tree, split="train", n_mels=32, onset_labels="midi")
        m = _large(mta)
        items = windows.collect_logits_windows(m, ds, [0, 1], 1.0, "cuda", all_heads=True, with_offset=True)
        out = {}
        for i, lg, roll, on, off in items:
            out.update({f"frame{i}": lg, f"roll{i}": roll, f"onset{i}": on, f"offset{i}": off})
        return out
    _check(run_under_fills(fn), "collect_logits_windows")


_SD = {}


def _large(mta):
    m = mta.TranscriptionModel("cnn_rnn_large", n_mels=32, hidden_size=16, num_layers=1, device="cuda")
    if "large" not in _SD:
        _SD["large"] = R.make_state_dict("cnn_rnn_large", 32, 16, 1, 71)
    m.load_state_dict(_SD["large"], strict=True)
    return m.eval()


def _small(mta):
    m = mta.TranscriptionModel("cnn_rnn", n_mels=32, hidden_size=32, num_layers=1, device="cuda")
    if "small" not in _SD:
        _SD["small"] = R.make_state_dict("cnn_rnn", 32, 32, 1, 72)
    m.load_state_dict(_SD["small"], strict=True)
    return m.eval()


def test_transcribe_windows_stitched_roll(mta):
    """windows.transcribe_windows on two recordings, one longer than a window (two overlapping windows meet in their overlap) and one
    shorter (one right-aligned window): the stitched logits of all three heads on each recording's own frame grid."""
    from music_transcription_amd import windows
    ys = [torch.from_numpy(frontend_ref.synth_audio(1, n, seed=s)[0]).cuda() for n, s in ((33 * SR + 137, 8), (3 * SR, 9))]

    def fn():
        _fresh_frontends()
        res = windows.transcribe_windows(_large(mta), ys, 2.0, batch=2, all_heads=True, n_mels=32, with_offset=True)
        return {f"{name}{r}": h for r, heads in enumerate(res) for name, h in zip(("frame", "onset", "offset"), heads)}
    ctl = _check(run_under_fills(fn), "transcribe_windows")
    assert ctl["frame0"].shape == (88, 1 + (33 * SR + 137) // HOP) and all(bool(torch.isfinite(v).all()) for v in ctl.values())


@pytest.mark.parametrize("decoder", ["frame", "onset", "onset_offset"])
def test_transcribe_three_seconds_end_to_end(mta, decoder):
    """A three-second synthetic recording -> notes through overlapping windows: the same note list under every fill."""
    from music_transcription_amd import transcribe as TR
    y = torch.from_numpy(frontend_ref.synth_audio(1, 3 * SR, seed=10)[0]).cuda()

    def fn():
        _fresh_frontends()
        m = _small(mta) if decoder == "frame" else _large(mta)
        notes = TR.transcribe_windows_to_notes(m, y, 1.0, threshold=0.5, n_mels=32, decoder=decoder, onset_threshold=0.5,
                                               offset_threshold=0.5, min_note_frames=2, bridge_frames=1, smooth_on=0.25, smooth_off=0.25)
        plain = TR.transcribe_windows_to_notes(m, y, 1.0, threshold=0.5, n_mels=32, decoder=decoder)
        return {"notes": _notes(notes), "notes_plain": _notes(plain)}
    ctl = _check(run_under_fills(fn), decoder)
    assert ctl["notes_plain"].shape[0] > 0, "the case decodes no note at all: it would compare nothing"


# ------------------------------------------------------------------------------------------------------------------ decoders, metrics
@pytest.fixture(scope="module")
def case():
    c = G.Case()
    dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(c, k))).cuda() for k in ("frame", "onset", "offset", "ref")}
    dev["notes"] = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in zip(("on", "off", "ptr"), c.notes)}
    dev["lengths"] = torch.tensor(G.LENGTHS, dtype=torch.int64)
    rng = np.random.default_rng(4)
    dev["pcm_i16"] = torch.from_numpy(rng.integers(-20000, 20000, size=(2 * 44100 + 17, 2)).astype(np.int16)).cuda()
    dev["pcm_f32"] = torch.from_numpy(rng.uniform(-0.8, 0.8, size=(48000 + 5, 1)).astype(np.float32)).cuda()
    return dev


def _decoder_cases():
    from music_transcription_amd import evaluate as E, notes as N, ops, transcribe as TR
    f, o, k, ref, lst, ln = "frame", "onset", "offset", "ref", "notes", "lengths"
    t = G.POOL
    sm = [(0.0, 0.0), (0.5, 0.25), (2.0, 1.0)]
    big_cl = G.CLEANUPS_8
    cases = {
        # ---- metric counts (the library clears them: post.hip mt_f1_counts / mt_f1_sweep_counts)
        "f1_counts": lambda c: {"counts": ops.f1_counts(ops.predict_from_logits(c[f], 0.4), c[ref], c[ln]),
                                "counts_all": ops.f1_counts(ops.predict_from_logits(c[f]), c[ref])},
        "onset_offset_targets": lambda c: dict(zip(("on", "off"), ops.onset_offset_targets(c[ref]))),
        "f1_at_thresholds": lambda c: {"f1": torch.from_numpy(E.f1_at_thresholds(
            [(i, c[f][i, :, :G.LENGTHS[i]].contiguous(), c[ref][i, :, :G.LENGTHS[i]].contiguous()) for i in range(6)], np.linspace(0.05, 0.95, 19)))},
        # ---- note counts against a roll / a note list: plain, onset-gated, offset-gated, cleaned, smoothed
        "match_counts": lambda c: {"frame": N.note_match_counts(c[f], c[ref], t[5], lengths=c[ln]),
                                   "onset": N.note_match_counts(c[f], c[ref], t[5], c[o], t[4], lengths=c[ln]),
                                   "offset": N.note_match_counts(c[f], c[ref], t[5], c[o], t[4], c[ln], c[k], t[10]),
                                   "clean": N.note_match_counts(c[f], c[ref], t[5], c[o], t[4], c[ln], c[k], t[10], 3, 2),
                                   "smooth": N.note_match_counts(c[f], c[ref], t[5], c[o], t[4], c[ln], smooth_on=0.5, smooth_off=0.25),
                                   "no_lengths": N.note_match_counts(c[f], c[ref], 0.5, smooth_on=1.0, smooth_off=1.0)},
        "match_list": lambda c: {"frame": N.note_match_list(c[f], c[lst], t[5], lengths=c[ln]),
                                 "onset": N.note_match_list(c[f], c[lst], t[5], c[o], t[4], lengths=c[ln]),
                                 "offset": N.note_match_list(c[f], c[lst], t[5], c[o], t[4], c[ln], c[k], t[10]),
                                 "clean": N.note_match_list(c[f], c[lst], t[5], c[o], t[4], c[ln], c[k], t[10], 3, 2),
                                 "smooth": N.note_match_list(c[f], c[lst], t[5], c[o], t[4], c[ln], smooth_on=0.5, smooth_off=0.25)},
        # ---- sweeps: one tile (written in place) and a grid past the kernel's limits (tiles pasted into the empty result)
        "sweep_counts": lambda c: {"one_tile": N.note_sweep_counts(c[f], c[ref], t[:4], c[o], t[:4], c[ln]),
                                   "tiles": N.note_sweep_counts(c[f], c[ref], t[:6], c[o], t, c[ln]),
                                   "frame_only": N.note_sweep_counts(c[f], c[ref], t, lengths=c[ln])},
        "sweep_list": lambda c: {"one_tile": N.note_sweep_counts(c[f], c[lst], t[:4], c[o], t[:4], c[ln]),
                                 "tiles": N.note_sweep_counts(c[f], c[lst], t[:6], c[o], t, c[ln])},
        "grid_counts": lambda c: {"one_tile": N.note_grid_counts(c[f], c[ref], lengths=c[ln], onset_logits=c[o], offset_logits=c[k], thresholds=G.GRID_64["tf"],
                                                                 onset_thresholds=G.GRID_64["to"], offset_thresholds=G.GRID_64["tk"], cleanups=big_cl),
                                  "tiles": N.note_grid_counts(c[f], c[ref], t[4:7], c[o], t[3:5], c[k], t[9:11], big_cl, c[ln]),
                                  "smoothed": N.note_grid_counts(c[f], c[ref], t[4:7], c[o], t[3:5], c[k], t[9:11], big_cl[:3], c[ln], smoothings=sm)},
        "grid_list": lambda c: {"tiles": N.note_grid_counts(c[f], c[lst], t[4:7], c[o], t[3:5], c[k], t[9:11], big_cl, c[ln]),
                                "smoothed": N.note_grid_counts(c[f], c[lst], t[4:6], c[o], t[3:5], None, None, big_cl[:3], c[ln], smoothings=sm)},
        # ---- frame smoothing: one wave per row, split rows, chunks, packed paths (the scratch half of `out` stays inside)
        "smooth_logits": lambda c: {"plain": N.smooth_frame_logits(c[f], 0.5, 0.5, 0.25), "ragged": N.smooth_frame_logits(c[f], 0.4, 2.0, 1.0, c[ln]),
                                    "chunks": N.smooth_frame_logits(c[f], 0.5, 0.5, 0.25, chunks=True),
                                    "split": N.smooth_frame_logits(c[f], 0.5, 0.5, 0.25, waves=4),
                                    "chunks_split": N.smooth_frame_logits(c[f], 0.5, 0.5, 0.25, chunks=True, waves=3)},
        "smooth_paths": lambda c: {"paths": N.smooth_frame_paths(c[f], [0.5, 0.4, 0.6], sm, c[ln]),
                                   "many": N.smooth_frame_paths(c[f], 0.5, [(0.125 * i, 0.25) for i in range(20)])},
        # ---- note lists
        "heads_to_notes": lambda c: {"onset": _notes(N.heads_to_notes_device(c[f], c[o], t[5], t[4])),
                                     "offset": _notes(N.heads_to_notes_device(c[f], c[o], t[5], t[4], offset_logits=c[k], offset_threshold=t[10])),
                                     "clean": _notes(N.heads_to_notes_device(c[f], c[o], t[5], t[4], offset_logits=c[k], offset_threshold=t[10],
                                                                             min_note_frames=3, bridge_frames=2)),
                                     "frame_clean_smooth": _notes(N.heads_to_notes_device(c[f], None, 0.5, min_note_frames=2, bridge_frames=1,
                                                                                          smooth_on=0.5, smooth_off=0.25)),
                                     "short_capacity": _notes(N.heads_to_notes_device(c[f].repeat(1, 6, 1), c[o].repeat(1, 6, 1), 0.5, 0.5))},
        "notes_batch": lambda c: {**{f"frame{b}": _notes(l) for b, l in enumerate(N.notes_batch_device(c[f], None, t[5], lengths=c[ln]))},
                                  **{f"onset{b}": _notes(l) for b, l in enumerate(N.notes_batch_device(c[f], c[o], t[5], t[4], c[ln]))},
                                  **{f"clean{b}": _notes(l) for b, l in enumerate(N.notes_batch_device(
                                      c[f], c[o], t[5], t[4], c[ln], min_note_frames=3, bridge_frames=2, smooth_on=0.5, smooth_off=0.25))},
                                  **{f"short_capacity{b}": _notes(l) for b, l in enumerate(N.notes_batch_device(
                                      c[f].repeat(1, 6, 1), c[o].repeat(1, 6, 1), 0.5, 0.5, c[ln]))}},
        "roll_to_notes": lambda c: {"logits": _notes(TR.notes_from_logits_device(c[f], t[5])),
                                    "roll": _notes(TR.notes_from_logits_device(c[ref], is_roll=True)),
                                    "clean": _notes(TR.notes_from_logits_device(c[f], 0.5, min_note_frames=3, bridge_frames=2)),
                                    "smooth": _notes(TR.notes_from_logits_device(c[f], 0.5, smooth_on=0.5, smooth_off=0.25)),
                                    "short_capacity": _notes(TR.notes_from_logits_device(c[f].repeat(1, 6, 1), 0.5))},
        # ---- PCM -> mono 16 kHz (transcribe.py: the output of mt_resample_polyphase is a torch.empty)
        "resample_pcm": lambda c: {"stereo_i16_44k": TR.resample_pcm_device(c["pcm_i16"], 44100),
                                   "mono_f32_48k": TR.resample_pcm_device(c["pcm_f32"], 48000)},
    }
    return cases


DECODER_CASES = ["f1_counts", "onset_offset_targets", "f1_at_thresholds", "match_counts", "match_list", "sweep_counts", "sweep_list", "grid_counts",
                 "grid_list", "smooth_logits", "smooth_paths", "heads_to_notes", "notes_batch", "roll_to_notes", "resample_pcm"]


@pytest.mark.parametrize("name", DECODER_CASES)
def test_decoders_and_metrics(mta, case, name):
    cases = _decoder_cases()
    assert sorted(cases) == sorted(DECODER_CASES)
    ctl = _check(run_under_fills(lambda: cases[name](case)), name)
    empty = [k for k, v in ctl.items() if not bool((v != 0).any())]
    assert len(empty) * 4 <= len(ctl), (name, empty, "the case counts next to nothing")          # (rows of length 0 or 1 decode no note)


def test_short_capacity_cases_do_retry(mta, case):
    """The note-list decoders guess a capacity and launch again when it was short (the count pass has then run twice over buffers of
    two sizes): the 'short_capacity' cases above must really take that path."""
    from music_transcription_amd import notes as N, transcribe as TR
    f6, o6 = case["frame"].repeat(1, 6, 1), case["onset"].repeat(1, 6, 1)
    first_cap = max(1024, G.B * 64)                                                       # heads_to_notes_device, notes_from_logits_device
    n = len(N.heads_to_notes_device(f6, o6, 0.5, 0.5))
    assert n > first_cap, n
    n = len(TR.notes_from_logits_device(f6, 0.5))
    assert n > first_cap, n
    n = sum(len(l) for l in N.notes_batch_device(f6, o6, 0.5, 0.5, case["lengths"]))
    assert n > max(1024, (G.B * G.T) // 16), n                                            # notes_batch_device's first guess


def test_pinned_staging_is_poisoned_too(mta):
    """The harness reaches pinned host memory (the staging tables of rawdata.py / windows.py), which the CPU tests cannot allocate."""
    with alloc_fill(BIG_FILL):
        t = torch.empty((2, 3), dtype=torch.int64, pin_memory=True)
        d = torch.empty(5, dtype=torch.float16, device="cuda")
    assert t.is_pinned() and t.view(torch.uint8).eq(BIG_FILL).all() and bool(d.view(torch.uint8).eq(BIG_FILL).all())
