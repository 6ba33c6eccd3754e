"""The decoder grid on the GPU: mt_note_grid_counts / mt_note_grid_list (csrc/notes.hip note_grid_kernel) against the single-configuration
_clean entry points cell by cell (bit for bit) and against the numpy restatement, notes.note_grid_counts' splitting of large grids,
evaluate.tune_note_decoder, and scripts/evaluate.py --tune_note_decoder.  Integer logic on thresholded activity: every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_grid_case as GC  # noqa: E402
from note_grid_case import B, CLEANUPS_8, GRID_64, LENGTHS, POOL  # noqa: E402
from oracle import model_ref as R  # noqa: E402
from test_gpu_note_sweep import H, L, NM, CountingModel, _model, _tiny_dataset, _write_cache  # noqa: E402

pytestmark = pytest.mark.gpu

DECODERS = ["frame", "onset", "onset_offset"]


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


class Dev:
    """The case on the device, the single-configuration entry points called through ctypes, and the device's own activities."""

    def __init__(self, seed=GC.SEED):
        self.case = GC.Case(seed)
        c = self.case
        self.frame, self.onset, self.offset, self.ref = (torch.tensor(a).cuda() for a in (c.frame, c.onset, c.offset, c.ref))
        self.notes = {k: torch.tensor(a).cuda() for k, a in zip(("on", "off", "ptr"), c.notes)}
        self._act = {}

    def ref_of(self, kind):
        return self.ref if kind == "roll" else self.notes

    def heads(self, decoder):
        return (self.onset if decoder != "frame" else None), (self.offset if decoder == "onset_offset" else None)

    def act(self, head, thr):
        """mt_predict_threshold's activity: the decoders' expression, evaluated where they evaluate it."""
        from music_transcription_amd.ops import predict_from_logits
        key = (head, float(np.float32(thr)))
        if key not in self._act:
            self._act[key] = predict_from_logits(getattr(self, head), key[1]).cpu().numpy() > 0
        return self._act[key]

    def loop(self, kind, decoder, tf, to, tk, cleanups, lengths):
        """The grid's contract, cell by cell through mt_note_match_counts_clean / mt_note_match_list_clean."""
        from music_transcription_amd import _lib
        lib, ptr = _lib.lib, _lib.ptr
        on, off = self.heads(decoder)
        to = to if on is not None else [0.5]
        tk = tk if off is not None else [0.5]
        ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
        out = torch.full((len(tf), len(to), len(tk), len(cleanups), B, 4), -7, dtype=torch.int64, device="cuda")
        _, Pn, Tn = self.frame.shape
        for i, a in enumerate(tf):
            for j, o in enumerate(to):
                for k, kt in enumerate(tk):
                    for c, (M, G) in enumerate(cleanups):
                        thr = [float(np.float32(v)) for v in (a, o, kt)]
                        tail = (ptr(ln), ptr(out[i, j, k, c]), B, Pn, Tn, int(M), int(G), _lib.stream_ptr())
                        if kind == "roll":
                            rc = lib.mt_note_match_counts_clean(ptr(self.frame), ptr(on), ptr(off), *thr, ptr(self.ref), *tail)
                        else:
                            rc = lib.mt_note_match_list_clean(ptr(self.frame), ptr(on), ptr(off), *thr, ptr(self.notes["on"]),
                                                              ptr(self.notes["off"]), ptr(self.notes["ptr"]), *tail)
                        assert rc == 0, _lib.last_error()
        return out.permute(4, 0, 1, 2, 3, 5).contiguous()

    def grid(self, kind, decoder, tf, to, tk, cleanups, lengths):
        from music_transcription_amd.notes import note_grid_counts
        on, off = self.heads(decoder)
        return note_grid_counts(self.frame, self.ref_of(kind), tf, on, to if on is not None else None, off, tk if off is not None else None,
                                cleanups, lengths)


@pytest.fixture(scope="module")
def dev(mta):
    return Dev()


F16 = POOL[:5] + [0.5] + POOL[6:]                                             # 0.5 is the sigmoid of the cells at logit 0: `>` leaves them inactive
CLEANUPS_16 = CLEANUPS_8 + [(2, 1), (5, 0), (1, 7), (16, 16), (33, 1), (2, 40), (64, 1), (63, 62)]
GRIDS = {
    # name: (decoder, frame thresholds, onset thresholds, offset thresholds, cleanups)
    "2x2x2x8": ("onset_offset", GRID_64["tf"], GRID_64["to"], GRID_64["tk"], CLEANUPS_8),
    "1x1x1x1": ("onset_offset", [POOL[7]], [POOL[6]], [0.5], [(1, 0)]),
    "16x1x1x4": ("onset_offset", F16, [0.5], [POOL[9]], [(2, 1), (1, 0), (64, 63), (4, 3)]),
    "3x3x1x5": ("onset", [POOL[4], 0.5, POOL[10]], [POOL[3], POOL[8], 0.5], None, [(1, 0), (3, 2), (1, 63), (64, 0), (10, 5)]),   # 45: no multiple of 8
    "4x1x1x16": ("frame", [POOL[5], 0.5, POOL[9], POOL[12]], None, None, CLEANUPS_16),
    "repeats, descending": ("onset_offset", [POOL[12], POOL[9], POOL[9]], [0.5, 0.5], [POOL[11], POOL[2]], [(3, 2), (1, 0), (3, 2)]),
}


def test_the_case_is_not_vacuous(dev):
    """On the numpy restatement's output for the 2 x 2 x 2 x 8 grid (offset-gated decoder, roll reference; seed 0 of note_grid_case.py,
    chosen on the CPU): 55 of the 64 count rows are distinct (at least three quarters asked), 40 cells differ from their (1, 0) neighbour
    in n_est, and 12 cells differ from their neighbour along the offset axis in tp_onset_offset at equal n_est.  The inputs hold exact ties."""
    case = dev.case
    want = GC.cpu_counts(case, "roll", "onset_offset", GRID_64["tf"], GRID_64["to"], GRID_64["tk"], CLEANUPS_8, LENGTHS)
    rows = {tuple(want[:, i, j, k, c].reshape(-1)) for i in range(2) for j in range(2) for k in range(2) for c in range(8)}
    assert len(rows) >= 48, len(rows)
    tot = want.sum(0)
    assert (tot[..., 1:, 1] != tot[..., :1, 1]).any()                        # cleanup changes the number of notes
    assert ((tot[:, :, 0, :, 3] != tot[:, :, 1, :, 3]) & (tot[:, :, 0, :, 1] == tot[:, :, 1, :, 1])).any()     # the offset head moves ends only
    for x in (case.frame, case.onset, case.offset):
        assert (x == 0.0).sum() >= 20
    assert want[..., 2].sum() > 0 and (want[..., 3] <= want[..., 2]).all()


@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_grid_equals_the_single_calls(dev, kind, grid):
    decoder, tf, to, tk, cleanups = GRIDS[grid]
    for lengths in (LENGTHS, None):
        got = dev.grid(kind, decoder, tf, to, tk, cleanups, lengths)
        shape = (B, len(tf), len(to or [0]), len(tk or [0]), len(cleanups), 4)
        assert got.shape == shape and got.dtype == torch.int64
        want = dev.loop(kind, decoder, tf, to, tk, cleanups, lengths)
        assert torch.equal(got, want), (lengths, (got != want).nonzero()[:5], got[got != want][:5], want[got != want][:5])
    assert int(got[..., 0].max()) > 0 and int(got[..., 1].max()) > 0


@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("decoder", DECODERS)
def test_grid_equals_the_numpy_restatement_on_some_cells(dev, kind, decoder):
    tf, to, tk, cleanups = [0.5, POOL[5]], [POOL[4]], [POOL[10]], [(3, 2), (64, 63), (1, 63), (1, 0)]
    for lengths in (LENGTHS, None):
        got = dev.grid(kind, decoder, tf, to, tk, cleanups, lengths).cpu().numpy()
        want = GC.cpu_counts(dev.case, kind, decoder, tf, to, tk, cleanups, lengths, act=dev.act)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("kind", ["roll", "list"])
def test_no_cleanup_and_no_offset_head_is_the_threshold_sweep(dev, kind):
    from music_transcription_amd.notes import note_grid_counts, note_sweep_counts
    tf, to = POOL[::2], POOL[1::2]
    got = note_grid_counts(dev.frame, dev.ref_of(kind), tf, dev.onset, to, lengths=LENGTHS)
    assert got.shape == (B, 8, 8, 1, 1, 4)
    assert torch.equal(got.reshape(B, 8, 8, 4), note_sweep_counts(dev.frame, dev.ref_of(kind), tf, dev.onset, to, LENGTHS))
    got = note_grid_counts(dev.frame, dev.ref_of(kind), F16, lengths=LENGTHS)
    assert torch.equal(got.reshape(B, 16, 1, 4), note_sweep_counts(dev.frame, dev.ref_of(kind), F16, lengths=LENGTHS))


def test_a_grid_past_the_kernel_limits_is_split_by_the_wrapper(dev):
    from music_transcription_amd.notes import note_grid_counts
    tf, to, tk = np.linspace(0.2, 0.8, 5), np.linspace(0.25, 0.75, 5), np.linspace(0.3, 0.7, 4)
    cleanups = [(1, 0), (3, 2), (6, 0)]
    got = dev.grid("roll", "onset_offset", tf, to, tk, cleanups, LENGTHS)
    assert got.shape == (B, 5, 5, 4, 3, 4)
    assert torch.equal(got, dev.loop("roll", "onset_offset", tf, to, tk, cleanups, LENGTHS))
    many = [(m, 0) for m in range(1, 21)]                                    # 20 > 16 on the cleanup axis
    got = dev.grid("list", "frame", [0.5], None, None, many, LENGTHS)
    assert torch.equal(got, dev.loop("list", "frame", [0.5], None, None, many, LENGTHS))
    with pytest.raises(ValueError):
        note_grid_counts(dev.frame, dev.ref, [0.5, 1.0])
    with pytest.raises(ValueError):
        note_grid_counts(dev.frame, dev.ref, [0.5], dev.onset, None)
    with pytest.raises(ValueError):
        note_grid_counts(dev.frame, dev.ref, [0.5], None, None, dev.offset, [0.5])
    with pytest.raises(ValueError):
        note_grid_counts(dev.frame, dev.ref, [0.5], cleanups=[(0, 0)])
    with pytest.raises(ValueError):
        note_grid_counts(dev.frame, dev.ref, [0.5], cleanups=[])


def test_two_streams_give_what_one_after_the_other_gives(dev):
    """The call takes its thresholds and cleanups by value and neither allocates nor synchronises, so two calls on two streams may overlap."""
    other = Dev(GC.SEED + 1)
    a = GRIDS["2x2x2x8"]
    b = GRIDS["3x3x1x5"]
    want_a = dev.grid("roll", *a, LENGTHS)
    want_b = other.grid("roll", *b, None)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            got_a = dev.grid("roll", *a, LENGTHS)
        with torch.cuda.stream(s2):
            got_b = other.grid("roll", *b, None)
        s1.synchronize()
        s2.synchronize()
        assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)


# ---------------------------------------------------------------------------------------------------- the tuner
@pytest.mark.parametrize("decoder", ["onset", "frame"])
def test_tuner_without_cleanup_is_tune_note_thresholds(mta, decoder):
    from music_transcription_amd import evaluate as E
    model, ds = _model(mta), _tiny_dataset()
    old = E.tune_note_thresholds(model, ds, "cuda", decoder=decoder, note_reference="roll", objective="onset", log=None)
    new = E.tune_note_decoder(model, ds, "cuda", decoder=decoder, note_reference="roll", objective="onset", cleanups=((1, 0),), log=None)
    assert new == (old[0], old[1], None, (1, 0), old[2]), (old, new)


def test_tuner_on_the_offset_gated_decoder_equals_brute_force(mta):
    from music_transcription_amd import evaluate as E
    model, ds = _model(mta), _tiny_dataset()
    counted = CountingModel(model)
    E._collect(counted, ds, list(range(len(ds))), "cuda", None, all_heads=True, with_offset=True)
    one_collect = counted.calls
    assert one_collect > 0
    cleanups = ((1, 0), (3, 1))
    for objective in ("onset", "onset_offset"):
        counted.calls = 0
        got = E.tune_note_decoder(counted, ds, "cuda", decoder="onset_offset", note_reference="roll", objective=objective, cleanups=cleanups,
                                  tune_range=(0.3, 0.7), tune_step=0.2, tune_rounds=1, log=None)
        assert counted.calls == one_collect                                  # the model ran once
        ths = np.arange(0.3, 0.7 + 0.1, 0.2)
        assert len(ths) == 3
        best, best_v = (0.5, 0.5, 0.5, cleanups[0]), -1.0                    # the 54 configurations in the search's order, strict improvement
        for a in ths:
            for o in ths:
                for k in ths:
                    for c in cleanups:
                        v = E.note_metrics_dataset(model, ds, float(a), float(o), offset_threshold=float(k), min_note_frames=c[0],
                                                   bridge_frames=c[1])["mean"][objective + "_f1"]
                        if v > best_v:
                            best, best_v = (float(a), float(o), float(k), c), v
        assert got[:4] == best, (got, best, best_v)
        assert got[4] == pytest.approx(best_v, abs=1e-12) and best_v > 0.0
    # more rounds: the value is still the single-configuration kernels' at the configuration returned
    thr, othr, kthr, c, f1 = E.tune_note_decoder(model, ds, "cuda", decoder="onset_offset", objective="onset", cleanups=cleanups, tune_rounds=2,
                                                 log=None)
    at = E.note_metrics_dataset(model, ds, thr, othr, offset_threshold=kthr, min_note_frames=c[0], bridge_frames=c[1])["mean"]["onset_f1"]
    assert f1 == pytest.approx(at, abs=1e-12) and c in cleanups
    with pytest.raises(ValueError):
        E.tune_note_decoder(model, ds, "cuda", decoder="both")
    with pytest.raises(ValueError):
        E.tune_note_decoder(model, ds, "cuda", cleanups=((0, 0),))


# ---------------------------------------------------------------------------------------------------- the script
def test_evaluate_script_tunes_the_note_decoder(mta, tmp_path):
    cache = str(tmp_path / "cache")
    _write_cache(mta, cache)
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, L, 5), ckpt)
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--cache_dir", cache, "--split", "test",
            "--model_type", "cnn_rnn_large", "--hidden_size", str(H), "--num_layers", str(L), "--headless", "--note_metrics", "--decoder",
            "onset_offset"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.strip().splitlines()
    tuned = run(["--tune_note_decoder", "--tune_min_note_ms", "0", "64", "--tune_bridge_gap_ms", "0", "32"])
    assert [l.split("=")[0] for l in tuned] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1", "EVAL_NOTE_THRESHOLD",
                                                "EVAL_NOTE_ONSET_THRESHOLD", "EVAL_NOTE_OFFSET_THRESHOLD", "EVAL_NOTE_MIN_NOTE_MS",
                                                "EVAL_NOTE_BRIDGE_GAP_MS"], tuned
    thr, othr, kthr, min_ms, gap_ms = (l.split("=")[1] for l in tuned[3:])
    assert all(len(v.split(".")[1]) == 4 and 0.0 < float(v) < 1.0 for v in (thr, othr, kthr))
    assert min_ms in ("0", "64") and gap_ms in ("0", "32")
    again = run(["--threshold", thr, "--onset_threshold", othr, "--offset_threshold", kthr, "--min_note_ms", min_ms, "--bridge_gap_ms", gap_ms])
    assert again[1:3] == tuned[1:3]
