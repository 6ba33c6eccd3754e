"""The threshold sweep of the note decoder on the GPU: mt_note_sweep_counts / mt_note_sweep_list (csrc/notes.hip) against the
single-pair entry points pair by pair (bit for bit) and against the numpy restatements, notes.note_sweep_counts' splitting of large
grids, evaluate.tune_note_thresholds, and scripts/evaluate.py --tune_note_thresholds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_list_ref as LR  # noqa: E402
import note_metrics_ref as NR  # noqa: E402
from oracle import model_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, P, T = 3, 5, 1062                      # rows no multiple of the waves; two slabs of 512 frames and a ragged tail of 38
LENGTHS = [1062, 513, 1]
SEED = 6                                  # 55 of the 64 count rows of the 8 x 8 grid are distinct (checked on the numpy restatement)
POOL = [round(float(v), 3) for v in np.linspace(0.06, 0.94, 16)]           # every grid but the tie grid draws from these


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _markov(rng, shape, p_on, p_off):
    u = rng.random(shape)
    out = np.zeros(shape, bool)
    state = rng.random(shape[:-1]) < p_on / (p_on + p_off)
    for t in range(shape[-1]):
        state = np.where(state, u[..., t] >= p_off, u[..., t] < p_on)
        out[..., t] = state
    return out


def _logits(rng, p_on, p_off, ties):
    """logit(u), u a run-structured process spread over (0.02, 0.98): in a run u is uniform over the upper half, outside over the
    lower, so every threshold moves cells.  u keeps 1e-3 from every threshold of POOL (host and device expf may differ in the last
    bit); `ties` cells are logit 0, whose sigmoid is exactly 0.5 everywhere."""
    run = _markov(rng, (B, P, T), p_on, p_off)
    u = np.where(run, rng.uniform(0.5, 0.98, size=(B, P, T)), rng.uniform(0.02, 0.5, size=(B, P, T)))
    for t in POOL:
        u = np.where(np.abs(u - t) < 1e-3, t + 2e-3, u)
    x = np.log(u / (1.0 - u)).astype(np.float32)
    idx = rng.integers(0, B * P * T, size=ties)
    x.reshape(-1)[idx] = 0.0
    return x


def _restruck_list(rng, ref):
    """The runs of the roll as a note list, with re-struck notes 300-900 ticks after some onsets (the list matcher's multi-edge components)."""
    on, off, ptr = LR.notes_from_roll(ref)
    ons, offs, new_ptr = [], [], [0]
    for r in range(len(ptr) - 1):
        a, b = on[ptr[r]:ptr[r + 1]].astype(np.int64), off[ptr[r]:ptr[r + 1]].astype(np.int64)
        again = rng.random(len(a)) < 0.4
        a2 = a[again] + rng.integers(300, 901, size=int(again.sum()))
        b2 = a2 + rng.integers(1, 4000, size=len(a2))
        aa, bb = np.concatenate([a, a2]), np.concatenate([b, b2])
        order = np.argsort(aa, kind="stable")
        ons.append(aa[order])
        offs.append(bb[order])
        new_ptr.append(new_ptr[-1] + len(aa))
    assert new_ptr[-1] > len(on) + 10
    return np.concatenate(ons).astype(np.int32), np.concatenate(offs).astype(np.int32), np.array(new_ptr, np.int64)


class Case:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.frame = _logits(rng, 0.05, 0.12, ties=40)
        self.onset = _logits(rng, 0.05, 0.5, ties=40)
        self.ref = _markov(rng, (B, P, T), 0.05, 0.15).astype(np.float32)
        self.notes = _restruck_list(rng, self.ref)
        self.d_frame, self.d_onset, self.d_ref = (torch.from_numpy(a).cuda() for a in (self.frame, self.onset, self.ref))
        self.d_notes = {k: torch.from_numpy(a).cuda() for k, a in zip(("on", "off", "ptr"), self.notes)}

    def ref_of(self, kind):
        return self.d_ref if kind == "roll" else self.d_notes

    def single(self, kind, tf, to, onset, lengths):
        from music_transcription_amd.notes import note_match_counts, note_match_list
        on = self.d_onset if onset else None
        if kind == "roll":
            return note_match_counts(self.d_frame, self.d_ref, tf, on, to, lengths)
        return note_match_list(self.d_frame, self.d_notes, tf, on, to, lengths)

    def loop(self, kind, tfs, tos, onset, lengths):
        """The sweep's contract, pair by pair through the single-pair entry points."""
        return torch.stack([torch.stack([self.single(kind, float(np.float32(a)), float(np.float32(b)), onset, lengths) for b in tos], 1)
                            for a in tfs], 1)

    def cpu(self, kind, tfs, tos, onset, lengths):
        out = np.zeros((B, len(tfs), len(tos), 4), np.int64)
        for i, a in enumerate(tfs):
            for j, b in enumerate(tos):
                if kind == "roll":
                    out[:, i, j] = NR.match_counts(self.frame, self.ref, a, self.onset if onset else None, b, lengths)
                else:
                    out[:, i, j] = LR.match_list_counts(self.frame, *self.notes, a, self.onset if onset else None, b, lengths)
        return out


@pytest.fixture(scope="module")
def case(mta):
    return Case(SEED)


GRIDS = {
    (1, 1): ([POOL[7]], [POOL[9]]),
    (3, 5): ([POOL[10], POOL[3], POOL[10]], POOL[2:12:2]),                 # unsorted, one threshold twice
    (8, 8): (POOL[::2], POOL[1::2]),
    (16, 4): (POOL[:5] + [0.5] + POOL[6:], [0.5, POOL[12], POOL[4], POOL[8]]),     # 0.5 is the sigmoid of the logits at 0: `>` leaves them inactive
    (4, 16): (POOL[3:15:3], POOL[::-1]),
}


def test_the_case_is_not_vacuous(case):
    """On the numpy restatement's output for the 8 x 8 grid at least three quarters of the 64 count rows are pairwise distinct, and the
    inputs hold exact ties at 0.5; checked before anything is compared (the seed was chosen on the CPU)."""
    tfs, tos = GRIDS[(8, 8)]
    want = case.cpu("roll", tfs, tos, True, LENGTHS)
    rows = {tuple(want[:, i, j].reshape(-1)) for i in range(8) for j in range(8)}
    assert len(rows) >= 48, len(rows)
    assert (case.frame == 0.0).sum() >= 20 and (case.onset == 0.0).sum() >= 20
    assert want[..., 2].min() >= 0 and want[..., 2].sum() > 0 and (want[..., 3] <= want[..., 2]).all()


@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_onset_decoder_sweep_equals_the_single_calls(case, kind, grid):
    from music_transcription_amd.notes import note_sweep_counts
    tfs, tos = GRIDS[grid]
    assert (len(tfs), len(tos)) == grid
    for lengths in (LENGTHS, None):
        got = note_sweep_counts(case.d_frame, case.ref_of(kind), tfs, case.d_onset, tos, lengths)
        assert got.shape == (B, grid[0], grid[1], 4) and got.dtype == torch.int64
        want = case.loop(kind, tfs, tos, True, lengths)
        assert torch.equal(got, want), (lengths, (got != want).nonzero()[:5])
        if grid == (3, 5):                                                   # and independently of the old kernels
            np.testing.assert_array_equal(got.cpu().numpy(), case.cpu(kind, tfs, tos, True, lengths))
    assert int(got[..., 2].sum()) > 0 and int(got[..., 1].max()) > 0


@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("Kf", [1, 16])
def test_frame_decoder_sweep_equals_the_single_calls(case, kind, Kf):
    from music_transcription_amd.notes import note_sweep_counts
    tfs = [POOL[6]] if Kf == 1 else POOL[8:] + POOL[:8]
    for lengths in (LENGTHS, None):
        got = note_sweep_counts(case.d_frame, case.ref_of(kind), tfs, lengths=lengths)
        assert got.shape == (B, Kf, 1, 4)
        want = case.loop(kind, tfs, [0.5], False, lengths)
        assert torch.equal(got, want), (lengths, (got != want).nonzero()[:5])
        np.testing.assert_array_equal(got.cpu().numpy(), case.cpu(kind, tfs, [0.5], False, lengths))
    tie = note_sweep_counts(case.d_frame, case.ref_of(kind), [0.5, POOL[2]], lengths=LENGTHS)
    assert torch.equal(tie, case.loop(kind, [0.5, POOL[2]], [0.5], False, LENGTHS))


@pytest.mark.parametrize("kind", ["roll", "list"])
def test_a_grid_past_the_kernel_limits_is_split_by_the_wrapper(case, kind):
    from music_transcription_amd.notes import note_sweep_counts
    tfs = np.linspace(0.05, 0.95, 10)
    tos = np.linspace(0.07, 0.93, 10)
    got = note_sweep_counts(case.d_frame, case.ref_of(kind), tfs, case.d_onset, tos, LENGTHS)
    assert got.shape == (B, 10, 10, 4)
    assert torch.equal(got, case.loop(kind, tfs, tos, True, LENGTHS))
    wide = note_sweep_counts(case.d_frame, case.ref_of(kind), np.linspace(0.1, 0.9, 20), lengths=LENGTHS)      # 20 > 16 on one axis
    assert torch.equal(wide, case.loop(kind, np.linspace(0.1, 0.9, 20), [0.5], False, LENGTHS))
    with pytest.raises(ValueError):
        note_sweep_counts(case.d_frame, case.ref_of(kind), [0.5, 1.0], lengths=LENGTHS)
    with pytest.raises(ValueError):
        note_sweep_counts(case.d_frame, case.ref_of(kind), [0.5], case.d_onset, None, LENGTHS)
    with pytest.raises(ValueError):
        note_sweep_counts(case.d_frame, case.ref_of(kind), [0.5], lengths=[5, 5])


def test_two_streams_give_what_one_after_the_other_gives(case):
    """The call takes its thresholds by value and neither allocates nor synchronises, so two calls on two streams may overlap."""
    from music_transcription_amd.notes import note_sweep_counts
    other = Case(SEED + 1)
    tfs, tos = GRIDS[(8, 8)]
    tfs2, tos2 = GRIDS[(4, 16)]
    want_a = note_sweep_counts(case.d_frame, case.d_ref, tfs, case.d_onset, tos, LENGTHS)
    want_b = note_sweep_counts(other.d_frame, other.d_ref, tfs2, other.d_onset, tos2, None)
    assert not torch.equal(want_a[:, :4, :4], want_b[:, :4, :4])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            got_a = note_sweep_counts(case.d_frame, case.d_ref, tfs, case.d_onset, tos, LENGTHS)
        with torch.cuda.stream(s2):
            got_b = note_sweep_counts(other.d_frame, other.d_ref, tfs2, other.d_onset, tos2, None)
        s1.synchronize()
        s2.synchronize()
        assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)


# ---------------------------------------------------------------------------------------------------- the tuner
NM, H, L = 32, 16, 2


def _model(mta, seed=3, nm=NM, h=H, layers=L):
    m = mta.TranscriptionModel(model_type="cnn_rnn_large", n_mels=nm, hidden_size=h, num_layers=layers, dropout=0.0, device="cuda")
    m.load_state_dict(R.make_state_dict("cnn_rnn_large", nm, h, layers, seed), strict=True)
    m.eval()
    return m


def _tiny_dataset(seed=0):
    g = torch.Generator().manual_seed(seed)
    items = []
    for t in (120, 120, 77, 200):
        mel = torch.randn(1, NM, t, generator=g) * 10.0 - 40.0
        roll = torch.from_numpy(_markov(np.random.default_rng(seed + t), (88, t), 0.05, 0.2).astype(np.float32))
        items.append((mel, roll))
    return items


class CountingModel:
    """Counts the forward passes that go through it (collect_logits calls the model; require_heads reads .model)."""

    def __init__(self, m):
        self.m, self.model, self.calls = m, m.model, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.m(*a, **k)


def _check_tuned(E, model, ds, decoder, objective, note_reference, got, **kw):
    thr, othr, f1 = got
    assert (othr is None) == (decoder == "frame") and 0.0 < thr < 1.0
    at = lambda a, b: E.note_metrics_dataset(model, ds, a, b if decoder == "onset" else None, note_reference=note_reference,
                                             **kw)["mean"][objective + "_f1"]
    assert f1 == pytest.approx(at(thr, othr), abs=1e-12)
    first = np.arange(0.05, 0.95 + 0.05, 0.1)
    for a, b in ((first[0], first[0]), (first[0], first[-1]), (first[-1], first[0]), (first[-1], first[-1]), (first[5], first[5])):
        assert f1 >= at(float(a), float(b)), (a, b)
    return f1


@pytest.mark.parametrize("decoder", ["onset", "frame"])
def test_tuner_on_the_roll_reference(mta, decoder):
    from music_transcription_amd import evaluate as E
    model, ds = _model(mta), _tiny_dataset()
    counted = CountingModel(model)
    E._collect(counted, ds, list(range(len(ds))), "cuda", None, all_heads=decoder == "onset")
    one_collect = counted.calls
    assert one_collect > 0
    best = []
    for objective in ("onset", "onset_offset"):
        counted.calls = 0
        got = E.tune_note_thresholds(counted, ds, "cuda", decoder=decoder, note_reference="roll", objective=objective, log=None)
        assert counted.calls == one_collect                                  # the model ran once, whatever the rounds
        best.append(_check_tuned(E, model, ds, decoder, objective, "roll", got))
    assert best[0] > 0.0 and best[0] >= best[1]
    with pytest.raises(ValueError):
        E.tune_note_thresholds(model, ds, "cuda", decoder="both")
    with pytest.raises(ValueError):
        E.tune_note_thresholds(model, ds, "cuda", objective="frames")


def _midi_tree(root):
    """Two short validation recordings with re-struck keys (2000 MIDI ticks per second), as the note-list tests build theirs."""
    from scipy.io import wavfile
    from test_rawdata_cpu import note, smf
    os.makedirs(os.path.join(root, "2004"), exist_ok=True)
    rng = np.random.default_rng(1)
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for i, (name, d) in enumerate((("a", 9.3), ("b", 6.1))):
        n = int(d * 44100)
        t = np.arange(n) / 44100.0
        sig = 0.3 * np.sin(2 * np.pi * 180.0 * (i + 1) * t) * np.exp(-0.5 * (t % 1.3)) + 0.02 * rng.standard_normal(n)
        wavfile.write(os.path.join(root, "2004", f"{name}.wav"), 44100, (np.stack([sig, 0.6 * sig], 1) * 32767).astype(np.int16))
        ev, k, at = [], 0, 400
        while at + 1500 < int((d - 1.0) * 2000):
            p = 40 + (k * 7) % 45
            ev += note(0, p, at, at + 600)
            if k % 2 == 0:
                ev += note(0, p, at + 600, at + 1200)                       # struck again as the note ends
            k, at = k + 1, at + 900
        with open(os.path.join(root, "2004", f"{name}.midi"), "wb") as fh:
            fh.write(smf([[], ev]))
        rows.append(f"X,Y,validation,2004,2004/{name}.midi,2004/{name}.wav,{d}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")


def test_tuner_on_the_midi_reference(mta, tmp_path):
    from music_transcription_amd import evaluate as E
    root = str(tmp_path / "maestro")
    _midi_tree(root)
    nm, h, layers = 64, 24, 3
    model = _model(mta, seed=5, nm=nm, h=h, layers=layers)
    ds = mta.MaestroDataset(root, split="validation", n_mels=nm, onset_labels="midi")
    got = E.tune_note_thresholds(model, ds, "cuda", decoder="onset", note_reference="midi", objective="onset", tune_rounds=2, log=None)
    _check_tuned(E, model, ds, "onset", "onset", "midi", got)
    with pytest.raises(ValueError, match="midi"):
        E.tune_note_thresholds(model, _tiny_dataset(), "cuda", note_reference="midi")


# ---------------------------------------------------------------------------------------------------- the script
def _write_cache(mta, root, t=60):
    rng = np.random.default_rng(0)
    chunks = []
    for i in range(3):
        mel = torch.from_numpy(rng.normal(-40.0, 10.0, size=(1, NM, t)).astype(np.float32))
        roll = torch.from_numpy(_markov(rng, (88, t), 0.05, 0.2).astype(np.float32))
        mta.write_cache_chunk(root, "test", i, mel, roll)
        chunks.append({"file_idx": i, "start_sample": 0, "end_sample": t * 512, "start_time": 0.0, "end_time": t * 512 / 16000})
    mta.write_cache_metadata(root, "test", chunks, chunk_length=t * 512 / 16000, n_mels=NM)


def test_evaluate_script_tunes_the_note_thresholds(mta, tmp_path):
    cache = str(tmp_path / "cache")
    _write_cache(mta, cache)
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, L, 5), ckpt)
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--cache_dir", cache, "--split", "test",
            "--model_type", "cnn_rnn_large", "--hidden_size", str(H), "--num_layers", str(L), "--headless", "--note_metrics", "--decoder", "onset"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.strip().splitlines()
    plain = run([])
    assert [l.split("=")[0] for l in plain] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1"], plain
    tuned = run(["--tune_note_thresholds"])
    assert [l.split("=")[0] for l in tuned] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1", "EVAL_NOTE_THRESHOLD",
                                                "EVAL_NOTE_ONSET_THRESHOLD"], tuned
    assert tuned[0] == plain[0]                                              # framewise F1 keeps --threshold
    thr, othr = tuned[3].split("=")[1], tuned[4].split("=")[1]
    assert all(len(v.split(".")[1]) == 4 and 0.0 < float(v) < 1.0 for v in (thr, othr))
    again = run(["--threshold", thr, "--onset_threshold", othr])
    assert again[1:3] == tuned[1:3]
    r = subprocess.run([a for a in base if a != "--note_metrics"] + ["--tune_note_thresholds"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--note_metrics" in r.stdout
