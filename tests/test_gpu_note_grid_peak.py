"""Peak-picked onsets in the decoder grid on the GPU (DESIGN.md 6c "Peak picking in the decoder grid"): the mt_note_grid_*_peak entry points
(csrc/notes.hip note_peak_grid_kernel) through notes.note_grid_counts(peak_reaches=...) against the single-configuration _peak / _clean
entry points cell by cell and against the numpy restatement, the tiling, the smoothing axis beside the reach axis, the merged triangle
pairs, evaluate.tune_note_decoder(peak_reaches=...), scripts/evaluate.py --tune_peak_reach, and the independence of the counts from
what fresh buffers held.  Integer logic on masks: every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_grid_peak_case as PC  # noqa: E402
import peak_decode_ref as PR  # noqa: E402
from alloc_fill import assert_fill_independent, run_under_fills  # noqa: E402
from note_grid_case import B, LENGTHS, POOL  # noqa: E402
from oracle import model_ref as R  # noqa: E402
from test_gpu_note_sweep import H, L, NM, CountingModel, _model, _tiny_dataset, _write_cache  # noqa: E402

pytestmark = pytest.mark.gpu

G = PC.GRID_PEAK


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


class Dev:
    """The case on the device, the single-configuration entry points called through ctypes, and the device's own activities."""

    def __init__(self):
        self.case = c = PC.Case()
        self.frame, self.onset, self.offset, self.ref = (torch.tensor(a).cuda() for a in (c.frame, c.onset, c.offset, c.ref))
        self.notes = {k: torch.tensor(a).cuda() for k, a in zip(("on", "off", "ptr"), c.notes)}
        self._act = {}

    def ref_of(self, kind):
        return self.ref if kind == "roll" else self.notes

    def act(self, head, thr):
        """mt_predict_threshold's activity: the decoders' expression, evaluated where they evaluate it."""
        from music_transcription_amd.ops import predict_from_logits
        key = (head, float(np.float32(thr)))
        if key not in self._act:
            self._act[key] = predict_from_logits(getattr(self, head), key[1]).cpu().numpy() > 0
        return self._act[key]

    def loop(self, kind, decoder, tf, to, tk, cleanups, reaches, lengths, frame=None):
        """The peak grid's contract, cell by cell: mt_note_match_counts_peak / mt_note_match_list_peak, at reach 0 their _clean namesakes."""
        from music_transcription_amd import _lib
        lib, ptr = _lib.lib, _lib.ptr
        frame = self.frame if frame is None else frame
        off = self.offset if decoder == "onset_offset" else None
        tk = tk if off is not None else [0.5]
        ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
        out = torch.full((len(tf), len(to), len(tk), len(cleanups), len(reaches), B, 4), -7, dtype=torch.int64, device="cuda")
        _, Pn, Tn = frame.shape
        for i, a in enumerate(tf):
            for j, o in enumerate(to):
                for k, kt in enumerate(tk):
                    for c, (M, Gp) in enumerate(cleanups):
                        for r, reach in enumerate(reaches):
                            thr = [float(np.float32(v)) for v in (a, o, kt)]
                            heads = (ptr(frame), ptr(self.onset), ptr(off), *thr)
                            tail = (ptr(ln), ptr(out[i, j, k, c, r]), B, Pn, Tn, int(M), int(Gp), *((int(reach),) if reach else ()),
                                    _lib.stream_ptr())
                            name = ("mt_note_match_counts" if kind == "roll" else "mt_note_match_list") + ("_peak" if reach else "_clean")
                            if kind == "roll":
                                rc = getattr(lib, name)(*heads, ptr(self.ref), *tail)
                            else:
                                rc = getattr(lib, name)(*heads, ptr(self.notes["on"]), ptr(self.notes["off"]), ptr(self.notes["ptr"]), *tail)
                            assert rc == 0, _lib.last_error()
        return out.permute(5, 0, 1, 2, 3, 4, 6).contiguous()

    def grid(self, kind, decoder, tf, to, tk, cleanups, reaches, lengths, **kw):
        from music_transcription_amd.notes import note_grid_counts
        off = self.offset if decoder == "onset_offset" else None
        return note_grid_counts(self.frame, self.ref_of(kind), tf, self.onset, to, off, tk if off is not None else None, cleanups, lengths,
                                peak_reaches=reaches, **kw)


@pytest.fixture(scope="module")
def dev(mta):
    return Dev()


def _differ(got, want):
    return (got != want).nonzero()[:5], got[got != want][:5], want[got != want][:5]


# ---------------------------------------------------------------------------------------------------- 1: cell by cell
@pytest.mark.parametrize("with_lengths", [True, False])
@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("decoder", ["onset", "onset_offset"])
def test_peak_grid_equals_the_single_calls_and_the_numpy_restatement(dev, decoder, kind, with_lengths):
    lengths = LENGTHS if with_lengths else None
    got = dev.grid(kind, decoder, G["tf"], G["to"], G["tk"], G["cleanups"], G["reaches"], lengths)
    Kk = 2 if decoder == "onset_offset" else 1
    assert got.shape == (B, 2, 2, Kk, 2, 4, 4) and got.dtype == torch.int64
    want = dev.loop(kind, decoder, G["tf"], G["to"], G["tk"], G["cleanups"], G["reaches"], lengths)
    assert torch.equal(got, want), _differ(got, want)
    cpu = PC.cpu_counts(dev.case, kind, decoder, G["tf"], G["to"], G["tk"], G["cleanups"], G["reaches"], lengths, act=dev.act)
    np.testing.assert_array_equal(got.cpu().numpy(), cpu)
    assert int(got[..., 0].max()) > 0 and int(got[..., 1].max()) > 0
    for r1 in range(4):                                     # every two reaches differ somewhere: no axis of copies
        for r2 in range(r1 + 1, 4):
            assert not torch.equal(got[..., r1, :], got[..., r2, :])


# ---------------------------------------------------------------------------------------------------- 2: reach 0 alone
@pytest.mark.parametrize("kind", ["roll", "list"])
@pytest.mark.parametrize("decoder", ["onset", "onset_offset"])
def test_reach_zero_alone_is_the_edge_grid(dev, decoder, kind):
    from music_transcription_amd.notes import note_grid_counts
    off = dev.offset if decoder == "onset_offset" else None
    args = (dev.frame, dev.ref_of(kind), G["tf"], dev.onset, G["to"], off, G["tk"] if off is not None else None, PC.GC.CLEANUPS_8, LENGTHS)
    got = note_grid_counts(*args, peak_reaches=[0])
    edge = note_grid_counts(*args)
    assert got.shape == edge.shape[:-1] + (1, 4)
    assert torch.equal(got[..., 0, :], edge), _differ(got[..., 0, :], edge)


# ---------------------------------------------------------------------------------------------------- 3: tiling
def test_a_peak_grid_past_the_kernel_limits_is_split_by_the_wrapper(dev):
    tf, to, tk = [POOL[4], 0.5, POOL[10]], [POOL[3], POOL[8], 0.5], [POOL[6], 0.5, POOL[11]]
    cleanups, reaches = [(1, 0), (3, 2)], [0, 1, 2, 4, 8]
    got = dev.grid("roll", "onset_offset", tf, to, tk, cleanups, reaches, LENGTHS)              # 270 cells, cut on several axes
    assert got.shape == (B, 3, 3, 3, 2, 5, 4)
    want = dev.loop("roll", "onset_offset", tf, to, tk, cleanups, reaches, LENGTHS)
    assert torch.equal(got, want), _differ(got, want)
    every = list(range(9))                                  # Kr = 9: all of 0..8, in one call of the kernel with 4 thresholds
    got = dev.grid("list", "onset", [0.5, POOL[5]], [POOL[4], 0.5], None, [(1, 0)], every, LENGTHS)
    assert got.shape == (B, 2, 2, 1, 1, 9, 4)
    want = dev.loop("list", "onset", [0.5, POOL[5]], [POOL[4], 0.5], None, [(1, 0)], every, LENGTHS)
    assert torch.equal(got, want), _differ(got, want)
    many = [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1, 0]                               # 18 > 16 on the reach axis, repeats
    got = dev.grid("roll", "onset", [0.5], [POOL[4]], None, [(2, 1)], many, LENGTHS)
    want = dev.loop("roll", "onset", [0.5], [POOL[4]], None, [(2, 1)], many, LENGTHS)
    assert torch.equal(got, want), _differ(got, want)


# ---------------------------------------------------------------------------------------------------- 4: with smoothings
@pytest.mark.parametrize("kind", ["roll", "list"])
def test_smoothings_beside_the_reaches(dev, kind):
    from music_transcription_amd.notes import smooth_frame_logits
    tf, to, tk, cleanups, reaches = [0.5, POOL[5]], [POOL[4]], [POOL[10]], [(1, 0), (3, 2)], [0, 2]
    smoothings = [(0.5, 0.25), (2.0, 1.0)]
    got = dev.grid(kind, "onset_offset", tf, to, tk, cleanups, reaches, LENGTHS, smoothings=smoothings)
    assert got.shape == (B, 2, 2, 1, 1, 2, 2, 4)
    for i, a in enumerate(tf):
        for s, (s_on, s_off) in enumerate(smoothings):
            smoothed = smooth_frame_logits(dev.frame, a, s_on, s_off, LENGTHS)
            want = dev.loop(kind, "onset_offset", [a], to, tk, cleanups, reaches, LENGTHS, frame=smoothed)
            assert torch.equal(got[:, i, s], want[:, 0]), (a, s_on, s_off, _differ(got[:, i, s], want[:, 0]))
    assert not torch.equal(got[..., 0, :], got[..., 1, :]) and not torch.equal(got[:, :, 0], got[:, :, 1])


# ---------------------------------------------------------------------------------------------------- 5: triangular targets
def test_triangle_pairs_two_frames_apart_split_at_reach_one(mta):
    """Two strikes of one key 2 frames apart under triangular targets of width J = 2, 4, 8 frames: the onset mask at threshold 0.3 is one
    run, so the edge rule (reach 0) counts one estimate per pair, and reach 1 counts both."""
    from music_transcription_amd.notes import note_grid_counts
    pairs = [(J, on, gap) for J, on, gap in PR.triangle_pairs() if gap in (640, 677)]
    assert sorted({J for J, _, _ in pairs}) == [2, 4, 8] and len(pairs) == 5
    T = 48
    xo = np.full((len(pairs), 1, T), -30.0, np.float32)
    for n, (J, on, gap) in enumerate(pairs):
        y, xo[n, 0] = PR.triangle_row(J, on, gap, T)
        assert y[int(round(on / 320)):int(round((on + gap) / 320)) + 1].min() > 0.3      # no dip below the threshold between the strikes
    xo = torch.from_numpy(xo).cuda()
    xf = torch.full_like(xo, -30.0)
    got = note_grid_counts(xf, torch.zeros_like(xo), [0.5], xo, [0.3], cleanups=[(1, 0), (2, 0)], peak_reaches=[0, 1, 2])
    assert got.shape == (len(pairs), 1, 1, 1, 2, 3, 4)
    n_est = got[:, 0, 0, 0, :, :, 1].cpu().numpy()
    np.testing.assert_array_equal(n_est[:, :, 0], 1)        # reach 0: merged
    np.testing.assert_array_equal(n_est[:, :, 1], 2)        # reach 1: both strikes, with and without the 2-frame minimum
    np.testing.assert_array_equal(n_est[:, :, 2], 1)        # reach 2 compares the two vertices: a tie (gap 640) or the first is higher (677)


# ---------------------------------------------------------------------------------------------------- 6: the tuner
class TriangleOnsetModel(CountingModel):
    """CountingModel whose onset head is replaced by triangular logits around the onsets of the sample's reference roll: vertex height h
    at a note's first frame, 0.1 less per frame of distance over 3 frames, 0.02 elsewhere, h cycling over 0.95 / 0.7 / 0.45 per pitch row."""

    def __init__(self, m, ds):
        super().__init__(m)
        self.ds = ds

    def onset_logits(self, roll):
        roll = roll.numpy() > 0
        y = np.full(roll.shape, 0.02)
        for p in range(roll.shape[0]):
            h = (0.95, 0.7, 0.45)[p % 3]
            for s in np.flatnonzero(roll[p] & ~np.concatenate([[False], roll[p, :-1]])):
                for d in range(-3, 4):
                    if 0 <= s + d < roll.shape[1]:
                        y[p, s + d] = max(y[p, s + d], h - 0.1 * abs(d))
        return torch.from_numpy(np.log(y / (1.0 - y)).astype(np.float32))

    def __call__(self, mel, **k):
        heads = super().__call__(mel, **k)
        if not isinstance(heads, dict):
            return heads
        onset = heads["onset"].clone()
        for b in range(mel.shape[0]):
            (i,) = [n for n, (m, _) in enumerate(self.ds) if m.shape == mel[b].shape and torch.equal(m, mel[b].cpu())]
            onset[b] = self.onset_logits(self.ds[i][1]).to(onset.device)
        return {**heads, "onset": onset}


def _restruck_dataset():
    """_tiny_dataset with every reference note struck again: frame s, a gap, and the rest of the run from s + 2 (two onsets 2 frames apart)."""
    items = []
    for mel, roll in _tiny_dataset():
        roll = roll.clone()
        st = (roll > 0) & ~torch.cat([torch.zeros(88, 1, dtype=torch.bool), roll[:, :-1] > 0], 1)
        for p, s in st.nonzero().tolist():
            if s + 3 < roll.shape[1] and bool((roll[p, s:s + 4] > 0).all()):
                roll[p, s + 1] = 0.0
        items.append((mel, roll))
    return items


def test_tuner_chooses_a_peak_reach_on_restruck_notes(mta):
    from music_transcription_amd import evaluate as E
    ds = _restruck_dataset()
    model = TriangleOnsetModel(_model(mta), ds)
    E._collect(model, ds, list(range(len(ds))), "cuda", None, all_heads=True)
    one_collect, model.calls = model.calls, 0
    assert one_collect > 0
    got = E.tune_note_decoder(model, ds, "cuda", decoder="onset", note_reference="roll", objective="onset", cleanups=((1, 0), (2, 0)),
                              peak_reaches=[0, 1, 2], log=None)
    assert model.calls == one_collect                       # the model ran once, whatever the rounds and candidates
    thr, othr, kthr, clean, (detect, reach), f1 = got
    assert kthr is None and detect == "peak" and reach in (1, 2) and clean in ((1, 0), (2, 0)), got
    at = E.note_metrics_dataset(model, ds, thr, othr, min_note_frames=clean[0], bridge_frames=clean[1], onset_detect="peak", peak_reach=reach)
    assert f1 == pytest.approx(at["mean"]["onset_f1"], abs=1e-12) and at["onset_detect"] == "peak" and at["peak_reach"] == reach
    edge = E.tune_note_decoder(model, ds, "cuda", decoder="onset", note_reference="roll", objective="onset", cleanups=((1, 0), (2, 0)),
                               peak_reaches=[0], log=None)
    plain = E.tune_note_decoder(model, ds, "cuda", decoder="onset", note_reference="roll", objective="onset", cleanups=((1, 0), (2, 0)), log=None)
    assert edge == (*plain[:4], ("edge", 0), plain[4]) and f1 > edge[-1], (edge, plain, f1)
    fixed = E.tune_note_decoder(model, ds, "cuda", decoder="onset", note_reference="roll", objective="onset", peak_reaches=[2],
                                smoothings=[(0.0, 0.0), (1.0, 1.0)], tune_rounds=1, log=None)
    assert len(fixed) == 7 and fixed[5] == ("peak", 2) and fixed[4] in ((0.0, 0.0), (1.0, 1.0))


# ---------------------------------------------------------------------------------------------------- 7: the script
def test_evaluate_script_tunes_the_peak_reach(mta, tmp_path):
    cache = str(tmp_path / "cache")
    _write_cache(mta, cache)
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, L, 5), ckpt)
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--cache_dir", cache, "--split", "test",
            "--model_type", "cnn_rnn_large", "--hidden_size", str(H), "--num_layers", str(L), "--headless", "--note_metrics", "--decoder",
            "onset"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout.strip().splitlines()
    tuned = run(["--tune_note_decoder", "--tune_peak_reach", "0", "1", "2"])
    assert [l.split("=")[0] for l in tuned] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1", "EVAL_NOTE_THRESHOLD",
                                                "EVAL_NOTE_ONSET_THRESHOLD", "EVAL_NOTE_MIN_NOTE_MS", "EVAL_NOTE_BRIDGE_GAP_MS",
                                                "EVAL_NOTE_PEAK_REACH"], tuned
    thr, othr, min_ms, gap_ms, reach = (l.split("=")[1] for l in tuned[3:])
    assert reach in ("0", "1", "2") and (min_ms, gap_ms) == ("0", "0")
    again = run(["--threshold", thr, "--onset_threshold", othr] + (["--onset_detect", "peak", "--peak_reach", reach] if reach != "0" else []))
    assert again[1:3] == tuned[1:3]


# ---------------------------------------------------------------------------------------------------- 8: uninitialised memory
def test_counts_do_not_depend_on_what_fresh_buffers_held(dev):
    """Test 1's smallest configuration (onset-gated, 32 cells) and a tiled, smoothed one (temporaries: the tiles and the packed paths)
    under alloc_fill's 0x00 twice, 0xFF and 0x47; no atomics on floats here, so the comparison is bitwise."""
    def fn():
        return {"roll": dev.grid("roll", "onset", G["tf"], G["to"], None, G["cleanups"], G["reaches"], LENGTHS),
                "list": dev.grid("list", "onset", G["tf"], G["to"], None, G["cleanups"], G["reaches"], LENGTHS),
                "tiled": dev.grid("roll", "onset_offset", G["tf"], G["to"], G["tk"], PC.GC.CLEANUPS_8[:3], list(range(9)), LENGTHS),
                "smoothed": dev.grid("list", "onset", G["tf"], G["to"], None, G["cleanups"], [0, 8], LENGTHS, smoothings=[(1.0, 0.5)])}
    res = run_under_fills(fn)
    spreads = assert_fill_independent(res)
    assert all(s == 0.0 for s in spreads.values()), spreads
    assert all(bool((v != 0).any()) for v in res[0].values())
