"""Note-level F1 and onset-gated decoding on the GPU (csrc/notes.hip, notes.py) against the numpy restatement in
note_metrics_ref.py (maximum matching by scipy on mir_eval's compatibility graph)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import note_metrics_ref as NR
from oracle import model_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def _markov(rng, shape, p_on, p_off):
    """Boolean rows of runs: a two-state chain along the last axis."""
    u = rng.random(shape)
    out = np.zeros(shape, bool)
    state = rng.random(shape[:-1]) < p_on / (p_on + p_off)
    for t in range(shape[-1]):
        state = np.where(state, u[..., t] >= p_off, u[..., t] < p_on)
        out[..., t] = state
    return out


def _case(B, P, T, thr, othr, seed):
    """Reference roll, and frame / onset logits whose activity is a jittered, noisy copy of it with re-strikes inside notes.
    Logits keep >= 0.01 from logit(threshold), far outside the band where host and device expf may disagree."""
    rng = np.random.default_rng(seed)
    ref = _markov(rng, (B, P, T), 0.06, 0.2)
    shift = rng.integers(-2, 3, size=(B, P, 1))
    est = np.take_along_axis(ref, np.clip(np.arange(T)[None, None, :] - shift, 0, T - 1), axis=2)
    est ^= rng.random((B, P, T)) < 0.03
    prev = np.concatenate([np.zeros((B, P, 1), bool), est[..., :-1]], axis=2)
    ons = (est & ~prev) & (rng.random((B, P, T)) > 0.1)                     # most note starts, some missed
    ons |= est & (rng.random((B, P, T)) < 0.04)                              # re-strikes inside held notes
    ons |= rng.random((B, P, T)) < 0.005                                     # onsets without frame activity
    mag = lambda: rng.uniform(0.01, 4.0, size=(B, P, T))
    frame = np.where(est, _logit(thr) + mag(), _logit(thr) - mag()).astype(np.float32)
    onset = np.where(ons, _logit(othr) + mag(), _logit(othr) - mag()).astype(np.float32)
    assert (NR.sigmoid_active(frame, thr) == est).all() and (NR.sigmoid_active(onset, othr) == ons).all()
    return frame, onset, ref.astype(np.float32)


CASES = [(1, 1), (3, 63), (3, 64), (3, 65), (1, 938), (128, 938), (2, 47000)]


@pytest.mark.parametrize("B,T", CASES)
@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_match_counts_equal_the_oracle(mta, B, T, decoder):
    from music_transcription_amd.notes import note_match_counts
    P = 88
    k = CASES.index((B, T))
    thr, othr = (0.3, 0.5, 0.7)[k % 3], (0.5, 0.7, 0.3)[k % 3]
    frame, onset, ref = _case(B, P, T, thr, othr, seed=100 + k)
    on = onset if decoder == "onset" else None
    rng = np.random.default_rng(7 + k)
    ragged = [T] + [int(v) for v in rng.integers(0, T + 1, size=B - 1)]
    for lengths in ([None, ragged] if B * T <= 100000 else [ragged]):
        got = note_match_counts(torch.from_numpy(frame).cuda(), torch.from_numpy(ref).cuda(), thr,
                                None if on is None else torch.from_numpy(on).cuda(), othr, lengths).cpu().numpy()
        want = NR.match_counts(frame, ref, thr, on, othr, lengths)
        assert got.dtype == np.int64 and got.shape == (B, 4)
        np.testing.assert_array_equal(got, want, err_msg=f"lengths={'ragged' if lengths else None}")
        assert want[:, 2].sum() > 0 or T < 8


def test_activity_at_the_threshold_equals_predict_threshold(mta):
    """Logits at logit(thr), one ulp either side and densely around it: the notes kernels' activity is mt_predict_threshold's bit
    for bit (device vs device).  Every candidate frame is a one-frame note between strongly inactive frames, so n_est counts active candidates."""
    from music_transcription_amd.notes import note_match_counts
    from music_transcription_amd import ops
    for thr in (0.3, 0.5, 0.7):
        x0 = np.float32(_logit(thr))
        near = [x0, np.nextafter(x0, np.float32(np.inf)), np.nextafter(x0, np.float32(-np.inf))]
        cand = np.concatenate([np.array(near, np.float32), (x0 + np.linspace(-3e-4, 3e-4, 2001)).astype(np.float32)])
        row = np.full(2 * len(cand) + 1, -30.0, np.float32)
        row[1::2] = cand
        x = torch.from_numpy(row).cuda().view(1, 1, -1)
        roll = ops.predict_from_logits(x, thr)
        n_active = int(roll.sum())
        ref = torch.zeros_like(x)
        c_frame = note_match_counts(x, ref, thr).cpu().numpy()[0]
        c_onset = note_match_counts(torch.full_like(x, -30.0), ref, thr, x, thr).cpu().numpy()[0]
        assert 0 < n_active < len(cand)
        assert c_frame[1] == n_active and c_onset[1] == n_active, (thr, n_active, c_frame, c_onset)


def test_frame_decoder_n_est_equals_roll_to_notes(mta):
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import note_match_counts
    B, P, T, thr = 4, 88, 938, 0.5
    frame, _, ref = _case(B, P, T, thr, 0.5, seed=3)
    x = torch.from_numpy(frame).cuda()
    c = note_match_counts(x, torch.from_numpy(ref).cuda(), thr).cpu().numpy()
    for b in range(B):
        counts = torch.empty(P, dtype=torch.int32, device="cuda")
        cap = P * T
        s, e = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib.mt_roll_to_notes(_lib.ptr(x[b:b + 1].contiguous()), 0, thr, 1, P, T, _lib.ptr(counts), _lib.ptr(s), _lib.ptr(e),
                                             cap, _lib.stream_ptr()))
        assert int(counts.sum()) == int(c[b, 1])


def test_heads_to_notes_equals_the_oracle_across_chunks(mta):
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import heads_to_notes_device
    NB, P, T, thr, othr = 3, 88, 938, 0.5, 0.3
    frame, onset, _ = _case(NB, P, T, thr, othr, seed=11)
    # notes that run across the chunk boundaries
    frame[:, 5, -3:] = frame[:, 5, :3] = 3.0
    onset[:, 5, :] = -3.0
    onset[0, 5, -3] = 3.0
    want = NR.heads_notes(frame, onset, thr, othr)
    fs = 16000 / 512
    got = heads_to_notes_device(torch.from_numpy(frame).cuda(), torch.from_numpy(onset).cuda(), thr, othr, fs=fs, min_midi=0)
    assert [(p, int(round(s * fs)), int(round(e * fs))) for p, s, e in got] == want
    assert any(p == 5 and s == T - 3 and e > T for p, s, e in want)
    # capacity protocol: too small a buffer -> counts still right, nothing written past capacity
    x, o = torch.from_numpy(frame).cuda(), torch.from_numpy(onset).cuda()
    counts = torch.empty(P, dtype=torch.int32, device="cuda")
    cap = 8
    s = torch.full((cap + 64,), -7, dtype=torch.int32, device="cuda")
    e = torch.full((cap + 64,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.mt_heads_to_notes(_lib.ptr(x), _lib.ptr(o), thr, othr, NB, P, T, _lib.ptr(counts), _lib.ptr(s), _lib.ptr(e), cap,
                                          _lib.stream_ptr()))
    assert int(counts.sum()) == len(want) > cap
    assert (s[cap:] == -7).all() and (e[cap:] == -7).all()
    got_small_first = heads_to_notes_device(x, o, thr, othr, fs=fs, min_midi=0)      # starts at capacity 1024 < len(want): retries
    assert len(want) > 1024 and len(got_small_first) == len(want)


def test_onset_decoder_with_onset_equal_frame_is_the_frame_decoder(mta):
    from music_transcription_amd.notes import note_match_counts
    frame, _, ref = _case(8, 88, 300, 0.5, 0.5, seed=5)
    x, r = torch.from_numpy(frame).cuda(), torch.from_numpy(ref).cuda()
    assert torch.equal(note_match_counts(x, r, 0.5), note_match_counts(x, r, 0.5, x, 0.5))


def test_bad_arguments_are_refused(mta):
    from music_transcription_amd import _lib
    from music_transcription_amd.notes import note_match_counts
    x = torch.zeros(1, 88, 10, device="cuda")
    with pytest.raises(ValueError):
        note_match_counts(x, x, 1.0)
    c = torch.empty(1, 4, dtype=torch.int64, device="cuda")
    assert _lib.lib.mt_note_match_counts(_lib.ptr(x), None, 0.0, 0.5, _lib.ptr(x), None, _lib.ptr(c), 1, 88, 10, _lib.stream_ptr()) != 0
    assert _lib.lib.mt_note_match_counts(_lib.ptr(x), None, 0.5, 0.5, _lib.ptr(x), None, _lib.ptr(c), 0, 88, 10, _lib.stream_ptr()) != 0
    assert _lib.lib.mt_heads_to_notes(_lib.ptr(x), _lib.ptr(x), 0.5, 1.5, 1, 88, 10, _lib.ptr(c), _lib.ptr(c), _lib.ptr(c), 4,
                                      _lib.stream_ptr()) != 0


# ---------------------------------------------------------------------------------------------------- model-level paths
NM, H, L = 32, 16, 2


def _large(mta, seed=3, heads=True):
    m = mta.TranscriptionModel(model_type="cnn_rnn_large", n_mels=NM, hidden_size=H, num_layers=L, dropout=0.0, device="cuda",
                               use_onset_offset_heads=heads)
    m.load_state_dict(R.make_state_dict("cnn_rnn_large", NM, H, L, seed, use_heads=heads), strict=True)
    m.eval()
    return m


def _dataset(seed=0):
    g = torch.Generator().manual_seed(seed)
    items = []
    for T in (120, 120, 77, 200):
        mel = torch.randn(1, NM, T, generator=g) * 10.0 - 40.0
        roll = torch.from_numpy(_markov(np.random.default_rng(seed + T), (88, T), 0.05, 0.2).astype(np.float32))
        items.append((mel, roll))
    return items


def _mid_threshold(logits):
    """A threshold near the median activation, so that a seeded random model yields plenty of notes."""
    return float(np.clip(torch.sigmoid(logits.float().median()).item(), 0.05, 0.95))


def test_note_metrics_dataset_equals_the_oracle(mta):
    from music_transcription_amd import evaluate as E, ops
    model = _large(mta)
    ds = _dataset()
    with torch.no_grad():
        h = model(ds[0][0][None].cuda(), return_all_heads=True)
    thr, othr = _mid_threshold(h["frame"]), _mid_threshold(h["onset"])
    before = E.evaluate_dataset(model, ds, thr)
    for onset_thr in (None, othr):
        got = E.note_metrics_dataset(model, ds, thr, onset_thr)
        per = {k: [] for k in E.NOTE_METRIC_KEYS}
        for mel, roll in ds:
            with torch.no_grad():
                out = model(mel[None].cuda(), return_all_heads=True)
            f_act = ops.predict_from_logits(out["frame"], thr).cpu().numpy() > 0                  # the device's activity bits
            o_act = None if onset_thr is None else ops.predict_from_logits(out["onset"], onset_thr).cpu().numpy() > 0
            n_ref, n_est, tp_on, tp_onoff = NR.match_counts_active(f_act, roll[None].numpy(), o_act)[0]
            for c, tp in (("onset", tp_on), ("onset_offset", tp_onoff)):
                for k, v in zip(("precision", "recall", "f1"), NR.prf(int(tp), int(n_ref), int(n_est))):
                    per[f"{c}_{k}"].append(v)
        for k in E.NOTE_METRIC_KEYS:
            assert got["per_sample"][k] == pytest.approx(per[k], abs=1e-12), (onset_thr, k)
            assert got["mean"][k] == pytest.approx(float(np.mean(per[k])), abs=1e-12)
        assert sum(per["onset_f1"]) > 0
    after = E.evaluate_dataset(model, ds, thr)
    assert before == after
    lr, lr_h = E.collect_logits(model, ds, range(len(ds))), E.collect_logits(model, ds, range(len(ds)), all_heads=True)
    assert all(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) for a, b in zip(lr, lr_h))
    with pytest.raises(ValueError):
        E.note_metrics_dataset(_large(mta, heads=False), ds, 0.5, 0.5)
    cnn = mta.TranscriptionModel("cnn_rnn", n_mels=NM, hidden_size=H, num_layers=L, device="cuda")
    with pytest.raises(ValueError):
        E.collect_logits(cnn, ds, [0], all_heads=True)


def test_transcribe_chunks_to_notes_decoders(mta):
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    from music_transcription_amd.notes import heads_to_notes_device
    model = _large(mta, seed=9)
    g = torch.Generator(device="cuda").manual_seed(4)
    chunks = 0.2 * torch.randn(2, 480000, device="cuda", generator=g)
    fe = get_frontend(16000, NM, 512, "cuda")
    with torch.no_grad():
        mel, cmax = fe(chunks, clamp=False)
        heads = model.model(mel, chunk_max_power=cmax, return_all_heads=True)
        frame_only = model.model(mel, chunk_max_power=cmax)
    fs = 16000 / 512
    thr, othr = _mid_threshold(frame_only), _mid_threshold(heads["onset"])
    old = tr.notes_from_logits_device(frame_only, thr, fs)
    assert len(old) > 0 and tr.transcribe_chunks_to_notes(model, chunks, thr, n_mels=NM) == old
    want = heads_to_notes_device(heads["frame"].contiguous(), heads["onset"].contiguous(), thr, othr, fs)
    assert len(want) > 0 and tr.transcribe_chunks_to_notes(model, chunks, thr, n_mels=NM, decoder="onset", onset_threshold=othr) == want
    with pytest.raises(ValueError):
        tr.transcribe_chunks_to_notes(_large(mta, heads=False), chunks, 0.5, n_mels=NM, decoder="onset")


def _batches(n, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        mel = torch.randn(B, 1, NM, T, generator=g) * 10.0 - 40.0
        roll = (torch.rand(B, 88, T, generator=g) < 0.1).float()
        out.append((mel, roll, torch.full((B,), T, dtype=torch.int64)))
    return out


@pytest.mark.parametrize("all_heads", [True, False])
def test_train_one_epoch_all_heads(mta, all_heads):
    model = _large(mta, seed=21)
    opt = mta.make_optimizer(model, lr=1e-3)
    seen = []
    orig = model.compute_loss

    def spy(logits, targets, lengths=None):
        seen.append(sorted(logits) if isinstance(logits, dict) else "tensor")
        return orig(logits, targets, lengths)
    model.compute_loss = spy
    w0 = {k: getattr(model.model, k).weight.detach().clone() for k in ("onset_head", "offset_head", "frame_head")}
    avg, losses = mta.train_one_epoch(model, _batches(2, 2, 40, 1), opt, torch.device("cuda"), all_heads=all_heads)
    assert len(losses) == 2 and np.isfinite(avg)
    moved = {k: not torch.equal(w0[k], getattr(model.model, k).weight.detach()) for k in w0}
    assert moved["frame_head"]
    if all_heads:
        assert seen == [["frame", "offset", "onset"]] * 2 and moved["onset_head"] and moved["offset_head"]
    else:
        assert seen == ["tensor"] * 2 and not moved["onset_head"] and not moved["offset_head"]
    from music_transcription_amd import train as T
    assert np.isfinite(T.evaluate(model, _batches(1, 2, 40, 2), torch.device("cuda"), all_heads=all_heads))


def _write_cache(mta, root, T=60):
    rng = np.random.default_rng(0)
    chunks = []
    for i in range(3):
        mel = torch.from_numpy(rng.normal(-40.0, 10.0, size=(1, NM, T)).astype(np.float32))
        roll = torch.from_numpy(_markov(rng, (88, T), 0.05, 0.2).astype(np.float32))
        mta.write_cache_chunk(root, "test", i, mel, roll)
        chunks.append({"file_idx": i, "start_sample": 0, "end_sample": T * 512, "start_time": 0.0, "end_time": T * 512 / 16000})
    mta.write_cache_metadata(root, "test", chunks, chunk_length=T * 512 / 16000, n_mels=NM)


def test_evaluate_script_note_metrics_lines(mta, tmp_path):
    cache = str(tmp_path / "cache")
    _write_cache(mta, cache)
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, L, 5), ckpt)
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", ckpt, "--cache_dir", cache, "--split", "test",
            "--model_type", "cnn_rnn_large", "--hidden_size", str(H), "--num_layers", str(L), "--headless"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    lines = plain.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("EVAL_MEAN_F1=")
    for dec in ("frame", "onset"):
        r = subprocess.run(base + ["--note_metrics", "--decoder", dec], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.strip().splitlines()
        assert [l.split("=")[0] for l in out] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1"], r.stdout
        assert out[0] == lines[0]
        assert all(0.0 <= float(l.split("=")[1]) <= 1.0 and len(l.split("=")[1].split(".")[1]) == 6 for l in out)

