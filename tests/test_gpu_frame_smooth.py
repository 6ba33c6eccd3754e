"""Frame smoothing on the GPU (csrc/smooth.hip, mt_frame_smooth / mt_frame_smooth_chunks, notes.py; DESIGN.md 6c "Frame smoothing") against the
literal specification of frame_smooth_ref.py: random rows over the length, slab and workgroup boundaries, rows built to stress the two
carries, the chunk layout, (0, 0) against the threshold kernel, the decoders behind smooth_on / smooth_off, the C ABI's refusals and
main.py.  The kernel is integer arithmetic on quantised evidence, so every comparison is exact.  The reference is given the activity
the library itself thresholds (mt_predict_threshold): the sign of the evidence follows it bit for bit, whatever expf rounds to."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frame_smooth_ref as FR
from oracle import model_ref as R
from test_gpu_offset_decoder import _midi_notes, _mid_threshold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, P, T = 3, 3, 1100                                # 9 rows against 4 waves per workgroup; 1100 frames: past one slab of 16 x 64
LENGTH_SETS = [(0, 1, 63), (64, 65, 127), (128, 129, 1024), (1025, 1100, 1)]
PENALTIES = [(0.0, 0.0), (0.5, 0.5), (2.0, 0.0), (0.0, 2.0), (64.0, 64.0)]
THRESHOLDS = (0.3, 0.5, 0.8)
SENTINEL = -7.0
EINVAL = -1


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _raw():
    from music_transcription_amd import _lib
    return _lib.lib, _lib.ptr, _lib.stream_ptr


def raw_smooth(x, thr, on, off, lengths=None, out=None):
    """mt_frame_smooth called directly -> rc, out (a tensor of sentinels where the kernel writes nothing)."""
    lib, ptr, stream = _raw()
    Bn, Pn, Tn = x.shape
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
    out = torch.full_like(x, SENTINEL) if out is None else out
    rc = lib.mt_frame_smooth(ptr(x), ptr(out), thr, on, off, ptr(ln), Bn, Pn, Tn, stream())
    torch.cuda.synchronize()
    return rc, out


def raw_smooth_chunks(x, thr, on, off, out=None):
    lib, ptr, stream = _raw()
    NB, Pn, Tn = x.shape
    out = torch.full_like(x, SENTINEL) if out is None else out
    rc = lib.mt_frame_smooth_chunks(ptr(x), ptr(out), thr, on, off, NB, Pn, Tn, stream())
    torch.cuda.synchronize()
    return rc, out


def _activity(x, thr):
    from music_transcription_amd import ops
    return ops.predict_from_logits(x.contiguous().float(), thr).cpu().numpy() > 0


def _expect(x, thr, on, off, lengths=None):
    """x (B, P, T) on the device -> what raw_smooth leaves: the specification on the valid frames, the sentinel elsewhere."""
    want = FR.smooth_ref(x.cpu().numpy(), thr, on, off, lengths, _activity(x, thr))
    if lengths is not None:
        for b, L in enumerate(lengths):
            want[b, :, L:] = SENTINEL
    return want


_CASE = {}


def _random_case():
    """Noisy evidence around Markov runs, so that every penalty finds blips, dropouts and long stretches inside the band; the first
    pitch on the 1/64 grid, the others off it; a few infinities.  Built once, nobody writes to it."""
    if not _CASE:
        from offset_decode_ref import markov
        rng = np.random.default_rng(11)
        runs = markov(rng, (B, P, T), 0.05, 0.08)
        x = (rng.normal(0, 1.0, (B, P, T)) + np.where(runs, 1.0, -1.0) * rng.choice([0.3, 1.5], (B, P, 1))).astype(np.float32)
        x[:, 0] = np.round(x[:, 0] * 64) / 64
        x[1, 1, 40], x[1, 1, 700], x[2, 2, 64], x[2, 2, 1087] = np.inf, -np.inf, 80.0, -80.0
        x.setflags(write=False)
        _CASE.update(x=x, dev=torch.from_numpy(x.copy()).cuda())
    return _CASE


@pytest.mark.parametrize("on,off", PENALTIES)
def test_random_rows_equal_the_specification(mta, on, off):
    x = _random_case()["dev"]
    changed = 0
    for thr in THRESHOLDS:
        for lengths in LENGTH_SETS:
            poisoned = x.clone()
            for b, L in enumerate(lengths):
                poisoned[b, :, L:] = float("nan")                                # frames that must never be read
            rc, got = raw_smooth(poisoned, thr, on, off, list(lengths))
            want = _expect(poisoned, thr, on, off, lengths)
            assert rc == 0 and np.array_equal(got.cpu().numpy(), want), (thr, lengths)
        rc, got = raw_smooth(x, thr, on, off)                                    # no lengths: all T frames
        want = _expect(x, thr, on, off)
        assert rc == 0 and np.array_equal(got.cpu().numpy(), want), thr
        assert set(np.unique(want)) <= {np.float32(-64.0), np.float32(64.0)}
        changed += int(((want > 0) != _activity(x, thr)).sum())
        buf = x.clone()
        rc, same = raw_smooth(buf, thr, on, off, out=buf)                        # in place
        assert rc == 0 and same is buf and np.array_equal(buf.cpu().numpy(), want)
    assert (changed > 100) == ((on, off) != (0.0, 0.0))                          # the penalties do change paths; (0, 0) changes none


def test_a_nan_inside_the_row_counts_as_the_strongest_evidence_against(mta):
    x = torch.full((1, 1, 200), 1.0, device="cuda")
    x[0, 0, 100] = float("nan")
    rc, got = raw_smooth(x, 0.5, 64.0, 64.0)
    assert rc == 0 and np.array_equal(got.cpu().numpy(), _expect(x, 0.5, 64.0, 64.0)) and (got > 0).all()      # 4096 < a + b: bridged
    rc, got = raw_smooth(x, 0.5, 20.0, 20.0)
    want = np.full((1, 1, 200), 64.0, np.float32)
    want[0, 0, 100] = -64.0                                                      # 4096 > 2560: the path leaves for that frame
    assert rc == 0 and np.array_equal(got.cpu().numpy(), want) and np.array_equal(_expect(x, 0.5, 20.0, 20.0), want)


# ------------------------------------------------------------------------------------------------ rows built for the carries
def _carry_rows():
    """-> x (N, 1, 768), lengths, names.  Penalties (2, 2): a = b = 128; +-0.1 logits are 6 grid steps, so alternating them keeps d
    inside the band, and a logit of +-5 is decisive on its own."""
    Tn = 768
    wiggle = np.where(np.arange(Tn) % 2 == 0, 0.1, -0.1).astype(np.float32)
    rows, lengths, names = [], [], []

    def add(name, row, L=Tn):
        rows.append(row.astype(np.float32))
        lengths.append(L)
        names.append(name)
    for sign in (1.0, -1.0):
        r = wiggle.copy()
        r[0], r[300], r[600] = -5.0 * sign, 5.0 * sign, -5.0 * sign               # 299 undecided frames below a decisive one: > 4 windows;
        r[1], r[301] = 1.0 * sign, -1.0 * sign                                   # (a logit of 1 brings d from the band's edge to its middle)
        add(f"band{sign:+.0f}", r)
    r = wiggle.copy()
    for k in range(0, Tn, 128):
        r[k], r[k + 63] = 5.0, -5.0                                              # decisive exactly on lanes 0 and 63,
        r[k + 64], r[k + 127] = -5.0, 5.0                                        # either way round
    add("lanes", r)
    for L in (703, 704, 640, 128, 64, 65):                                       # resolved by the last frame alone: its parity decides;
        add(f"last{L}", wiggle.copy(), L)                                        # 704, 640, 128, 64: L a multiple of 64
        add(f"last{L}-", -wiggle, L)
    return np.stack(rows)[:, None, :], lengths, names


def test_rows_that_stress_the_carries(mta):
    x, lengths, names = _carry_rows()
    dev = torch.from_numpy(x).cuda()
    rc, got = raw_smooth(dev, 0.5, 2.0, 2.0, lengths)
    want = _expect(dev, 0.5, 2.0, 2.0, lengths)
    got = got.cpu().numpy()
    for n, name in enumerate(names):
        assert rc == 0 and np.array_equal(got[n], want[n]), name
    path = {name: want[n, 0, :lengths[n]] > 0 for n, name in enumerate(names)}    # and the rows do what they are named for
    for name in ("band+1", "band-1"):
        d = FR.forward_d(FR.quantise(x[names.index(name), 0], 0.5), 128, 128)
        assert (np.abs(d[1:300]) < 128).all() and (np.abs(d[301:600]) < 128).all() and all(abs(d[t]) > 128 for t in (0, 300, 600))
    assert not path["band+1"][0] and path["band+1"][1:301].all() and not path["band+1"][301:].any()
    assert path["band-1"][0] and not path["band-1"][1:301].any() and path["band-1"][301:].all()
    assert path["lanes"][0] and not path["lanes"][63] and not path["lanes"][64] and path["lanes"][127]
    for L in (703, 704, 640, 128, 64, 65):                                       # d of the last frame is 6 or 0 (-6 or 0): one state all along
        assert path[f"last{L}"].all() == (L % 2 == 1) and path[f"last{L}"].any() == (L % 2 == 1)
        assert not path[f"last{L}-"].any()


# ------------------------------------------------------------------------------------------------ the chunk layout
def _cat(x):
    """(NB, P, T) chunks -> (1, P, NB * T): the recording they are."""
    return x.permute(1, 0, 2).reshape(1, x.shape[1], -1).contiguous()


def _uncat(y, NB):
    return y.reshape(y.shape[1], NB, -1).permute(1, 0, 2).contiguous()


def test_chunks_are_one_recording(mta):
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.normal(0, 1.2, (3, 2, 70)).astype(np.float32)).cuda()      # 210 frames: chunk boundaries inside windows
    for on, off in PENALTIES[1:]:
        rc, got = raw_smooth_chunks(x, 0.5, on, off)
        rc2, whole = raw_smooth(_cat(x), 0.5, on, off)
        assert rc == 0 and rc2 == 0 and torch.equal(_cat(got), whole)
        assert np.array_equal(whole.cpu().numpy(), _expect(_cat(x), 0.5, on, off))
    two = np.where(np.arange(140) % 2 == 0, 0.1, -0.1).astype(np.float32).reshape(2, 1, 70)           # undecided all along at (2, 2) ...
    two[1, 0, 5] = 5.0                                                           # ... but for one frame of the second chunk
    two = torch.from_numpy(two).cuda()
    rc, got = raw_smooth_chunks(two, 0.5, 2.0, 2.0)
    rc2, alone = raw_smooth(two[:1].contiguous(), 0.5, 2.0, 2.0)
    assert rc == 0 and rc2 == 0 and (got[0] == 64.0).all() and (alone == -64.0).all()             # the backward carry crosses the chunks,
    assert np.array_equal(_cat(got).cpu().numpy(), _expect(_cat(two), 0.5, 2.0, 2.0))                # as the specification has it
    big =_random_case()["dev"]                                                  # 3 x 1100 frames: past one slab, T no multiple of 64
    rc, got = raw_smooth_chunks(big, 0.3, 2.0, 0.5)
    assert rc == 0 and np.array_equal(_cat(got).cpu().numpy(), _expect(_cat(big), 0.3, 2.0, 0.5))
    buf = big.clone()
    rc, _ = raw_smooth_chunks(buf, 0.3, 2.0, 0.5, out=buf)                       # in place
    assert rc == 0 and torch.equal(buf, got)


# ------------------------------------------------------------------------------------------------ (0, 0) is the threshold
def test_no_penalty_through_the_kernel_is_the_threshold(mta):
    rng = np.random.default_rng(13)
    x = rng.normal(0, 0.05, (2, 3, 1100)).astype(np.float32)                     # crowded around the thresholds' logits
    for i, thr in enumerate(THRESHOLDS):
        c = FR.centre(thr)
        x[0, i, :5] = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)), c - np.float32(1e-3), c + np.float32(1e-3)]
        x[1, i] += c
    dev = torch.from_numpy(x).cuda()
    for thr in THRESHOLDS:
        rc, got = raw_smooth(dev, thr, 0.0, 0.0)
        act = _activity(dev, thr)
        assert rc == 0 and np.array_equal(got.cpu().numpy() > 0, act) and 0 < act.mean() < 1
        assert np.array_equal(_activity(got, thr), act) and np.array_equal(_activity(got, 1e-6), act) and np.array_equal(_activity(got, 1 - 1e-6), act)


# ------------------------------------------------------------------------------------------------ behind the decoders
@pytest.mark.parametrize("decoder", ["frame", "onset", "onset_offset"])
def test_the_decoders_smooth_first_and_then_proceed_as_ever(mta, decoder):
    from music_transcription_amd.notes import heads_to_notes_device, note_match_counts, note_match_list, notes_batch_device
    from music_transcription_amd.transcribe import notes_from_logits_device
    from offset_decode_ref import markov
    rng = np.random.default_rng(14)
    x = _random_case()["dev"]
    hi, lo = 2.0, -2.0
    heads = lambda p_on: torch.from_numpy(np.where(markov(rng, (B, P, T), p_on, 0.6), hi, lo).astype(np.float32)).cuda()
    on = heads(0.03) if decoder != "frame" else None
    off = heads(0.03) if decoder == "onset_offset" else None
    ref = torch.from_numpy(markov(rng, (B, P, T), 0.02, 0.05).astype(np.float32)).cuda()
    thr, lengths = 0.5, [1100, 1025, 640]
    sm_chunks = _uncat(torch.from_numpy(_expect(_cat(x), thr, 1.0, 1.0)).cuda(), B)
    sm_batch = torch.from_numpy(FR.smooth_ref(x.cpu().numpy(), thr, 1.0, 1.0, lengths, _activity(x, thr))).cuda()
    assert not np.array_equal(sm_chunks.cpu().numpy() > 0, _activity(x, thr))
    for clean in ((1, 0), (3, 2)):
        kw = dict(min_note_frames=clean[0], bridge_frames=clean[1])
        if decoder == "frame" and clean == (1, 0):
            got, want, plain = (notes_from_logits_device(x, thr, 1.0, 0, smooth_on=1.0, smooth_off=1.0), notes_from_logits_device(sm_chunks, thr, 1.0, 0),
                                notes_from_logits_device(x, thr, 1.0, 0))
        else:
            got = heads_to_notes_device(x, on, thr, 0.5, 1.0, 0, off, 0.5, smooth_on=1.0, smooth_off=1.0, **kw)
            want = heads_to_notes_device(sm_chunks, on, thr, 0.5, 1.0, 0, off, 0.5, **kw)
            plain = heads_to_notes_device(x, on, thr, 0.5, 1.0, 0, off, 0.5, **kw)
        assert len(want) > 0 and got == want and got != plain
        got = note_match_counts(x, ref, thr, on, 0.5, lengths, off, 0.5, smooth_on=1.0, smooth_off=1.0, **kw)
        want = note_match_counts(sm_batch, ref, thr, on, 0.5, lengths, off, 0.5, **kw)
        assert torch.equal(got, want) and int(got[:, 1].sum()) > 0
        if decoder != "onset_offset":
            got = notes_batch_device(x, on, thr, 0.5, lengths, 1.0, 0, smooth_on=1.0, smooth_off=1.0, **kw)
            assert got == notes_batch_device(sm_batch, on, thr, 0.5, lengths, 1.0, 0, **kw) and sum(len(g) for g in got) > 0
    tables = {"on": torch.zeros(0, dtype=torch.int32, device="cuda"), "off": torch.zeros(0, dtype=torch.int32, device="cuda"),
              "ptr": torch.zeros(B * P + 1, dtype=torch.int64, device="cuda")}
    got = note_match_list(x, tables, thr, on, 0.5, lengths, off, 0.5, smooth_on=1.0, smooth_off=1.0)
    assert torch.equal(got, note_match_list(sm_batch, tables, thr, on, 0.5, lengths, off, 0.5)) and int(got[:, 1].sum()) > 0


def test_smooth_frame_logits(mta):
    x = _random_case()["dev"]
    lengths = [1100, 1025, 640]
    act = _activity(x, 0.3)
    y = mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, lengths)
    assert y is not x and y.shape == x.shape and np.array_equal(y.cpu().numpy(), FR.smooth_ref(x.cpu().numpy(), 0.3, 1.0, 0.5, lengths, act))
    y = mta.smooth_frame_logits(x, 0.3, 1.0, 0.5, chunks=True)
    assert np.array_equal(_cat(y).cpu().numpy(), _expect(_cat(x), 0.3, 1.0, 0.5))
    y = mta.smooth_frame_logits(x[0], 0.3, 1.0, 0.5)                              # (P, T)
    assert y.shape == x[0].shape and np.array_equal(y.cpu().numpy(), FR.smooth_ref(x[:1].cpu().numpy(), 0.3, 1.0, 0.5, None, act[:1])[0])
    assert mta.smooth_frame_logits(x) is x
    assert np.array_equal(x.cpu().numpy(), _random_case()["x"])                  # the input is never written


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_c_abi_refusals_leave_the_output_alone(mta):
    from music_transcription_amd import _lib
    lib, ptr, stream = _raw()
    x = _random_case()["dev"]
    nan = float("nan")
    bad = [(0.5, -0.5, 0.0), (0.5, 0.0, -1e-3), (0.5, 64.5, 0.0), (0.5, 0.0, 1e9), (0.5, nan, 0.0), (0.5, 0.0, nan), (0.0, 1.0, 1.0), (1.0, 1.0, 1.0),
           (-0.1, 1.0, 1.0), (nan, 1.0, 1.0)]
    for thr, on, off in bad:
        rc, got = raw_smooth(x, thr, on, off, [5, 5, 5])
        assert rc == EINVAL and (got == SENTINEL).all(), (thr, on, off)
        rc, got = raw_smooth_chunks(x, thr, on, off)
        assert rc == EINVAL and (got == SENTINEL).all(), (thr, on, off)
    assert "penalty" in _lib.last_error() or "threshold" in _lib.last_error()
    out = torch.full_like(x, SENTINEL)
    for xp, op in ((None, ptr(out)), (ptr(x), None)):
        assert lib.mt_frame_smooth(xp, op, 0.5, 1.0, 1.0, None, B, P, T, stream()) == EINVAL
        assert lib.mt_frame_smooth_chunks(xp, op, 0.5, 1.0, 1.0, B, P, T, stream()) == EINVAL
    for dims in ((0, P, T), (B, 0, T), (B, P, 0), (B, -1, T)):
        assert lib.mt_frame_smooth(ptr(x), ptr(out), 0.5, 1.0, 1.0, None, *dims, stream()) == EINVAL
        assert lib.mt_frame_smooth_chunks(ptr(x), ptr(out), 0.5, 1.0, 1.0, *dims, stream()) == EINVAL
    both = torch.full((2 * x.numel(),), SENTINEL, device="cuda")                  # out overlaps the input without being it
    assert lib.mt_frame_smooth(both.data_ptr(), both.data_ptr() + 4 * T, 0.5, 1.0, 1.0, None, B, P, T, stream()) == EINVAL
    assert lib.mt_frame_smooth_chunks(both.data_ptr() + 4, both.data_ptr(), 0.5, 1.0, 1.0, B, P, T, stream()) == EINVAL
    assert "overlap" in _lib.last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (both == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ end to end
NM, H, NL = 32, 16, 2
TICK = lambda t: int(round(t * 220 * 120.0 / 60.0))                               # transcribe.write_midi's ticks


def _main(wav, ckpt, mid, thr, *more):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), wav, ckpt, "-o", mid, "-d", "cuda", "-t", str(thr), "--decoder", "frame",
                        "--n-mels", str(NM), "--hidden-size", str(H), "--num-layers", str(NL), *more], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return _midi_notes(mid)


def test_main_writes_the_smoothed_notes(mta, tmp_path):
    from scipy.io import wavfile
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    from music_transcription_amd.windows import transcribe_windows
    wav, ckpt, mid = str(tmp_path / "a.wav"), str(tmp_path / "m.pth"), str(tmp_path / "a.mid")
    rng = np.random.default_rng(4)
    wavfile.write(wav, 16000, (0.2 * rng.standard_normal(16000 * 40)).clip(-1, 1).astype(np.float32))
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, NL, 9), ckpt)
    model = mta.TranscriptionModel(model_type="cnn_rnn_large", n_mels=NM, hidden_size=H, num_layers=NL, dropout=0.0, device="cuda")
    model.load_state_dict(R.make_state_dict("cnn_rnn_large", NM, H, NL, 9), strict=True)
    model.eval()
    y = tr.load_audio_device(wav, 16000, "cuda")
    chunks, _ = tr.split_into_chunks_device(y)
    with torch.no_grad():
        mel, cmax = get_frontend(16000, NM, 512, "cuda")(chunks, clamp=False)
        logits = model.model(mel, chunk_max_power=cmax)
    stitched = transcribe_windows(model, [y], 2.0)[0][None]
    thr = _mid_threshold(logits)
    ticks = lambda notes: sorted((p, TICK(s), TICK(e)) for p, s, e in notes)
    flags = ["--smooth-on", "1", "--smooth-off", "1"]
    for lg, more in ((logits, []), (stitched, ["--overlap", "2"])):
        lg = lg.contiguous().float()
        by_ref = _uncat(torch.from_numpy(_expect(_cat(lg), thr, 1.0, 1.0)).cuda(), lg.shape[0])
        want = tr.notes_from_logits_device(lg, thr, smooth_on=1.0, smooth_off=1.0)                   # the Python path,
        assert want == tr.notes_from_logits_device(by_ref, thr)                                      # which decodes the specification's path
        plain = tr.notes_from_logits_device(lg, thr)
        assert want != plain
        assert _main(wav, ckpt, mid, thr, *more, *flags) == ticks(want)
    assert _main(wav, ckpt, mid, thr, "--overlap", "2") == ticks(plain)                              # and without the flags, today's file
    tr.write_midi(plain, str(tmp_path / "plain.mid"))
    assert open(mid, "rb").read() == open(str(tmp_path / "plain.mid"), "rb").read()
