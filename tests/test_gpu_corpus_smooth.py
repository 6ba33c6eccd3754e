"""Frame smoothing in corpus transcription (corpus.transcribe_shard / transcribe_shard_windows with smooth_on / smooth_off,
scripts/transcribe_corpus.py --smooth-on / --smooth-off): the notes and note scores are those of the decoders in notes.py given the
same penalties on the same logits, and those of the specification (frame_smooth_ref.smooth_ref on the logits copied to the host, then
the CPU decoders of note_clean_ref); the framewise F1 stays the raw threshold's; (0, 0) is today's call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frame_smooth_ref as FR
import note_clean_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
SR, HOP = 16000, 512
FS = SR / HOP
SECONDS = (40.0, 0.5, 61.0)                         # 2, 1, 3 chunks; 2, 1, 3 windows: groups [0, 1], [2]
NM, H, NL = 32, 16, 2
SMOOTH = dict(smooth_on=1.5, smooth_off=1.5)
CLEANUPS = ((1, 0), (3, 2))
KW = dict(overlap_s=2.0, batch=4, streams=2, group_windows=3, warm=False)


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _audio(seconds, seed):
    """tests/test_gpu_corpus_windows.py's synthetic audio: noise plus decaying tones."""
    n = int(seconds * SR)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = 0.05 * rng.standard_normal(n)
    for k, f in enumerate((110.0, 440.0 * (seed + 1), 1760.0, 3520.0)):
        y += 0.2 * np.sin(2 * np.pi * f * t + k) * np.exp(-0.7 * (t % (1.3 + 0.4 * k)))
    return torch.from_numpy(y.astype(np.float32)).cuda()


def _mid_threshold(logits):
    return float(np.clip(torch.sigmoid(logits.float().median()).item(), 0.05, 0.95))


def _reference_roll(i, frames):
    """Seeded random rolls: recording 0's is shorter than the recording, recording 1's longer."""
    n = {0: frames - 100, 1: frames + 9}.get(i, frames)
    g = torch.Generator(device="cuda").manual_seed(100 + i)
    return (torch.rand(88, n, device="cuda", generator=g) < 0.05).float()


def _activity(x, thr):
    from music_transcription_amd import ops
    return ops.predict_from_logits(x.contiguous().float(), thr).cpu().numpy() > 0


def _seconds(notes):
    return [(21 + p, float(s) / FS, float(e) / FS) for p, s, e in notes]


@pytest.fixture(scope="module")
def case(mta):
    """The model, the recordings, thresholds near the median activation, and per decoder the logits both corpus paths decode: the
    stitched ones of transcribe_windows per group (padded to the group's longest, zero-filled, as the shard holds them) and the
    chunk logits of one slab of all six chunks.  Computed once; nobody writes to them."""
    from oracle import model_ref as R
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=NM, hidden_size=H, num_layers=NL, dropout=0.0, device="cuda")
    model.load_state_dict(R.make_state_dict("cnn_rnn_large", NM, H, NL, 5), strict=True)
    model.eval()
    ys = [_audio(s, 10 + k) for k, s in enumerate(SECONDS)]
    groups = [[0, 1], [2]]
    stitched = {"frame": {}, "onset": {}}               # (each decoder's own forward: with and without the other heads)
    for decoder, group in ((d, g) for d in stitched for g in groups):
        got = mta.transcribe_windows(model, [ys[i] for i in group], 2.0, batch=4, all_heads=decoder == "onset")
        got = [g if decoder == "onset" else (g, None) for g in got]
        Tg = [int(g[0].shape[1]) for g in got]
        pad = [torch.zeros(len(group), 88, max(Tg), device="cuda") for _ in range(2)]
        for r, g in enumerate(got):
            pad[0][r, :, :Tg[r]] = g[0]
            if g[1] is not None:
                pad[1][r, :, :Tg[r]] = g[1]
        stitched[decoder][tuple(group)] = (pad[0], pad[1], Tg)
    chunks = [tr.split_into_chunks_device(y)[0] for y in ys]
    assert [int(c.shape[0]) for c in chunks] == [2, 1, 3]
    with torch.no_grad():
        mel, cmax = get_frontend(SR, NM, HOP, "cuda")(torch.cat(chunks), clamp=False)
        heads = model.model(mel, chunk_max_power=cmax, return_all_heads=True)
        alone = model.model(mel, chunk_max_power=cmax)
    frame = {"frame": alone.float().contiguous(), "onset": heads["frame"].float().contiguous()}
    onset = heads["onset"].float().contiguous()
    thr, othr = _mid_threshold(stitched["onset"][(2,)][0]), _mid_threshold(stitched["onset"][(2,)][1])
    return dict(model=model, ys=ys, groups=groups, stitched=stitched, chunks=chunks, frame=frame, onset=onset, thr=thr, othr=othr)


def _shard_windows(case, decoder, clean, **more):
    from music_transcription_amd import corpus
    kw = dict(KW, n_mels=NM, device="cuda", threshold=case["thr"], decoder=decoder, onset_threshold=case["othr"],
              reference_roll_of=_reference_roll, note_metrics=True, min_note_frames=clean[0], bridge_frames=clean[1], **more)
    return corpus.transcribe_shard_windows(case["model"], [0, 1, 2], lambda i: case["ys"][i], **kw)


@pytest.mark.parametrize("clean", CLEANUPS)
@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_windows_path_smooths_before_the_decoder_and_the_matcher(mta, case, decoder, clean):
    from music_transcription_amd import ops
    from music_transcription_amd.notes import note_match_counts, note_prf, notes_batch_device
    thr, othr = case["thr"], case["othr"]
    ckw = dict(min_note_frames=clean[0], bridge_frames=clean[1])
    res = _shard_windows(case, decoder, clean, **SMOOTH)
    plain = _shard_windows(case, decoder, clean)
    assert res["groups"] == case["groups"] and res["finite"] is True
    differ = 0
    for group in case["groups"]:
        frame, onset, Tg = case["stitched"][decoder][tuple(group)]
        onset = onset if decoder == "onset" else None
        want = notes_batch_device(frame, onset, thr, othr, Tg, FS, **ckw, **SMOOTH)
        refs = [_reference_roll(i, t) for i, t in zip(group, Tg)]
        cmp = [min(t, int(r.shape[1])) for t, r in zip(Tg, refs)]
        roll = torch.zeros_like(frame)
        for r, ref in enumerate(refs):
            roll[r, :, :cmp[r]] = ref[:, :cmp[r]]
        counts = note_match_counts(frame, roll, thr, onset, othr, cmp, **ckw, **SMOOTH)
        prf = note_prf(counts)
        raw_f1 = ops.f1_from_counts(ops.f1_counts(ops.predict_from_logits(frame, thr), roll, torch.tensor(cmp, device="cuda")))
        # the specification: the path of smooth_ref as the frame activity of the CPU decoders
        act = _activity(frame, thr)
        o_act = None if onset is None else _activity(onset, othr)
        path = FR.smooth_ref(frame.cpu().numpy(), thr, 1.5, 1.5, Tg, act) > 0
        spec_notes = CR.batch_notes_active(path, o_act, Tg, *clean)
        path_cmp = FR.smooth_ref(frame.cpu().numpy(), thr, 1.5, 1.5, cmp, act) > 0        # the matcher smooths over the frames it compares
        spec_counts = CR.match_counts_active(path_cmp, roll.cpu().numpy(), o_act, None, cmp, *clean)
        assert np.array_equal(counts.cpu().numpy(), spec_counts) and int(spec_counts[:, 1].sum()) > 0
        for r, i in enumerate(group):
            assert res["notes"][i] == want[r] == _seconds(spec_notes[r]), (group, i)
            assert res["note_f1"][i] == (prf[r]["onset"][2], prf[r]["onset_offset"][2])
            assert res["f1"][i] == plain["f1"][i] == float(raw_f1[r])                     # the framewise F1 is the raw threshold's
            differ += res["notes"][i] != plain["notes"][i]
    assert differ >= 1 and res["n_notes"] == sum(len(v) for v in res["notes"].values()) > 0
    zero = _shard_windows(case, decoder, clean, smooth_on=0.0, smooth_off=0.0)           # (0, 0) is the call without the arguments
    for key in ("notes", "f1", "note_f1", "n_notes", "groups", "frames", "windows"):
        assert zero[key] == plain[key], key


@pytest.mark.parametrize("decoder", ["frame", "onset"])
def test_chunk_path_smooths_the_recording_as_a_whole(mta, case, decoder):
    from music_transcription_amd import corpus
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.notes import heads_to_notes_device, note_match_counts, note_prf
    thr, othr = case["thr"], case["othr"]
    heads = decoder == "onset"
    refs = {i: _reference_roll(i, int(c.shape[0]) * 938) for i, c in enumerate(case["chunks"])}
    kw = dict(n_mels=NM, device="cuda", batch=8, streams=2, threshold=thr, decoder=decoder, onset_threshold=othr, warm=False,
              reference_roll_of=lambda i, n: refs[i], note_metrics=True)               # batch 8: one slab of all six chunks, as `case` ran them
    differ, a = 0, 0
    for clean in CLEANUPS:
        ckw = dict(min_note_frames=clean[0], bridge_frames=clean[1])
        res = corpus.transcribe_shard(case["model"], [0, 1, 2], lambda i: case["chunks"][i], **kw, **ckw, **SMOOTH)
        plain = corpus.transcribe_shard(case["model"], [0, 1, 2], lambda i: case["chunks"][i], **kw, **ckw)
        zero = corpus.transcribe_shard(case["model"], [0, 1, 2], lambda i: case["chunks"][i], **kw, **ckw, smooth_on=0, smooth_off=0.0)
        assert res["slabs"] == 1 and res["finite"] is True
        a = 0
        for i, c in enumerate(case["chunks"]):
            n = int(c.shape[0])
            lg = case["frame"][decoder][a:a + n].contiguous()
            on = case["onset"][a:a + n].contiguous() if heads else None
            a += n
            want = (heads_to_notes_device(lg, on, thr, othr, FS, **ckw, **SMOOTH) if heads else
                    tr.notes_from_logits_device(lg, thr, FS, **ckw, **SMOOTH))
            cat = lambda x: x.permute(1, 0, 2).reshape(1, 88, -1).contiguous()
            act = _activity(cat(lg), thr)
            o_act = _activity(cat(on), othr) if heads else None
            path = FR.smooth_ref(cat(lg).cpu().numpy(), thr, 1.5, 1.5, None, act) > 0
            spec = CR.heads_notes_active(path, o_act, None, *clean)
            assert res["notes"][i] == want == _seconds(spec), (clean, i)
            L = min(int(refs[i].shape[1]), n * 938)
            rows = lambda x: cat(x)[0, :, :L].contiguous()
            counts = note_match_counts(rows(lg), refs[i][:, :L].contiguous(), thr, rows(on) if heads else None, othr, **ckw, **SMOOTH)
            m = note_prf(counts)[0]
            assert res["note_f1"][i] == (m["onset"][2], m["onset_offset"][2])
            path_L = FR.smooth_ref(cat(lg)[:, :, :L].cpu().numpy(), thr, 1.5, 1.5, None, act[:, :, :L]) > 0
            spec_counts = CR.match_counts_active(path_L, refs[i][None, :, :L].cpu().numpy(), None if o_act is None else o_act[:, :, :L], None, None, *clean)
            assert np.array_equal(counts.cpu().numpy().reshape(1, 4), spec_counts)
            assert res["f1"][i] == plain["f1"][i]
            differ += res["notes"][i] != plain["notes"][i]
        for key in ("notes", "f1", "note_f1", "n_notes", "chunks", "slabs"):
            assert zero[key] == plain[key], key
    assert differ >= 1


def test_cli_writes_the_smoothed_midi_files(mta, case, tmp_path):
    from oracle import model_ref as R
    from music_transcription_amd import corpus
    from music_transcription_amd import transcribe as tr
    from music_transcription_amd.frontend import get_frontend
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", NM, H, NL, 5), ckpt)
    chunks = corpus.synth_recording(0, 0.01 * 3600.0, "cuda", 0)                        # --synthetic 1 --hours 0.01: one recording of 36 s
    with torch.no_grad():
        mel, cmax = get_frontend(SR, NM, HOP, "cuda")(chunks, clamp=False)
        lg = case["model"].model(mel, chunk_max_power=cmax).float().contiguous()
    thr = _mid_threshold(lg)
    want, plain = tr.notes_from_logits_device(lg, thr, **SMOOTH), tr.notes_from_logits_device(lg, thr)
    assert want != plain
    base = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "scripts", "transcribe_corpus.py"), "--synthetic", "1", "--hours",
            "0.01", "--model", ckpt, "--model-type", "cnn_rnn_large", "--n-mels", str(NM), "--hidden-size", str(H), "--num-layers", str(NL),
            "--batch", "4", "--threshold", repr(thr)]
    mids = {}
    for name, more in (("smooth", ["--smooth-on", "1.5", "--smooth-off", "1.5"]), ("plain", [])):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["--out-dir", out] + more, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        assert os.listdir(out) == ["synthetic_000.mid"]
        mids[name] = open(os.path.join(out, "synthetic_000.mid"), "rb").read()
    for name, notes in (("smooth", want), ("plain", plain)):
        tr.write_midi(notes, str(tmp_path / (name + ".mid")))
        assert mids[name] == open(str(tmp_path / (name + ".mid")), "rb").read(), name
    assert mids["smooth"] != mids["plain"]
