"""Peak-picked onsets in the decoders on the GPU (csrc/note_decode.h peak_mask, the mt_*_peak entry points, notes.py; DESIGN.md 6c
"Peak-picked onsets") against the plain loops of peak_decode_ref.py, with scipy's maximum matching for the counts.  Logits are
multiples of 1/4, so neighbours tie all the time and every comparison is exact: random rows plus planted rows on the window (64),
slab (512 for notes.hip, 1024 for notes_batch.hip), chunk and length boundaries, ragged lengths with NaN in the padding.  Then: edge
mode calls what it called before, the merged triangle pairs of the CPU test on the device, and one run of scripts/evaluate.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_metrics_ref as NR  # noqa: E402
import offset_decode_ref as OD  # noqa: E402
import peak_decode_ref as PR  # noqa: E402
from test_gpu_note_list import _random_list  # noqa: E402
from test_rawdata_cpu import note, smf  # noqa: E402

pytestmark = pytest.mark.gpu

P, B = 88, 2
REACHES = [1, 2, 8]
CLEANUPS = [(1, 0), (3, 2)]
# T -> the lengths the case runs with (None = all T).  Every set is ragged and together they hold 0, 1, T and lengths off the window grid.
NOTES_LENGTHS = {130: ([1, 129], None), 600: ([0, 577], [600, 513])}
BATCH_T, BATCH_LENGTHS = 1100, ([1100, 1], [0, 1057])
CHUNKS, CHUNK_T = 3, 70


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _quarter(rng, shape, mean, scale):
    return (np.rint(4.0 * (mean + scale * rng.standard_normal(shape))) / 4.0).astype(np.float32)


def _plant(xo, n, lengths):
    """Planted onset rows of one sample (n = its frames, a sample of the batch or the chunks concatenated; lengths = the valid frames it
    is run with): quiet rows with
      row 0: peaks on 0, 63, 511, 1023 and on L - 1 of every length; row 1: peaks on 64, 512, 1024;
      row 2: a plateau over 62 .. 66, across the window edge; row 3: one over 510 .. 514 / 1022 .. 1026, across the slab edges;
      rows 4 + 2 i, 5 + 2 i for R = REACHES[i]: a higher value exactly R frames past a window / slab edge (63, 511, 1023 are then
      no peaks at reach R and peaks below it), and one exactly R frames before the edge frames 64, 512, 1024 (the low-side carry)."""
    rows = xo[:4 + 2 * len(REACHES)]
    rows[...] = -6.0
    for t in (0, 63, 511, 1023) + tuple(L - 1 for L in lengths if L > 0):
        if t < n:
            rows[0, t] = 3.0
    for t in (64, 512, 1024):
        if t < n:
            rows[1, t] = 3.0
    if n > 66:
        rows[2, 62:67] = 2.5
    for t in (512, 1024):
        if t + 2 < n:
            rows[3, t - 2:t + 3] = 2.5
    for i, R in enumerate(REACHES):
        for t in (63, 511, 1023):
            if t + R < n:
                rows[4 + 2 * i, t], rows[4 + 2 * i, t + R] = 2.0, 3.0
        for t in (64, 512, 1024):
            if t < n:
                rows[5 + 2 * i, t], rows[5 + 2 * i, t - R] = 2.0, 3.0


_CASES = {}


def _case(kind, T):
    """The logits of one shape as host arrays, built once and never written again (NaN past each set of lengths is added per run, on
    the copy that goes to the device)."""
    key = (kind, T)
    if key not in _CASES:
        rng = np.random.default_rng(1000 + T)
        nb = CHUNKS if kind == "chunks" else B
        xf, xo, xk = _quarter(rng, (nb, P, T), -0.5, 2.0), _quarter(rng, (nb, P, T), -0.75, 1.5), _quarter(rng, (nb, P, T), -2.0, 1.5)
        sets = {"notes": NOTES_LENGTHS.get(T, ()), "batch": BATCH_LENGTHS, "chunks": ()}[kind]
        if kind == "chunks":
            cat = np.ascontiguousarray(xo.transpose(1, 0, 2)).reshape(P, nb * T)          # the rows as the kernel walks them
            _plant(cat, nb * T, [nb * T])
            cat[10:12] = -6.0
            cat[10, [T - 1, 2 * T]] = 3.0                                                  # peaks on a chunk's last and first frame
            cat[11, T - 2:T + 2], cat[11, 2 * T - 1], cat[11, 2 * T] = 2.5, 2.0, 3.0       # a plateau and a rising step across chunk boundaries
            xo = np.ascontiguousarray(cat.reshape(P, nb, T).transpose(1, 0, 2))
        else:
            for b in range(nb):
                _plant(xo[b], T, [T] + [ls[b] for ls in sets if ls])
        ref = OD.markov(rng, (nb, P, T), 0.1, 0.2)
        f, o = NR.sigmoid_active(xf, 0.5), NR.sigmoid_active(xo, 0.5)
        lst = _random_list(rng, f, o, T) if kind == "notes" else None
        for a in (xf, xo, xk, ref):
            a.setflags(write=False)
        _CASES[key] = dict(xf=xf, xo=xo, xk=xk, ref=ref, list=lst)
    return _CASES[key]


def _device(c, lengths):
    """The case on the device with NaN in every head and in the roll at and past each sample's length."""
    out = {}
    for k in ("xf", "xo", "xk", "ref"):
        a = c[k].astype(np.float32).copy()
        if lengths is not None:
            for b, L in enumerate(lengths):
                a[b, :, L:] = np.nan
        out[k] = torch.from_numpy(a).cuda()
    if c["list"] is not None:
        on, off, ptr = c["list"]
        out["list"] = {"on": torch.from_numpy(np.asarray(on, np.int32)).cuda(), "off": torch.from_numpy(np.asarray(off, np.int32)).cuda(),
                       "ptr": torch.from_numpy(np.asarray(ptr, np.int64)).cuda()}
    return out


def _lib():
    from music_transcription_amd import _lib
    return _lib.lib, _lib.ptr, _lib.stream_ptr


def _ln(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")


def _twice(run):
    """Every entry point runs twice on the same inputs and has to give the same answer."""
    a, b = run(), run()
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    return a


# ------------------------------------------------------------------------------------------------ exact equality with the reference
@pytest.mark.parametrize("M,G", CLEANUPS)
@pytest.mark.parametrize("off", [False, True])
@pytest.mark.parametrize("R", REACHES)
@pytest.mark.parametrize("T", sorted(NOTES_LENGTHS))
def test_match_counts_and_list_equal_the_reference(mta, T, R, off, M, G):
    lib, ptr, stream = _lib()
    c = _case("notes", T)
    for lengths in NOTES_LENGTHS[T]:
        d, ln = _device(c, lengths), _ln(lengths)
        xk, dk = (c["xk"], d["xk"]) if off else (None, None)

        def counts_of(call):
            out = torch.full((B, 4), -7, dtype=torch.int64, device="cuda")
            assert call(out) == 0
            torch.cuda.synchronize()
            return (out.cpu().numpy(),)

        got, = _twice(lambda: counts_of(lambda out: lib.mt_note_match_counts_peak(
            ptr(d["xf"]), ptr(d["xo"]), ptr(dk), 0.5, 0.5, 0.5, ptr(d["ref"]), ptr(ln), ptr(out), B, P, T, M, G, R, stream())))
        want = PR.match_counts(c["xf"], c["xo"], xk, c["ref"], lengths, R, M, G)
        assert np.array_equal(got, want), (lengths, got, want)
        n = d["list"]
        got, = _twice(lambda: counts_of(lambda out: lib.mt_note_match_list_peak(
            ptr(d["xf"]), ptr(d["xo"]), ptr(dk), 0.5, 0.5, 0.5, ptr(n["on"]), ptr(n["off"]), ptr(n["ptr"]), ptr(ln), ptr(out), B, P, T,
            M, G, R, stream())))
        want = PR.match_list_counts(c["xf"], c["xo"], xk, *c["list"], lengths, R, M, G)
        assert np.array_equal(got, want), (lengths, got, want)


@pytest.mark.parametrize("M,G", CLEANUPS)
@pytest.mark.parametrize("off", [False, True])
@pytest.mark.parametrize("R", REACHES)
def test_heads_to_notes_across_chunk_boundaries_equals_the_reference(mta, R, off, M, G):
    lib, ptr, stream = _lib()
    c = _case("chunks", CHUNK_T)
    d = _device(c, None)
    xk, dk = (c["xk"], d["xk"]) if off else (None, None)
    cap = 1 << 15

    def run():
        counts = torch.full((P,), -7, dtype=torch.int32, device="cuda")
        se = torch.full((2, cap), -7, dtype=torch.int32, device="cuda")
        assert lib.mt_heads_to_notes_peak(ptr(d["xf"]), ptr(d["xo"]), ptr(dk), 0.5, 0.5, 0.5, CHUNKS, P, CHUNK_T, ptr(counts), ptr(se[0]), ptr(se[1]),
                                          cap, M, G, R, stream()) == 0
        torch.cuda.synchronize()
        return counts.cpu().numpy(), se.cpu().numpy()

    cnt, se = _twice(run)
    n = int(cnt.sum())
    assert (se[:, n:] == -7).all()
    got = [(int(p), int(s), int(e)) for p, s, e in zip(np.repeat(np.arange(P), cnt), se[0, :n], se[1, :n])]
    want = PR.heads_notes(c["xf"], c["xo"], xk, R, M, G)
    assert got == want
    if (M, G) == (1, 0):                                              # the planted rows across chunk boundaries, spelled out
        starts = lambda q: [s for p, s, _ in want if p == q]
        assert starts(10) == [CHUNK_T - 1, 2 * CHUNK_T]               # peaks on a chunk's last and on a chunk's first frame
        assert starts(11) == [CHUNK_T - 2, 2 * CHUNK_T]               # the plateau's first frame; the step's upper frame


@pytest.mark.parametrize("M,G", CLEANUPS)
@pytest.mark.parametrize("R", REACHES)
def test_notes_batch_equals_the_reference(mta, R, M, G):
    lib, ptr, stream = _lib()
    T = BATCH_T
    c = _case("batch", T)
    cap = 1 << 17
    for lengths in BATCH_LENGTHS:
        d, ln = _device(c, lengths), _ln(lengths)

        def run():
            counts = torch.full((B * P,), -7, dtype=torch.int32, device="cuda")
            row_off = torch.full((B * P + 1,), -7, dtype=torch.int64, device="cuda")
            se = torch.full((2, cap), -7, dtype=torch.int32, device="cuda")
            assert lib.mt_notes_batch_peak(ptr(d["xf"]), ptr(d["xo"]), 0.5, 0.5, ptr(ln), B, P, T, ptr(counts), ptr(row_off), ptr(se[0]),
                                           ptr(se[1]), cap, M, G, R, stream()) == 0
            torch.cuda.synchronize()
            return counts.cpu().numpy(), row_off.cpu().numpy(), se.cpu().numpy()

        cnt, ro, se = _twice(run)
        assert ro[0] == 0 and (np.diff(ro) == cnt).all() and ro[-1] <= cap and (se[:, ro[-1]:] == -7).all()
        got = [[(p, int(se[0, i]), int(se[1, i])) for p in range(P) for i in range(ro[b * P + p], ro[b * P + p + 1])] for b in range(B)]
        want = PR.batch_notes(c["xf"], c["xo"], lengths, R, M, G)
        assert got == want, lengths
        if lengths[0] == T and (M, G) == (1, 0):                     # the planted rows, spelled out
            starts = lambda p: [s for q, s, _ in want[0] if q == p]
            assert starts(0) == [0, 63, 511, 1023, T - 1] and starts(1) == [64, 512, 1024]
            assert starts(2) == [62] and starts(3) == [510, 1022]
            i = REACHES.index(R)
            assert starts(4 + 2 * i) == [63 + R, 511 + R, 1023 + R] and starts(5 + 2 * i) == [64 - R, 512 - R, 1024 - R]
            for j, Q in enumerate(REACHES):                          # a smaller reach sees both frames as peaks
                if Q > R:
                    assert starts(4 + 2 * j) == sorted([63, 511, 1023] + [63 + Q, 511 + Q, 1023 + Q])


# ------------------------------------------------------------------------------------------------ edge mode is untouched
def test_edge_mode_is_what_the_call_without_the_argument_gives(mta):
    from music_transcription_amd import notes as N
    c = _case("notes", 600)
    lengths = [600, 513]
    d = _device(c, lengths)
    h = _device(_case("chunks", CHUNK_T), None)
    for off, clean in ((False, {}), (True, {}), (False, {"min_note_frames": 3, "bridge_frames": 2})):
        for fn, ref in ((N.note_match_counts, d["ref"]), (N.note_match_list, d["list"])):
            kw = dict(clean, offset_logits=d["xk"] if off else None)
            a = fn(d["xf"], ref, 0.5, d["xo"], 0.5, lengths, **kw)
            b = fn(d["xf"], ref, 0.5, d["xo"], 0.5, lengths, onset_detect="edge", peak_reach=5, **kw)
            assert torch.equal(a, b)
        kw = dict(clean, offset_logits=h["xk"] if off else None)
        assert N.heads_to_notes_device(h["xf"], h["xo"], **kw) == N.heads_to_notes_device(h["xf"], h["xo"], onset_detect="edge", **kw)
    for kw in ({}, {"min_note_frames": 3, "bridge_frames": 2}, {"refine_onsets": True}):
        assert N.notes_batch_device(d["xf"], d["xo"], lengths=lengths, **kw) == \
            N.notes_batch_device(d["xf"], d["xo"], lengths=lengths, onset_detect="edge", **kw)
    # and peak mode through the same Python calls is the reference's
    got = N.note_match_counts(d["xf"], d["ref"], 0.5, d["xo"], 0.5, lengths, onset_detect="peak", peak_reach=2).cpu().numpy()
    assert np.array_equal(got, PR.match_counts(c["xf"], c["xo"], None, c["ref"], lengths, 2))
    got = N.note_match_list(d["xf"], d["list"], 0.5, d["xo"], 0.5, lengths, offset_logits=d["xk"], onset_detect="peak").cpu().numpy()
    assert np.array_equal(got, PR.match_list_counts(c["xf"], c["xo"], c["xk"], *c["list"], lengths, 1))


# ------------------------------------------------------------------------------------------------ the merge case on the device
def test_triangle_pairs_merge_under_edge_and_split_under_peak(mta):
    from music_transcription_amd import notes as N
    pairs = PR.triangle_pairs()
    T = 48
    xo = np.full((1, P, T), -30.0, np.float32)
    dips = []
    for p, (J, on, gap) in enumerate(pairs):
        y, xo[0, p] = PR.triangle_row(J, on, gap, T)
        dips.append(float(y[int(round(on / 320)):int(round((on + gap) / 320)) + 1].min()))
    xf = torch.full((1, P, T), -30.0, device="cuda")
    on_dev = torch.from_numpy(xo).cuda()
    edge = N.notes_batch_device(xf, on_dev, onset_detect="edge")[0]
    peak = N.notes_batch_device(xf, on_dev, onset_detect="peak")[0]
    ticks = [N.notes_batch_device(xf, on_dev, onset_detect="peak", refine_onsets=True, refine_reach=r)[0] for r in (0, 8)]
    assert ticks[0] == ticks[1]
    fs = 16000 / 512
    for p, ((J, on, gap), dip) in enumerate(zip(pairs, dips)):
        of = lambda notes: [n for n in notes if n[0] == 21 + p]
        assert len(of(edge)) == (1 if dip > 0.5 else 2), (J, gap, dip, of(edge))
        assert [int(round(s * fs)) for _, s, _ in of(peak)] == [int(round(on / 320)), int(round((on + gap) / 320))], (J, gap, of(peak))
        for (_, s, _), want in zip(of(ticks[0]), (on, on + gap)):
            assert abs(s * 1e4 - want) <= 320 + 1                     # the vertex frame's centre is within 160 ticks, the shift within half a frame
    assert sum(d > 0.5 for d in dips) >= 3 and len(peak) == 2 * len(pairs)


# ------------------------------------------------------------------------------------------------ one command line
def _small_tree(root, durs):
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "2004"), exist_ok=True)
    rng = np.random.default_rng(0)
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for i, (name, (d, split)) in enumerate(durs.items()):
        n = int(d * 16000)
        t = np.arange(n) / 16000.0
        sig = 0.3 * np.sin(2 * np.pi * 220.0 * (i + 1) * t) * np.exp(-0.5 * (t % 1.7)) + 0.02 * rng.standard_normal(n)
        wavfile.write(os.path.join(root, "2004", f"{name}.wav"), 16000, (sig * 32767).astype(np.int16))
        ev = []
        for k, s in enumerate(np.arange(0.3, d - 1.0, 0.37)):                       # 2000 MIDI ticks per second; onsets at every phase
            ev += note(0, 30 + (k * 7) % 50, int(s * 2000) + 3 * k, int((s + 0.3 + 0.1 * (k % 3)) * 2000))
        with open(os.path.join(root, "2004", f"{name}.midi"), "wb") as fh:
            fh.write(smf([[], ev]))
        rows.append(f"X,Y,{split},2004,2004/{name}.midi,2004/{name}.wav,{d}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")


def test_evaluate_script_with_peak_picked_onsets(mta, tmp_path, monkeypatch, capsys):
    """scripts/evaluate.py --onset_detect peak on logits built from the width-4 regression targets of a two-recording tree: its
    EVAL_NOTE_* lines are the means of the reference's counts (peak_decode_ref on the same logits against the MIDI note list)."""
    from oracle import model_ref as R
    from music_transcription_amd import evaluate as E
    tree = str(tmp_path / "maestro")
    _small_tree(tree, {"a": (12.0, "train"), "b": (9.5, "train")})
    nm, H, L, J = 64, 24, 3, 4
    ckpt = str(tmp_path / "m.pth")
    torch.save(R.make_state_dict("cnn_rnn_large", nm, H, L, 5), ckpt)
    spec = importlib.util.spec_from_file_location("evaluate_script", os.path.join(ROOT, "scripts", "evaluate.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    src = mta.MaestroDataset(tree, split="train", n_mels=nm, onset_labels="midi", onset_target="regress", onset_width=J)
    seen = {}

    def fake(model, dataset, indices, device="cuda", max_batch=128, all_heads=False, with_offset=False):
        out = []
        for i in indices:
            _, lab, _ = src.get_batch([i])
            on = torch.logit(lab["onset"][0], eps=1e-6)
            frame = (lab["frame"][0] * 20.0 - 10.0).contiguous()
            seen[i] = (frame.cpu().numpy(), on.cpu().numpy(), dataset.ref_notes([i]))
            item = (i, frame, lab["frame"][0].contiguous())
            out.append(item + (on,) if all_heads else item)
        return out
    monkeypatch.setattr(E, "collect_logits", fake)
    f1 = {}
    for detect in ("peak", "edge"):
        argv = ["evaluate.py", "--model", ckpt, "--data_source", "full", "--root_dir", tree, "--split", "train", "--model_type", "cnn_rnn_large",
                "--n_mels", str(nm), "--hidden_size", str(H), "--num_layers", str(L), "--dropout", "0.0", "--cache_dir", str(tmp_path / "none"),
                "--note_metrics", "--note_reference", "midi", "--decoder", "onset", "--headless", "--onset_detect", detect]
        monkeypatch.setattr(sys, "argv", argv)
        assert script.main() == 0
        out = capsys.readouterr().out.strip().splitlines()
        assert [l.split("=")[0] for l in out] == ["EVAL_MEAN_F1", "EVAL_NOTE_ONSET_F1", "EVAL_NOTE_ONSET_OFFSET_F1"], out
        f1[detect] = (float(out[1].split("=")[1]), float(out[2].split("=")[1]))
    want = {"onset": [], "onset_offset": []}
    for i in sorted(seen):
        xf, xo, notes = seen[i]
        r_on, r_off, r_ptr = (notes[k].cpu().numpy() for k in ("on", "off", "ptr"))
        n_ref, n_est, tp_on, tp_onoff = PR.match_list_counts(xf[None], xo[None], None, r_on, r_off, r_ptr, None, 1)[0]
        want["onset"].append(NR.prf(tp_on, n_ref, n_est)[2])
        want["onset_offset"].append(NR.prf(tp_onoff, n_ref, n_est)[2])
    print("note F1 (onset, onset+offset) peak:", f1["peak"], "edge:", f1["edge"], "reference:", np.mean(want["onset"]), np.mean(want["onset_offset"]))
    assert f1["peak"] == (float(f"{np.mean(want['onset']):.6f}"), float(f"{np.mean(want['onset_offset']):.6f}"))
    assert f1["peak"][0] == 1.0 and f1["edge"][0] < 1.0               # width 4: the edge stamp is up to two frames early, the peak is the vertex frame
