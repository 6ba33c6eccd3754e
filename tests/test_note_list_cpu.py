"""CPU tests of the MIDI note list: rawdata.label_notes against label_spans, the streaming matching rule of mt_note_match_list
(note_list_ref.stream_matching) against scipy's maximum bipartite matching, dict targets of the loop helpers, and the new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_list_ref as LR  # noqa: E402
import note_metrics_ref as NR  # noqa: E402
from test_rawdata_cpu import CASES, cc64, note, smf  # noqa: E402

FS = 16000 / 512


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _restrike_cases():
    # 120 bpm, 1000 ticks per beat: one MIDI tick = 0.5 ms = 5 ticks of 100 us; a frame is 64 MIDI ticks
    c = {}
    # pitch 60 struck at 0.1 s and again at 0.6 s while the pedal (0.05 s .. 2 s) holds the first; pitch 64 alone under the pedal
    c["pedalled_restrike"] = [[], note(0, 60, 200, 700) + note(0, 60, 1200, 1600) + note(0, 64, 400, 500)
                              + cc64(0, 100, 127) + cc64(0, 4000, 0) + note(0, 67, 5000, 5400)]
    # pitch 62: the note-off of the first note and the note-on of the second fall on the same tick (0.065 s, 0.645 s, 1.285 s)
    c["gapless_restrike"] = [[], note(0, 62, 130, 1290) + note(0, 62, 1290, 2570) + note(0, 65, 300, 900)]
    # two keys struck on two tracks at the same instant, the longer note once on the second track and once on the first
    c["duplicates"] = [[], note(0, 70, 1000, 1500) + note(0, 72, 64, 640), note(1, 70, 1000, 2500) + note(1, 72, 64, 320)]
    return c


NEW_CASES = _restrike_cases()
ALL_CASES = {**CASES, **NEW_CASES}


def _midi(name):
    from music_transcription_amd import midi as MD
    return MD.MidiFile(smf(ALL_CASES[name]))


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_label_notes_merge_to_label_spans(mta, name):
    from music_transcription_amd import rawdata as RD
    m = _midi(name)
    spans, poff, _, _ = RD.label_spans(m, FS)
    nt = RD.label_notes(m, FS)
    assert nt.pitch_off[0] == 0 and nt.pitch_off[-1] == len(nt.on_tick) == len(nt.off_tick) == len(nt.on_frame) == len(nt.end_frame)
    rows = np.repeat(np.arange(88), np.diff(nt.pitch_off))
    # (a) the un-cut, pedal-extended spans [on_frame, end_frame), merged per pitch, are label_spans' spans
    got, got_off = RD._merge_spans(nt.on_frame.astype(np.int64), nt.end_frame.astype(np.int64), rows.astype(np.int64))
    assert np.array_equal(got, spans) and np.array_equal(got_off, poff)
    # (c) per pitch: onsets strictly rising (duplicates collapsed), off > on, no note sounds past the next onset of its pitch
    assert np.all(nt.off_tick > nt.on_tick)
    for p in range(88):
        on, off = nt.on_tick[nt.pitch_off[p]:nt.pitch_off[p + 1]], nt.off_tick[nt.pitch_off[p]:nt.pitch_off[p + 1]]
        assert np.all(np.diff(on) > 0) and np.all(off[:-1] <= on[1:])
        f = nt.on_frame[nt.pitch_off[p]:nt.pitch_off[p + 1]]
        assert np.all(np.diff(f) >= 0)
    # every note-on lies in a span of its pitch: the onset roll can only mark cells the roll marks
    on_sp, on_po = RD.onset_spans(nt)
    for p in range(88):
        sp = spans[poff[p]:poff[p + 1]]
        for u, v in on_sp[on_po[p]:on_po[p + 1]]:
            assert v == u + 1 and np.any((sp[:, 0] <= u) & (u < sp[:, 1])), (name, p, u)
        assert np.all(np.diff(on_sp[on_po[p]:on_po[p + 1], 0]) > 0)


def _row(nt, midi_pitch):
    p = midi_pitch - 21
    sl = slice(nt.pitch_off[p], nt.pitch_off[p + 1])
    return list(zip(nt.on_tick[sl].tolist(), nt.off_tick[sl].tolist()))


def test_restrikes_are_two_notes_where_the_roll_has_one_run(mta):
    from music_transcription_amd import rawdata as RD
    m = _midi("pedalled_restrike")
    spans, poff, _, _ = RD.label_spans(m, FS)
    nt = RD.label_notes(m, FS)
    assert poff[60 - 21 + 1] - poff[60 - 21] == 1                       # one run: the pedal holds the first strike into the second
    # 0.1 s, 0.6 s; the first is cut at the second's onset, the second lasts to the pedal's release at 2 s
    assert _row(nt, 60) == [(1000, 6000), (6000, 20000)]
    assert _row(nt, 64) == [(2000, 20000)]                              # sustained to the release
    assert _row(nt, 67) == [(25000, 27000)]                             # after the pedal: its own end
    m = _midi("gapless_restrike")
    spans, poff, _, _ = RD.label_spans(m, FS)
    nt = RD.label_notes(m, FS)
    assert poff[62 - 21 + 1] - poff[62 - 21] == 1 and spans[poff[62 - 21]].tolist() == [2, 40]
    assert _row(nt, 62) == [(650, 6450), (6450, 12850)]
    assert nt.on_frame[nt.pitch_off[62 - 21]:nt.pitch_off[62 - 21 + 1]].tolist() == [2, 20]
    on_sp, on_po = RD.onset_spans(nt)
    assert on_sp[on_po[62 - 21]:on_po[62 - 21 + 1]].tolist() == [[2, 3], [20, 21]]


def test_duplicates_collapse_into_the_longest(mta):
    from music_transcription_amd import rawdata as RD
    nt = RD.label_notes(_midi("duplicates"), FS)
    assert _row(nt, 70) == [(5000, 12500)]                              # two tracks, same instant: the longer one
    assert _row(nt, 72) == [(320, 3200)]


def _notes_one_by_one(m):
    """label_notes' rule restated note by note: {pitch row: [(on_tick, off_tick)]}."""
    rows = {}
    for inst in m.instruments:
        if inst.is_drum or not inst.notes:
            continue
        t_end = inst.get_end_time()
        width = int(FS * t_end)
        pedal, down = [], None
        for number, value, t in inst.control_changes:
            if number == 64 and down is None and value >= 64:
                down = t
            elif number == 64 and down is not None and value < 64:
                pedal.append((down, min(t, t_end)))
                down = None
        for n in inst.notes:
            if not 21 <= n.pitch < 109 or not min(int(n.start * FS), width) < min(int(n.end * FS), width):
                continue
            end = n.end
            for a, b in pedal:
                if max(n.start, a) < min(n.end, b):                      # the note sounds inside the interval
                    end = max(end, b)
            d = rows.setdefault(n.pitch - 21, {})
            on = int(round(n.start * 1e4))
            d[on] = max(d.get(on, 0), int(round(end * 1e4)))             # equal onsets: the longest
    out = {}
    for p, d in rows.items():
        ons = sorted(d)
        out[p] = [(on, max(on + 1, min(d[on], ons[k + 1] if k + 1 < len(ons) else d[on]))) for k, on in enumerate(ons)]
    return out


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_label_notes_equal_the_rule_note_by_note(mta, name):
    from music_transcription_amd import rawdata as RD
    m = _midi(name)
    nt = RD.label_notes(m, FS)
    want = _notes_one_by_one(m)
    for p in range(88):
        assert _row(nt, p + 21) == want.get(p, []), (name, p)
    if name == "overlap_same_pitch":                                     # a later strike cuts the note that still sounds
        (a, b), (c, d) = _row(nt, 60)
        assert b == c


def test_ticks_meet_frames_in_integers():
    assert LR.TICKS_PER_FRAME * 16000 == 512 * 10000
    # criteria on the frame grid coincide with mt_note_match_counts': 320 <= 500 < 640
    for d in range(-3, 4):
        assert (abs(LR.TICKS_PER_FRAME * d) <= LR.ONSET_TOL) == (abs(d) <= 1)


def _random_runs(rng, T, p_on, p_off):
    out = np.zeros(T, bool)
    s = False
    for t in range(T):
        s = (rng.random() >= p_off) if s else (rng.random() < p_on)
        out[t] = s
    return out


def _random_notes(rng, T, est):
    """A sorted note list in ticks over T frames: uniform onsets, clusters closer than 50 ms, equal onsets, notes near estimates."""
    n = int(rng.integers(0, 12))
    end = LR.TICKS_PER_FRAME * T
    on = rng.integers(0, end, size=n).tolist()
    for _ in range(int(rng.integers(0, 4))):                             # a burst of re-strikes within 50 ms
        if on:
            c = on[int(rng.integers(0, len(on)))]
            on += (c + rng.integers(-400, 400, size=int(rng.integers(1, 4)))).tolist()
    for s, e in est:                                                     # references at and around estimated onsets
        if rng.random() < 0.6:
            on.append(LR.TICKS_PER_FRAME * s + int(rng.integers(-700, 700)))
        if on and rng.random() < 0.15:
            on.append(on[-1])                                            # equal onsets
    on = np.sort(np.clip(np.array(on, np.int64), 0, end - 1)) if on else np.zeros(0, np.int64)
    length = np.where(rng.random(on.size) < 0.5, rng.integers(1, 1500, size=on.size), rng.integers(1, 12000, size=on.size))
    for k, (s, e) in enumerate(est):                                     # some offsets near estimated offsets
        if on.size and rng.random() < 0.5:
            i = int(np.argmin(np.abs(on - LR.TICKS_PER_FRAME * s)))
            length[i] = max(1, LR.TICKS_PER_FRAME * e - on[i] + int(rng.integers(-900, 900)))
    return on, on + length


def test_streaming_rule_is_a_maximum_matching():
    rng = np.random.default_rng(0)
    rows = nonzero = two_compatible = touching = close = 0
    for k in range(3000):
        T = int(rng.integers(3, 90))
        f = _random_runs(rng, T, rng.uniform(0.05, 0.6), rng.uniform(0.1, 0.9))
        o = _random_runs(rng, T, rng.uniform(0.05, 0.5), 0.7)
        for est in (NR.frame_notes(f), NR.onset_notes(f, o)):            # both decoders
            on, off = _random_notes(rng, T, est)
            got = LR.stream_matching(on, off, est)
            want = (LR.max_matching_ticks(on, off, est, False), LR.max_matching_ticks(on, off, est, True))
            assert got == want, (k, on.tolist(), off.tolist(), est)
            rows += 1
            nonzero += want[0] > 0
            if len(est) and on.size:
                two_compatible += bool((LR.compatible_ticks(on, off, est, False).sum(1) == 2).any())
            touching += any(a[1] == b[0] for a, b in zip(est, est[1:]))
            close += bool(on.size > 1 and (np.diff(on) < LR.ONSET_TOL).any())
    assert rows == 6000
    assert nonzero >= 0.3 * rows, nonzero                                # it cannot pass on empty graphs
    assert two_compatible >= 100 and touching >= 100 and close >= 1000, (two_compatible, touching, close)


def test_list_counts_on_the_frame_grid_equal_roll_counts():
    rng = np.random.default_rng(1)
    for _ in range(40):
        B, P, T = 2, 3, int(rng.integers(5, 150))
        ref = np.stack([[_random_runs(rng, T, 0.1, 0.3) for _ in range(P)] for _ in range(B)]).astype(np.float32)
        f = np.stack([[_random_runs(rng, T, 0.1, 0.3) for _ in range(P)] for _ in range(B)])
        o = np.stack([[_random_runs(rng, T, 0.1, 0.7) for _ in range(P)] for _ in range(B)])
        lengths = [T, int(rng.integers(0, T + 1))]
        on, off, ptr = LR.notes_from_roll(ref)
        for oa in (None, o):
            want = NR.match_counts_active(f, ref, oa, lengths)
            for matcher in ("scipy", "stream"):
                got = LR.match_list_counts_active(f, on, off, ptr, oa, lengths, matcher)
                # a roll run cut by `lengths` ends at L; the list clips its offset to 320 L: the same note
                np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("script,flags", [("scripts/train_cnn.py", ["--onset_labels"]), ("scripts/evaluate.py", ["--note_reference"])])
def test_help_lists_the_new_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for f in flags:
        assert f in r.stdout and "midi" in r.stdout, (script, f)


def test_onset_labels_midi_needs_all_heads_and_recordings(tmp_path):
    base = [sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--model", "cnn_rnn_large", "--onset_labels", "midi",
            "--chunk_length", "30", "--cached_dir", str(tmp_path / "none")]
    r = subprocess.run(base + ["--root_dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--train_all_heads" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["--train_all_heads", "--root_dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--onset_labels midi" in r.stderr and str(tmp_path) in r.stderr, r.stderr[-2000:]
    with open(tmp_path / "maestro-v3.0.0.csv", "w") as fh:               # a csv without train recordings
        fh.write("canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration\nX,Y,test,2004,a.midi,a.wav,1.0\n")
    r = subprocess.run(base + ["--train_all_heads", "--root_dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "no train recordings" in r.stderr, r.stderr[-2000:]


def test_note_reference_midi_needs_full_files(tmp_path):
    for source in ([], ["--data_source", "cache"], ["--data_source", "auto"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", str(tmp_path / "m.pth"), "--note_metrics",
                            "--note_reference", "midi", "--headless"] + source, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--data_source full" in r.stdout + r.stderr, (r.stdout[-2000:], r.stderr[-2000:])


def test_dataset_and_evaluation_refuse_bad_references(mta):
    from music_transcription_amd import evaluate as E, rawdata as RD
    with pytest.raises(ValueError, match="onset_labels"):
        mta.MaestroDataset("root", onset_labels="diff")
    ds = RD.MaestroDataset.__new__(RD.MaestroDataset)
    ds.onset_labels, ds.chunk_length = "midi", 30.0
    with pytest.raises(NotImplementedError, match="--data_source full"):
        ds.ref_notes([0])
    ds.onset_labels = "roll"
    with pytest.raises(RuntimeError, match="onset_labels='midi'"):
        ds.ref_notes([0])
    with pytest.raises(ValueError, match="data_source full"):
        E.note_metrics_dataset(None, ds, note_reference="midi")
    with pytest.raises(ValueError, match="note_reference"):
        E.note_metrics_dataset(None, ds, note_reference="notes")
