"""The decoder grid in ticks without a GPU (DESIGN.md 6c "Decoder grid in ticks"): the conditions that keep test_gpu_note_grid_ticks.py
from being vacuous, asserted on the host composition decode -> refine -> notes.note_match_ticks of note_grid_ticks_case; the argument
checks and refusals of evaluate.tune_note_decoder(refine_onsets=True) that need no device; and the compiler's metadata of the new
kernels (no private segment, LDS for at least two workgroups per compute unit)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import note_grid_ticks_case as C
import note_ticks_case as TC
from music_transcription_amd import evaluate as E
from music_transcription_amd import notes as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "music-transcription_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def case():
    return C.Case()


@pytest.fixture(scope="module")
def main_counts(case):
    """{cell index: (counts on refined ticks, counts on the 320 s stamps)} of the 32 cells of the main grid, (B, 4) each."""
    out = {}
    for idx, cell in C.cells(C.GRID):
        out[idx] = tuple(N.note_match_ticks(case.host_tables(cell, 2, refined=r), case.ref).astype(np.int64) for r in (True, False))
    return out


def test_case_shape(case):
    assert case.frame.shape == (C.B, C.P, C.T) == (3, 88, 1100) and C.LENGTHS == [1100, 600, 0]
    for b, L in enumerate(C.LENGTHS):
        assert np.isnan(case.frame[b, :, L:]).all() and not np.isnan(case.frame[b, :, :L]).any()
    ptr = case.ref["ptr"]
    assert len(ptr) == C.B * C.P + 1 and ptr[-1] == len(case.ref["on"]) > 500
    for on, off in TC.rows_of(case.ref):
        assert (np.diff(on) >= 0).all() and (off > on).all() and (on >= 0).all()
    assert ptr[-1] > ptr[2 * C.P]                           # the recording without frames has reference notes


def test_most_cells_differ(main_counts):
    """At least three quarters of the 32 cells of the main grid have count vectors of their own."""
    assert len(main_counts) == 32
    distinct = {tuple(c[0].reshape(-1)) for c in main_counts.values()}
    print("distinct count vectors:", len(distinct))
    assert len(distinct) >= 24


def test_refinement_changes_tp_onset(main_counts):
    """For at least one cell tp_onset on refined ticks differs from tp_onset on the 320 s stamps."""
    diff = [idx for idx, (a, b) in main_counts.items() if (a[:, 2] != b[:, 2]).any()]
    print("cells whose tp_onset moves with the refinement:", len(diff))
    assert diff
    for a, b in main_counts.values():                       # the refinement moves onsets, it neither adds nor removes a note
        assert (a[:, :2] == b[:, :2]).all()


def test_special_rows(case):
    """TRIPLE: three refined onsets within 960 ticks (peak detector, reach 1).  CHAIN: one connected component of more than 64 reference
    notes, by the kernel's own definition (note_ticks_case.row_counts)."""
    cell = (0.4, 0.35, 0.4, (1, 0), 1)
    est = case.host_tables(cell, 2)
    rows_e, rows_r = TC.rows_of(est), TC.rows_of(case.ref)
    b, p = C.TRIPLE
    on = np.sort(rows_e[b * C.P + p][0])
    assert len(on) == 3 and on[2] - on[0] <= 960, on
    r_on = rows_r[b * C.P + p][0]
    assert any(((on >= r - 500) & (on <= r + 500)).sum() == 3 for r in r_on)       # three estimates inside one reference window
    b, p = C.CHAIN
    (eo, ef), (ro, rf) = rows_e[b * C.P + p], rows_r[b * C.P + p]
    assert len(ro) == C.CHAIN_N and len(eo) == C.CHAIN_N
    stats = TC.row_counts(eo, ef, ro, rf)
    assert max(j - i for i, j in stats["components"]) > 64, stats["components"]
    # somewhere in the case the refinement is not a no-op, and strikes 2 to 3 frames apart decode as notes of their own
    assert (est["on"] % 320 != 0).sum() > 100
    gaps = np.concatenate([np.diff(o) for o, _ in rows_e if len(o) > 1])
    assert ((gaps >= 640 - 320) & (gaps <= 960 + 320)).sum() > 50


class _NoModel:
    pass


class _Midi:
    onset_labels, chunk_length = "midi", None

    def __len__(self):
        return 0


class _Roll:
    onset_labels, chunk_length = "roll", 938

    def __len__(self):
        return 0


@pytest.mark.parametrize("kwargs, words", [
    (dict(decoder="frame", note_reference="midi"), "needs decoder 'onset' or 'onset_offset'"),
    (dict(decoder="onset", note_reference="roll"), "note_reference='midi'"),
    (dict(decoder="onset", note_reference="midi", smoothings=[(0.0, 0.0), (1.0, 1.0)]), "smoothings"),
    (dict(decoder="onset", note_reference="midi", refine_reach=9), "refine_reach"),
    (dict(decoder="onset", note_reference="midi", refine_reach=True), "refine_reach"),
    (dict(decoder="onset_offset", note_reference="midi", onset_detect="peak"), "peak_reaches"),
    (dict(decoder="onset", note_reference="midi", smooth_on=1.0), "smooth"),
])
def test_tuner_refusals(kwargs, words):
    """tune_note_decoder(refine_onsets=True) refuses, before it touches the model or a device, what the tick grid cannot score."""
    ds = _Roll() if kwargs.get("note_reference") == "roll" else _Midi()
    with pytest.raises(ValueError, match=re.escape(words)):
        E.tune_note_decoder(_NoModel(), ds, device="cpu", refine_onsets=True, **kwargs)


def test_tuner_needs_midi_dataset():
    with pytest.raises(ValueError, match="MaestroDataset"):
        E.tune_note_decoder(_NoModel(), _Roll(), device="cpu", decoder="onset", note_reference="midi", refine_onsets=True)


def test_script_still_refuses_its_tuners_with_refined_onsets():
    """scripts/evaluate.py keeps refusing --refine_onsets with its three tuners (tests/test_onset_regress_cpu.py pins that); for
    --tune_note_decoder the message names the Python call that does tune on refined onsets."""
    import sys
    base = [sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", "none.pth", "--data_source", "full", "--note_metrics",
            "--note_reference", "midi", "--decoder", "onset", "--refine_onsets"]
    for flag in ("--tune_threshold", "--tune_note_thresholds", "--tune_note_decoder"):
        r = subprocess.run(base + [flag], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--refine_onsets cannot be combined with " + flag in r.stderr, (flag, r.stderr)
        assert ("tune_note_decoder(refine_onsets=True)" in r.stderr) == (flag == "--tune_note_decoder"), (flag, r.stderr)
    r = subprocess.run(base, capture_output=True, text=True, timeout=120)           # without a tuner the flags parse
    assert r.returncode == 1 and "Model checkpoint not found" in r.stdout, (r.stdout, r.stderr)


def test_grid_ticks_argument_checks():
    """notes.note_grid_ticks_counts raises on the host, before any device work, for what needs no tensor to see."""
    with pytest.raises(ValueError, match="onset_logits"):
        N.note_grid_ticks_counts(None, None, {}, [0.5], [0.5])
    with pytest.raises(ValueError, match="refine_reach"):
        N.note_grid_ticks_counts(None, object(), {}, [0.5], [0.5], refine_reach=9)
    with pytest.raises(ValueError, match="peak_reaches"):
        N.note_grid_ticks_counts(None, object(), {}, [0.5], [0.5], peak_reaches=[9])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_have_no_scratch(tmp_path):
    """Every kernel of notes_grid_ticks.hip and the tick matcher: private_seg_size 0; the grid kernels' LDS fits a compute unit at least
    twice (the figures of DESIGN.md 6c "Decoder grid in ticks")."""
    seen = 0
    for src, pattern, lds_bound in (("notes_grid_ticks.hip", "notes_grid_ticks", CU_LDS // 2), ("note_ticks.hip", "note_match_ticks_kernel", 0)):
        out = tmp_path / (src + ".s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                        os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True, timeout=900)
        txt = out.read_text()
        scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (\S+)\.private_seg_size, (\d+)", txt)}
        meta = {}
        for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)", txt):
            meta[m.group(2)] = (int(m.group(1)), int(m.group(3)))
        names = [k for k in meta if pattern in k]
        assert names, (src, sorted(meta))
        for k in names:
            lds, priv = meta[k]
            print(k, "lds", lds, "scratch", scratch.get(k), priv)
            assert scratch[k] == 0 and priv == 0, (k, scratch[k], priv)
            assert lds <= lds_bound, (k, lds)
            seen += 1
    assert seen >= 7            # count / fill x onset- / offset-gated, prefix, refine, and the matcher
