"""Workgroups of the plain inference recurrence per compute unit, checked on the compiler's own metadata of the gfx950 code object
(hipcc cross-compiles without a GPU).

A plain inference recurrence workgroup is five waves (4 compute + the gx loader).  A SIMD has 512 registers per lane: at 96 or fewer
(VGPRs + AGPRs, in the allocation granule of 8) it holds 5 waves, a CU 20 -- FOUR workgroups, 32 CUs per launch at H = 512 instead of the
43 of three per CU.  That packing was built (the f16-gx instances compile to 96 registers without scratch under a bound of 5 waves per
SIMD) and measured: a launch under load runs 15 % longer, the GEMMs of the other forwards gain nothing, the default schedule loses 3 %
(profiles/lstm_pack4_*.txt).  What ships is the same leaner kernel at THREE per CU, which is 4 - 5 % faster than before.  So this test
pins three: registers above 96 and within 128, no scratch, and a third of the CU's LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "music-transcription_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SIMD_REGS = 512            # registers per lane of one SIMD (VGPRs + AGPRs, unified)
CU_LDS = 160 * 1024        # bytes of LDS per compute unit (gfx950)
WAVES_PER_WG = 5
SIMDS = 4


def _alloc(v, a):
    """registers a wave occupies: the AGPRs start at a multiple of 4, the total is allocated in granules of 8"""
    return ((v + 3) // 4 * 4 + a + 7) // 8 * 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_three_inference_recurrence_workgroups_per_cu_not_four(tmp_path):
    """lstm_rec_kernel<8, false, false, NG, true> for NG = 1..4 -- H = 512, f16 gx: the instances of the default bench schedule -- have no
    private segment, fit a CU three times by registers and by LDS, and do NOT fit it four times (the occupancy query, and with it the
    residency accounting of csrc/residency.hip, follows these figures: 43 CUs per launch of 128 workgroups)."""
    out = tmp_path / "lstm.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    os.path.join(CSRC, "lstm.hip"), "-o", str(out)], check=True, capture_output=True, timeout=900)
    txt = out.read_text()
    v = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (\S+)\.num_vgpr, (\d+)", txt)}
    a = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (\S+)\.num_agpr, (\d+)", txt)}
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (\S+)\.private_seg_size, (\d+)", txt)}
    # the kernel descriptors' own figures (what the loader and the occupancy query see)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)", txt):
        meta[m.group(2)] = (int(m.group(1)), int(m.group(3)), int(m.group(4)))
    want = ["_ZN2mt15lstm_rec_kernelILi8ELb0ELb0ELi%dELb1EEEvNS_8LstmArgsE" % ng for ng in (1, 2, 3, 4)]
    for k in want:
        assert k in v and k in scratch and k in meta, k
        regs = _alloc(v[k], a.get(k, 0))
        lds, priv, vcount = meta[k]
        print(k, "vgpr", v[k], "agpr", a.get(k, 0), "allocated", regs, "lds", lds, "scratch", scratch[k])
        assert scratch[k] == 0 and priv == 0, (k, scratch[k], priv)
        assert 96 < regs <= 128 and vcount <= 128, (k, v[k], a.get(k, 0), vcount)
        assert lds <= CU_LDS // 3, (k, lds)
        # what the numbers are for: waves per SIMD -> workgroups per CU, by registers and by LDS
        waves = SIMD_REGS // regs
        assert min(SIMDS * waves // WAVES_PER_WG, CU_LDS // lds) == 3, (k, regs, lds)
