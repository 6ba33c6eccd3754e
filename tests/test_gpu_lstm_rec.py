"""The persistent LSTM recurrence kernels of csrc/lstm.hip and csrc/lstm_bwd.hip, every variant the dispatch code can launch, one by one
through the C ABI against the float64 step models of tests/lstm_rec_ref.py (checked on the CPU by tests/test_lstm_rec_ref_cpu.py): gx, the saved
tensors and dh are fed in their packed layouts with no projection GEMM in front; one recurrence entry point per call; the status word must be 0.

Two comparisons per case (live batch slots only, every element counts):
  * against the KERNEL-ROUNDED model (float64 arithmetic with the kernel's rounding points): the tolerances below;
  * against the EXACT model: 2 x (distance of the kernel-rounded model to the exact one, computed per case on the CPU) + 8 f32 epsilons of the
    quantity's magnitude (tests/lstm_rec_ref.py, exact_slack: at T = 1 the two models agree exactly in c and the gates, the first term is 0 and the
    kernel still rounds in f32) -- a bound that comes from the reference alone and can fail on its own.

Tolerances = 4 x the worst error measured over ALL cases of this module on an MI355X (f32 summation order, v_exp_f32 / v_rcp_f32, and a published
f16 / stored bf16 value landing on the other side of a rounding boundary), never above the ceiling the quantity has for other reasons:

  quantity                      metric               measured worst (case)                   4 x        tolerance
  h   (published, f16)          max |d|              4.883e-4  fwd (48, 33, 11)              1.95e-3    6e-4    the ceiling of test_lstm_layer_matches_oracle (*)
  h                             mean |d|             2.149e-6  xproj (512, 32, 9)            8.6e-6     8.6e-6  (ceiling 2e-5, the same test)
  c   (train mode, f32)         max |d|              2.882e-4  train (512, 40, 11)           1.15e-3    1.16e-3
  c                             mean |d|             4.230e-6  train (512, 40, 11)           1.69e-5    1.7e-5
  activated gates (train, f32)  max |d|              2.809e-4  train (128, 70, 11)           1.12e-3    1.13e-3
  activated gates               mean |d|             2.352e-6  train (512, 40, 11)           9.4e-6     9.5e-6
  dgates (bf16), gate i         max |d| / max |ref|  5.682e-3  bwd (512, 16, 9)              2.27e-2    2.28e-2  per gate, each relative to that gate's maximum in the
  dgates, gate f                of the gate (**)     8.097e-3  bwd (512, 16, 9)              3.24e-2    3.24e-2  case (tests/lstm_rec_ref.py, dg_rel): 2.8 .. 4.2 bf16 ulps
  dgates, gate g                                     5.405e-3  bwd (48, 16, 9)               2.16e-2    2.17e-2  (2^-7) of a maximum that is itself at most the case's
  dgates, gate o                                     6.849e-3  bwd (400, 1, 9)               2.74e-2    2.74e-2
  (*) 4.883e-4 is 2^-11, ONE f16 ulp of an |h| in [0.5, 1): a published h on the other side of a rounding boundary.  The error of h cannot be a
      second ulp unless the pre-activations are off by far more than f32 noise, so the ceiling (1.23 ulps) is kept and not raised to 4 x.
  (**) each worst value is about one bf16 ulp of an element near the gate's maximum (2^-8 .. 2^-7 of it): a stored dgate on the other side of a
      rounding boundary.  A gate whose reference is all zero (f at T = 1: c_prev = 0) must be exactly zero.  bwd (16, 1, 9) reproduces the
      kernel-rounded model bit for bit.

What is launched (read against launch_rec / launch_rec_plain, lstm_fwd_impl, mt_lstm_bidir_bwd_ex).  NKSW = ceil(H / 64) rounded up to 1, 2, 4, 8 or 16: H = 16, 48 -> 1; 96, 128 -> 2; 208, 256 -> 4
(208 ragged); 272 (ragged), 512 -> 8; 528 -> 16.
  forward   B <= 16 and NKSW <= 8: lstm_rec16_kernel plain / G16 / TRAIN;  B = 17 .. 32: lstm_rec_kernel NG = 1 (plain, G16, TRAIN);
            B = 33, 70, 100: NG = 2, 3, 4 interleaved in one set of workgroups, B = 130: 4 + 1 groups in grid.z = 2 with a ragged last group;
            TRAIN with B = 40, 70: grid.z = 2, 3;  H = 528: the 32-column kernel at every B, one group per workgroup and -- 2 x 66 = 132 workgroups
            per group, so zmax = 256 / 132 = 1 in lstm_fwd_impl -- B = 40 as TWO launches of 132 workgroups made by the library (g0 = 0, 1);
            XP (fused projection): H <= 512 (NKSW = 1, 2, 4, 8 at H = 16 / 48, 128, 256, 512), one group per grid.z.
  backward  lstm_bptt_kernel<TPW, ONE>: TPW = 1 for NW = ceil(H / 32) <= 8 (H = 16, 48, 96, 256 -> NW = 1, 2, 3, 8), TPW = 2 above (272, 400, 512 ->
            NW = 9, 13, 16: `wc < NW` ragged at 9 and 13); ONE for B <= 16; H = 48: 6 unit blocks in 2 workgroups (`kb < nkb`); B = 17, 40: `cb < Bg`.
Every launch has at most 256 workgroups: the backward's 2 NW NG and the fused projection's 2 H/8 NG (one workgroup per CU: at most 128 here) are
asserted; the other forward grids are cut to 2 H/8 zmax <= 256 by lstm_fwd_impl itself, which a test through the C ABI cannot observe.

Run only this file:  python -m pytest tests/test_gpu_lstm_rec.py -q -m gpu -s      (-s shows every measured figure)
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_layout_ref as L  # noqa: E402
import lstm_rec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# ---- tolerances against the kernel-rounded model (the table above)
TOL_H_MAX, TOL_H_MEAN = 6e-4, 8.6e-6
TOL_C_MAX, TOL_C_MEAN = 1.16e-3, 1.7e-5
TOL_G_MAX, TOL_G_MEAN = 1.13e-3, 9.5e-6
TOL_DG_REL = (2.28e-2, 3.24e-2, 2.17e-2, 2.74e-2)                   # per gate i, f, g, o

# ---- cases (H, B, T)
FWD_CASES = [(16, 1, 1), (16, 17, 2), (16, 130, 2), (48, 16, 11), (48, 33, 11), (96, 32, 1), (96, 70, 11), (128, 16, 2), (128, 100, 2), (128, 130, 11),
             (208, 5, 11), (256, 17, 2), (272, 1, 11), (272, 17, 2), (512, 16, 11), (512, 32, 2), (528, 3, 11), (528, 40, 11)]
G16_CASES = [(16, 16, 11), (48, 1, 2), (48, 100, 11), (96, 17, 11), (96, 70, 2), (128, 33, 11), (128, 16, 2), (128, 130, 1), (208, 40, 2), (256, 16, 11), (272, 32, 11), (512, 1, 11),
             (512, 17, 2), (528, 3, 2), (528, 40, 11)]
TRAIN_CASES = [(16, 1, 11), (16, 70, 1), (48, 16, 2), (96, 17, 11), (128, 1, 2), (128, 70, 11), (208, 1, 2), (256, 17, 11), (272, 16, 11), (272, 40, 2), (512, 16, 1),
               (512, 40, 11), (528, 3, 11), (528, 40, 2)]
XP_CASES = [(16, 3, 9, None), (48, 32, 9, None), (48, 40, 1, None), (48, 3, 9, 40), (128, 3, 1, None), (128, 40, 9, None), (256, 3, 9, None), (512, 3, 9, None),
            (512, 32, 9, None)]                                                     # (H, B, T, Hv): Hv = 40: zero w_ihx columns for the padded units
BWD_CASES = [(16, 1, 9), (16, 40, 2), (48, 16, 9), (48, 17, 9), (48, 40, 1), (96, 1, 1), (96, 32, 9), (96, 32, 2), (256, 16, 9), (256, 40, 9), (272, 16, 9),
             (272, 17, 9), (272, 40, 9), (400, 1, 9), (400, 32, 9), (512, 16, 9), (512, 40, 9)]      # (T = 2 at NW <= 3: see test_gpu_backward_cases_discriminate)

GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
GX_F16 = 0x10                               # MT_GX_F16 of include/mt_hip.h


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _lib():
    from music_transcription_amd._lib import lib, check, stream_ptr
    return lib, check, stream_ptr()


def _dev(a):
    """a numpy array of any word size -> its bytes on the device"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class _Out:
    """nbytes of output between two 4-KB guard bands; `init` (a numpy array) is what the middle holds before the call, the sentinel byte otherwise"""

    def __init__(self, nbytes, init=None):
        self.n = nbytes
        self.buf = torch.full((2 * GUARD_BYTES + nbytes,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        if init is not None:
            src = _dev(init)
            assert src.numel() == nbytes
            self.buf[GUARD_BYTES:GUARD_BYTES + nbytes] = src
        self.ptr = self.buf.data_ptr() + GUARD_BYTES
        assert self.ptr % 16 == 0

    def read(self, dtype):
        return self.buf[GUARD_BYTES:GUARD_BYTES + self.n].cpu().numpy().view(dtype)

    def guards_ok(self):
        return bool((self.buf[:GUARD_BYTES] == GUARD_BYTE).all().item()) and bool((self.buf[GUARD_BYTES + self.n:] == GUARD_BYTE).all().item())


def _status_ok(sync):
    assert int(sync[:4].view(torch.int32).item()) == 0, "hand-off timeout"


def _f16_bits_to_f64(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)


def _errs(got, want):
    d = np.abs(got - want)
    return float(d.max()), float(d.mean())


# ================================================================== forward
def _run_fwd(entry, H, B, T, w_hh, gx_img=None, xp=None):
    """one call of one forward entry point; returns (h bits [B][T][2][H], c or None, activated gates or None) of the live batch slots"""
    lib, check, st = _lib()
    assert entry != "xproj" or 2 * (H // 8) * L.groups(B) <= 128           # (one workgroup per CU there; the other forward grids: see the header)
    whh = _dev(w_hh)
    hx = _Out(lib.mt_lstm_hx_bytes(B, T, H))
    assert hx.n == L.hx_words(B, T, H) * 2
    sync = torch.full((lib.mt_lstm_sync_bytes(B, H),), 0x5A, dtype=torch.uint8, device="cuda")
    cx = gx = None
    if entry == "xproj":
        x_img, w_ihx, bias = xp
        xd, wd, bd = _dev(x_img), _dev(w_ihx), _dev(bias)
        check(lib.mt_lstm_bidir_fwd_xproj(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), whh.data_ptr(), hx.ptr, sync.data_ptr(), sync.numel(), B, T, H, st))
    elif entry == "train":
        assert lib.mt_lstm_gx_bytes(B, T, H) == gx_img.nbytes
        gx = _Out(gx_img.nbytes, gx_img)
        cx = _Out(lib.mt_lstm_cx_bytes(B, T, H))
        assert cx.n == L.cell_words(B, T, H) * 4
        check(lib.mt_lstm_bidir_fwd_train(gx.ptr, whh.data_ptr(), hx.ptr, cx.ptr, sync.data_ptr(), sync.numel(), B, T, H, st))
    else:
        gxd = _dev(gx_img)
        if entry == "fwd":
            check(lib.mt_lstm_bidir_fwd(gxd.data_ptr(), whh.data_ptr(), hx.ptr, sync.data_ptr(), sync.numel(), B, T, H, st))
        else:
            check(lib.mt_lstm_bidir_fwd_ex(gxd.data_ptr(), whh.data_ptr(), hx.ptr, sync.data_ptr(), sync.numel(), B, T, H, GX_F16 if entry == "g16" else 0, st))
    torch.cuda.synchronize()
    _status_ok(sync)
    assert hx.guards_ok(), "hx: a guard band was written"
    h_bits = L.decode_hx(hx.read(np.uint16), B, T, H)
    c = gates = None
    if entry == "train":
        assert cx.guards_ok() and gx.guards_ok(), "cx / gates: a guard band was written"
        c = L.decode_cell(cx.read(np.float32), B, T, H).astype(np.float64)
        gates = R.decode_gx(gx.read(np.float32), B, T, H).astype(np.float64)
    return h_bits, c, gates


@functools.lru_cache(maxsize=4)
def _fwd_ref(H, B, T, g16):
    gx, w_hh = R.fwd_case(H, B, T, g16)
    return gx, w_hh, R.lstm_fwd(gx, w_hh, True), R.lstm_fwd(gx, w_hh, False)


def _check_h(tag, case, h_bits, rounded, exact):
    h = _f16_bits_to_f64(h_bits)
    assert np.isfinite(h).all(), "h holds a non-finite value (an unpublished, still poisoned word?)"
    assert np.abs(h).max() > 0.05
    emax, emean = _errs(h, rounded[0])
    eex, dist = _errs(h, exact[0])[0], _errs(rounded[0], exact[0])[0]
    print(f"MEASURE {tag} {case} h_max {emax:.3e} h_mean {emean:.3e} h_exact {eex:.3e} model_dist {dist:.3e}")
    assert emax < TOL_H_MAX and emean < TOL_H_MEAN, (emax, emean)
    assert eex <= 2 * dist + R.exact_slack(exact[0]), (eex, dist)


def _inference(entry, case, g16):
    H, B, T = case
    gx, w_hh, rounded, exact = _fwd_ref(H, B, T, g16)
    img = R.encode_gx(gx, np.nan, np.float16 if g16 else np.float32)           # padded batch slots: NaN (the kernel must not let them in)
    h_bits, _, _ = _run_fwd(entry, H, B, T, w_hh, img)
    _check_h(entry, case, h_bits, rounded, exact)
    again, _, _ = _run_fwd(entry, H, B, T, w_hh, img)
    assert np.array_equal(h_bits, again), "two runs of the same launch differ"


@pytest.mark.parametrize("case", FWD_CASES, ids=str)
def test_fwd_inference(mta, case):
    """mt_lstm_bidir_fwd, f32 gx: lstm_rec16_kernel<NK, false, false> (B <= 16, H <= 512), lstm_rec_kernel<NKSW, false, false, NG, false> otherwise"""
    _inference("fwd", case, False)


@pytest.mark.parametrize("case", G16_CASES, ids=str)
def test_fwd_inference_gx_f16(mta, case):
    """mt_lstm_bidir_fwd_ex(MT_GX_F16): the loader wave streams 2-KB f16 blocks; the model gets the same f16 values"""
    _inference("g16", case, True)


@pytest.mark.parametrize("case", TRAIN_CASES, ids=str)
def test_fwd_train(mta, case):
    """mt_lstm_bidir_fwd_train: lstm_rec16_kernel<NK, true, false> (B <= 16, H <= 512) / lstm_rec_kernel<NKSW, true, false> with batch groups in grid.z:
    h, the cell states and the activated gates (which overwrite gx) against the model; h bit for bit the inference run's (mt_lstm_bidir_fwd_ex, flags 0)"""
    H, B, T = case
    gx, w_hh, rounded, exact = _fwd_ref(H, B, T, False)
    img = R.encode_gx(gx, np.nan)
    h_bits, c, gates = _run_fwd("train", H, B, T, w_hh, img)
    _check_h("train", case, h_bits, rounded, exact)
    for name, got, k, tmax, tmean in (("c", c, 1, TOL_C_MAX, TOL_C_MEAN), ("gates", gates, 2, TOL_G_MAX, TOL_G_MEAN)):
        assert np.isfinite(got).all(), name
        emax, emean = _errs(got, rounded[k])
        eex, dist = _errs(got, exact[k])[0], _errs(rounded[k], exact[k])[0]
        print(f"MEASURE train {case} {name}_max {emax:.3e} {name}_mean {emean:.3e} {name}_exact {eex:.3e} model_dist {dist:.3e}")
        assert emax < tmax and emean < tmean, (name, emax, emean)
        assert eex <= 2 * dist + R.exact_slack(exact[k]), (name, eex, dist)
    inf_bits, _, _ = _run_fwd("ex", H, B, T, w_hh, img)
    assert np.array_equal(h_bits, inf_bits), "train mode changed h"


@pytest.mark.parametrize("case", XP_CASES, ids=str)
def test_fwd_fused_projection(mta, case):
    """mt_lstm_bidir_fwd_xproj: lstm_rec_kernel<NKSW, false, true>; x_t is read from the previous layer's hx image (encode_hx; padded batch slots 0)"""
    H, B, T, Hv = case
    x_bits, w_ihx, bias, w_hh = R.xproj_case(H, B, T, Hv)
    x = _f16_bits_to_f64(x_bits).reshape(B, T, 2 * H)
    rounded, exact = R.lstm_fwd(None, w_hh, True, xproj=(x, w_ihx, bias)), R.lstm_fwd(None, w_hh, False, xproj=(x, w_ihx, bias))
    xp = (L.encode_hx(x_bits, 0), w_ihx, bias)
    h_bits, _, _ = _run_fwd("xproj", H, B, T, w_hh, xp=xp)
    _check_h("xproj", case, h_bits, rounded, exact)
    again, _, _ = _run_fwd("xproj", H, B, T, w_hh, xp=xp)
    assert np.array_equal(h_bits, again), "two runs of the same launch differ"


# ================================================================== backward
def _run_bwd(H, B, T, imgs, w_hh, poisoned):
    """one mt_lstm_bidir_bwd_ex call on the packed saved tensors; returns the dgates' bf16 bits [B][T][2][4][H] of the live batch slots"""
    lib, check, st = _lib()
    assert 2 * ((H + 31) // 32) * L.groups(B) <= 256
    gd, cd, dd, whh = (_dev(a) for a in imgs + (w_hh,))
    dgx = _Out(lib.mt_lstm_dgx_bytes(B, T, H))
    assert dgx.n == R.dgx_words(B, T, H) * 2
    pbytes = lib.mt_lstm_bwd_part_bytes(B, T, H)
    part = torch.zeros(pbytes, dtype=torch.uint8, device="cuda")           # zeros: a hand-off that is not poisoned reads wrong partials, never waits
    sync = torch.full((lib.mt_lstm_sync_bytes(B, H),), 0x5A, dtype=torch.uint8, device="cuda")
    if poisoned:
        check(lib.mt_lstm_bwd_poison(part.data_ptr(), pbytes, B, T, H, st))
    check(lib.mt_lstm_bidir_bwd_ex(gd.data_ptr(), cd.data_ptr(), dd.data_ptr(), whh.data_ptr(), dgx.ptr, part.data_ptr(), pbytes, sync.data_ptr(), sync.numel(),
                                   B, T, H, 1 if poisoned else 0, st))
    torch.cuda.synchronize()
    _status_ok(sync)
    assert dgx.guards_ok(), "dgx: a guard band was written"
    return R.decode_dgx(dgx.read(np.uint16), B, T, H)


@pytest.mark.parametrize("case", BWD_CASES, ids=str)
def test_bwd(mta, case):
    """mt_lstm_bidir_bwd_ex on synthetic saved tensors: the per-step dgates themselves against the backward model; the pre-poisoned workspace
    (flags = 1 behind mt_lstm_bwd_poison, the path training uses) and a second run are bit-identical"""
    H, B, T = case
    gates, cx, dh, w_hh = R.bwd_case(H, B, T)
    rounded, exact = R.lstm_bwd(gates, cx, dh, w_hh, True), R.lstm_bwd(gates, cx, dh, w_hh, False)
    imgs = (R.encode_gx(gates, np.nan), L.encode_cell(cx, np.nan), L.encode_cell(dh, np.nan))        # padded batch slots: NaN (never read)
    bits = _run_bwd(H, B, T, imgs, w_hh, False)
    got = R.bf16_bits_to_f64(bits)
    assert np.isfinite(got).all()
    assert np.abs(rounded).max() > 0.05
    rel, rel_ex, dist = R.dg_rel(got, rounded), R.dg_rel(got, exact), R.dg_rel(rounded, exact)          # per gate i, f, g, o
    fmt = lambda a: " ".join(f"{v:.3e}" for v in a)
    print(f"MEASURE bwd {case} dg_rel {fmt(rel)} dg_exact {fmt(rel_ex)} model_dist {fmt(dist)}")
    assert (rel < np.array(TOL_DG_REL)).all(), rel
    assert (rel_ex <= 2 * dist + 8 * R.F32_EPS).all(), (rel_ex, dist)
    assert np.array_equal(bits, _run_bwd(H, B, T, imgs, w_hh, True)), "the pre-poisoned workspace (flags = 1) changed dgx"
    assert np.array_equal(bits, _run_bwd(H, B, T, imgs, w_hh, False)), "two runs of the same launch differ"
