"""The LSTM layout movers of csrc/lstm.hip and csrc/lstm_bwd.hip, one by one through the C ABI: mt_lstm_unpack_f32, mt_lstm_relayout_dt /
_ex / _bf16, mt_lstm_relayout_train, mt_lstm_dh_relayout, mt_lstm_hprev_t and mt_lstm_dg_unpack.  Exact comparisons only, and nothing here runs a
recurrence: every input image is built by tests/lstm_layout_ref.py (numpy; tests/test_post_optim_ref_cpu.py checks it index by index against the
formulas of include/mt_hip.h; the dgx image of mt_lstm_dg_unpack by tests/lstm_rec_ref.py, checked by tests/test_lstm_rec_ref_cpu.py) from random
finite f16 bit patterns that are all distinct while there are enough of them, so a misplaced
element cannot equal the right one.  Batch slots >= B of an input image hold NaN; every output lies in a sentinel-filled buffer (0x7FC1 for
16-bit words, an f32 NaN pattern for floats) between two guard bands with spare rows behind it, and is compared whole: what the contract
does not write must still hold the sentinel.

Run only this file:  python -m pytest tests/test_gpu_lstm_layouts.py -q -m gpu
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_layout_ref as L  # noqa: E402
import lstm_rec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256
SENT16, SENT32 = 0x7FC1, 0x7FC0BEEF
PAD16 = 0x7E00                              # an f16 NaN in the batch slots >= B of an hx image
MT_EINVAL = -1
DT = {"bf16": 0, "f16": 1}                  # MT_DT_* of include/mt_hip.h
SHAPES = [(1, 1, 16), (5, 3, 16), (16, 4, 48), (33, 5, 32), (70, 3, 64), (40, 2, 512)]       # one, two, three batch groups, ragged last groups,
SPARE_ROWS = 2                                                                               # H/16 odd and even, the canonical width


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _lib():
    from music_transcription_amd._lib import lib, stream_ptr
    return lib, stream_ptr()


def _ok(rc):
    if rc != 0:
        from music_transcription_amd._lib import last_error
        raise AssertionError(f"call failed (code {rc}): {last_error()}")


def _dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


class _Out:
    """n words of 2 or 4 bytes between two guard bands, all of it pre-filled with the sentinel; read back as unsigned bits"""

    def __init__(self, n, size):
        self.n, self.size = n, size
        self.sent = SENT16 if size == 2 else SENT32
        self.buf = torch.full((2 * GUARD + n,), self.sent, dtype=torch.int16 if size == 2 else torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * size

    def bits(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(np.uint16 if self.size == 2 else np.uint32)

    def guards_ok(self):
        return bool((self.buf[:GUARD] == self.sent).all().item()) and bool((self.buf[GUARD + self.n:] == self.sent).all().item())

    def untouched(self):
        return bool((self.buf == self.sent).all().item())


def _case(B, T, H):
    bits = L.distinct_f16_bits((B, T, 2, H), 100 + B + 7 * T + H)
    return bits, _dev(L.encode_hx(bits, PAD16))


def _f32_bits(bits16):
    return bits16.view(np.float16).astype(np.float32).view(np.uint32)


def _roundup(x, m):
    return (x + m - 1) // m * m


# ================================================================== mt_lstm_unpack_f32
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_unpack_f32_exact(mta, B, T, H):
    """y[b][t][d H + k] == float(h[b][t][d][k]); the NaN of the pad slots appears nowhere"""
    lib, st = _lib()
    bits, hx = _case(B, T, H)
    y = _Out(B * T * 2 * H, 4)
    _ok(lib.mt_lstm_unpack_f32(hx.data_ptr(), y.ptr, B, T, H, st))
    torch.cuda.synchronize()
    assert y.guards_ok() and np.array_equal(y.bits(), _f32_bits(bits).reshape(-1))


# ================================================================== mt_lstm_relayout_dt / _ex / _bf16
def _relayout(lib, st, hx, B, T, H, Hv, col_off, dt, want_x, want_y, ldx=None, ldy=None, entry="dt"):
    ldx = _roundup(col_off + 2 * Hv, 8) + 8 if ldx is None else ldx
    ldy = col_off + 2 * Hv + 3 if ldy is None else ldy
    rows = T * B + SPARE_ROWS
    X = _Out(rows * ldx, 2) if want_x else None
    Y = _Out(rows * ldy, 4) if want_y else None
    xp, yp = (X.ptr if X else None), (Y.ptr if Y else None)
    if entry == "dt":
        rc = lib.mt_lstm_relayout_dt(hx.data_ptr(), xp, ldx, yp, ldy if Y else 0, col_off, B, T, H, Hv, DT[dt], st)
    elif entry == "ex":
        rc = lib.mt_lstm_relayout_ex(hx.data_ptr(), xp, ldx, yp, ldy if Y else 0, col_off, B, T, H, Hv, st)
    else:
        rc = lib.mt_lstm_relayout_bf16(hx.data_ptr(), xp, ldx, B, T, H, st)
    torch.cuda.synchronize()
    return rc, X, Y, ldx, ldy


def _want_rows(words, B, T, Hv, col_off, ld, sent):
    body = np.full((T * B + SPARE_ROWS, ld), sent, dtype=words.dtype)
    body[:T * B] = L.rows_from_h(words, Hv, col_off, ld, sent)
    return body.reshape(-1)


@pytest.mark.parametrize("B,T,H", SHAPES)
def test_relayout_dt_exact(mta, B, T, H):
    """X[(t B + b) ldx + col_off + d Hv + j]: the f16 bits themselves (f16) or their round-to-nearest-even bf16 (torch's cast); Y the float
    value; units >= Hv are dropped; every other column and every row >= T B keeps its sentinel.  (Hv, col_off) reach the 16-byte path (aligned
    columns, whole 8-unit pieces), the per-element path (col_off = 5, Hv = H - 3: the reverse direction starts off a multiple of 8) and Hv = 1"""
    lib, st = _lib()
    bits, hx = _case(B, T, H)
    as_bf16 = torch.from_numpy(bits.view(np.int16)).view(torch.float16).float().to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(as_bf16, L.bf16_bits_rne(bits))
    f32 = _f32_bits(bits)
    for dt in ("bf16", "f16"):
        xw = as_bf16 if dt == "bf16" else bits
        for Hv, col_off in ((H, 0), (H, 64), (H - 3, 0), (H - 8, 5), (1, 0)):
            for want_x, want_y in ((True, False), (False, True), (True, True)):
                rc, X, Y, ldx, ldy = _relayout(lib, st, hx, B, T, H, Hv, col_off, dt, want_x, want_y)
                _ok(rc)
                what = (dt, Hv, col_off, want_x, want_y)
                if X:
                    assert X.guards_ok() and np.array_equal(X.bits(), _want_rows(xw, B, T, Hv, col_off, ldx, SENT16)), what
                if Y:
                    assert Y.guards_ok() and np.array_equal(Y.bits(), _want_rows(f32, B, T, Hv, col_off, ldy, SENT32)), what
    # the older entry points are the bf16 _dt call
    _, X0, Y0, ldx, ldy = _relayout(lib, st, hx, B, T, H, H - 3, 5, "bf16", True, True)
    rc, X1, Y1, _, _ = _relayout(lib, st, hx, B, T, H, H - 3, 5, "bf16", True, True, entry="ex")
    _ok(rc)
    assert np.array_equal(X0.bits(), X1.bits()) and np.array_equal(Y0.bits(), Y1.bits())
    _, X0, _, ldx, _ = _relayout(lib, st, hx, B, T, H, H, 0, "bf16", True, False)
    rc, X1, _, _, _ = _relayout(lib, st, hx, B, T, H, H, 0, "bf16", True, False, entry="bf16")
    _ok(rc)
    assert np.array_equal(X0.bits(), X1.bits()) and X1.guards_ok()
    # leading dimensions
    for ldx_bad in (2 * H + 4, 2 * H - 8):
        rc, X, _, _, _ = _relayout(lib, st, hx, B, T, H, H, 0, "bf16", True, False, ldx=ldx_bad)
        assert rc == MT_EINVAL and X.untouched()
    rc, _, Y, _, _ = _relayout(lib, st, hx, B, T, H, H, 0, "bf16", False, True, ldy=2 * H - 1)
    assert rc == MT_EINVAL and Y.untouched()


# ================================================================== mt_lstm_relayout_train, mt_lstm_dh_relayout
def _relayout_train(lib, st, hx, B, T, H, Hv, p, seed, layer, ldx):
    X = _Out((T * B + SPARE_ROWS) * ldx, 2)
    _ok(lib.mt_lstm_relayout_train(hx.data_ptr(), X.ptr, ldx, B, T, H, Hv, p, seed, layer, st))
    torch.cuda.synchronize()
    assert X.guards_ok()
    return X.bits()


def _dh_relayout(lib, st, a, B, T, H, Hv, p, seed, layer):
    """a [B][T][2][Hv] f32 -> the dh image as uint32 bits; dX has ld = 2 Hv + 5 with NaN in the pad columns"""
    ld = 2 * Hv + 5
    dX = L.rows_from_h(np.ascontiguousarray(a, dtype=np.float32), Hv, 0, ld, np.float32(np.nan))
    dXd = _dev(dX)
    dh = _Out(L.cell_words(B, T, H), 4)
    _ok(lib.mt_lstm_dh_relayout(dXd.data_ptr(), ld, dh.ptr, B, T, H, Hv, p, seed, layer, st))
    torch.cuda.synchronize()
    assert dh.guards_ok()
    return dh.bits()


@pytest.mark.parametrize("B,T,H", SHAPES)
def test_relayout_train_and_dh_relayout(mta, B, T, H):
    lib, st = _lib()
    bits, hx = _case(B, T, H)
    as_bf16 = L.bf16_bits_rne(bits)
    h32 = bits.view(np.float16).astype(np.float32)
    scale = np.float32(1) / (np.float32(1) - np.float32(0.3))
    for Hv in (H, H - 3):
        ldx = _roundup(2 * Hv, 8) + 8
        # p = 0: the bf16 re-layout at col_off 0
        got = _relayout_train(lib, st, hx, B, T, H, Hv, 0.0, 5, 1, ldx)
        assert np.array_equal(got, _want_rows(as_bf16, B, T, Hv, 0, ldx, SENT16)), Hv
        # p = 0.3: every element is 0 or bf16(h / (1 - p)); the kept set is the one mt_lstm_dh_relayout regenerates from (seed, layer)
        masks = []
        for layer in (1, 2):
            got = _relayout_train(lib, st, hx, B, T, H, Hv, 0.3, 5, layer, ldx).reshape(T * B + SPARE_ROWS, ldx)
            assert (got[T * B:] == SENT16).all() and (got[:, 2 * Hv:] == SENT16).all()
            x = np.stack([got[:T * B, d * Hv:(d + 1) * Hv].reshape(T, B, Hv).transpose(1, 0, 2) for d in range(2)], axis=2)      # [B][T][2][Hv]
            full = L.bf16_bits_rne_f32(h32[..., :Hv] * scale)
            kept_x = (x & 0x7FFF) != 0
            assert (np.where(kept_x, x == full, True)).all(), "a kept element is not bf16(h / (1 - p))"
            ones = np.ones((B, T, 2, Hv), dtype=np.float32)
            dh = L.decode_cell(_dh_relayout(lib, st, ones, B, T, H, Hv, 0.3, 5, layer), B, T, H)
            kept_dh = dh[..., :Hv] != 0
            assert set(np.unique(dh[..., :Hv]).tolist()) <= {0, int(scale.view(np.uint32))} and (dh[..., Hv:] == 0).all()
            nonzero = (full & 0x7FFF) != 0                                    # (+-0 among the inputs says nothing about its mask bit)
            assert np.array_equal(kept_x[nonzero], kept_dh[nonzero]), (Hv, layer)
            if kept_dh.size >= 64:
                assert 0.5 < kept_dh.mean() < 0.9
            masks.append(kept_dh)
        if masks[0].size >= 64:
            assert not np.array_equal(masks[0], masks[1]), "the mask does not depend on the layer"
        # p = 0: dh == encode_cell(dX), with zeros at units >= Hv and batch slots >= B
        a = np.zeros((B, T, 2, H), dtype=np.float32)
        a[..., :Hv] = h32[..., :Hv] + np.float32(0.5)
        want = L.encode_cell(a, 0.0).view(np.uint32)
        assert np.array_equal(_dh_relayout(lib, st, a[..., :Hv], B, T, H, Hv, 0.0, 5, 1), want), Hv


# ================================================================== mt_lstm_hprev_t
@pytest.mark.parametrize("B,T,H", SHAPES + [(8, 1, 32)])
def test_hprev_t_exact(mta, B, T, H):
    """HT[(d rows_per_dir + k) ld + t B + b] == bf16(h of step t - 1 (forward) / t + 1 (reverse)), exactly 0 at the sequence boundary (all of
    it when T = 1); rows [H, rows_per_dir) and columns >= T B keep the sentinel.  ld a multiple of 8 with B a multiple of 8 takes the 16-byte
    path, anything else the per-element path"""
    lib, st = _lib()
    bits, hx = _case(B, T, H)
    as_bf16 = L.bf16_bits_rne(bits)
    rpd = H + 16
    for ld in (_roundup(T * B, 8) + 8, T * B + 3):
        want = np.full((2, rpd, ld), SENT16, dtype=np.uint16)
        prev = np.zeros((B, T, 2, H), dtype=np.uint16)
        prev[:, 1:, 0] = as_bf16[:, :-1, 0]
        prev[:, :-1, 1] = as_bf16[:, 1:, 1]
        want[:, :H, :T * B] = prev.transpose(2, 3, 1, 0).reshape(2, H, T * B)                 # [d][k][t B + b]
        HT = _Out(2 * rpd * ld, 2)
        _ok(lib.mt_lstm_hprev_t(hx.data_ptr(), HT.ptr, ld, rpd, B, T, H, st))
        torch.cuda.synchronize()
        assert HT.guards_ok() and np.array_equal(HT.bits(), want.reshape(-1)), ld
        if T == 1:
            assert (HT.bits().reshape(2, rpd, ld)[:, :H, :B] == 0).all()


# ================================================================== mt_lstm_dg_unpack
def _dg_unpack(lib, st, dgx, B, T, H, ldg, ldt, want_g, want_t):
    rows_g, rows_t = T * B + SPARE_ROWS, 8 * H + SPARE_ROWS
    dG = _Out(rows_g * ldg, 2) if want_g else None
    dGT = _Out(rows_t * ldt, 2) if want_t else None
    _ok(lib.mt_lstm_dg_unpack(dgx.data_ptr(), dG.ptr if dG else None, ldg, dGT.ptr if dGT else None, ldt, B, T, H, st))
    torch.cuda.synchronize()
    for o in (dG, dGT):
        assert o is None or o.guards_ok()
    return (dG.bits().reshape(rows_g, ldg) if dG else None), (dGT.bits().reshape(rows_t, ldt) if dGT else None)


@pytest.mark.parametrize("B,T,H", [(1, 3, 16), (5, 2, 48), (16, 2, 96), (33, 2, 272), (40, 1, 16)])
def test_dg_unpack_exact(mta, B, T, H):
    """dG[(t B + b) ldg + d 4H + p H + j] and dGT[(d 4H + p H + j) ldt + t B + b] are the bf16 words of the dgx image, bit for bit; the dG-only and
    dGT-only calls (how training calls it) write what the both-outputs call writes; columns >= 8H / >= T B and the spare rows keep their sentinel.
    ldg = 8H takes the 16-byte pieces (H = 16, 48, 272: a last workgroup with 16 of its 32 units live), ldg = 8H + 4 the per-element path; ldt a
    multiple of 8 the 16-byte columns when B is a multiple of 8 (B = 16; B = 40: a ragged second group of 8), odd ldt the per-element path"""
    lib, st = _lib()
    bits = L.distinct_f16_bits((B, T, 2, 4, H), 500 + B + 7 * T + H)                # any 16-bit patterns: the kernel only moves them
    dgx = _dev(R.encode_dgx(bits, PAD16))
    want_g = bits.transpose(1, 0, 2, 3, 4).reshape(T * B, 8 * H)                     # row t B + b, column d 4H + p H + j
    for ldg in (8 * H, 8 * H + 4):
        for ldt in (_roundup(T * B, 8) + 8, T * B + 3):
            full_g = np.full((T * B + SPARE_ROWS, ldg), SENT16, dtype=np.uint16)
            full_g[:T * B, :8 * H] = want_g
            full_t = np.full((8 * H + SPARE_ROWS, ldt), SENT16, dtype=np.uint16)
            full_t[:8 * H, :T * B] = want_g.T
            dG, dGT = _dg_unpack(lib, st, dgx, B, T, H, ldg, ldt, True, True)
            assert np.array_equal(dG, full_g) and np.array_equal(dGT, full_t), (ldg, ldt)
            only_g, none_t = _dg_unpack(lib, st, dgx, B, T, H, ldg, ldt, True, False)
            none_g, only_t = _dg_unpack(lib, st, dgx, B, T, H, ldg, ldt, False, True)
            assert none_t is None and none_g is None and np.array_equal(only_g, dG) and np.array_equal(only_t, dGT), (ldg, ldt)
