"""The weight-gradient and BatchNorm-activation kernels and the training helpers, one by one through the C ABI against float64 / exact references.

  mt_conv_wgrad_ws_bytes                    == the restated cw_plan; 0 for unsupported shapes
  mt_conv_wgrad (24 instantiations)         EXACT (==) on integer operands, twice bit-identical, NaN-filled workspace; one random-bf16 case within
                                            n_acc u sum|products| of float64; refusals leave every output untouched
  mt_conv2_wgrad + mt_sum_slices_f32        EXACT (==), n_wg in {1, 3, 256}; idle workgroups write zero partials
  mt_bn_act_fwd                             EXACT (== the bf16 rounding of float64), rounding case on bf16 ties, one case beyond the 8192-workgroup cap
  mt_bn_act_bwd                             sums / dgamma / dbeta EXACT (==) on integer data; on real data within R.dz_tolerance's bounds;
                                            dz_hi within tol_dz + 2^-8 |dz|, dz_hi + dz_lo within tol_dz + 2^-16 |dz| of the float64 closed form,
                                            dz_hi a nearest bf16 of the sum, the sum closer than dz_hi alone by W.lo_gain; twice: dz bit-identical,
                                            sums within 2 ulp (f64), parameter gradients within 1 ulp (f32); one case beyond the 2048-workgroup cap
  mt_transpose_bf16, mt_gather4_f32, mt_sum_slices_f32, mt_pack_wih_cf, mt_pack_jobs      EXACT (==)

Inputs and references come from tests/wgrad_bn_ref.py (CPU only; tests/test_wgrad_bn_ref_cpu.py checks them, and that every subtle fault it lists
would be caught, without a GPU).  Harness as in tests/test_gpu_conv.py and tests/test_gpu_train_cnn.py: every output and the workspace lie in a
sentinel-filled buffer (the 4- and 8-byte sentinels are NaNs) between two guard bands, and everything that is not a logical element must still
hold the sentinel afterwards; every input is sized exactly between NaN bands; pad channels of wide pitches hold NaN or +-Inf.  Every test prints
the figure it asserts (`-s` shows them).

Share of each derived bound used in the measured run on one MI355X (113 cases, every `==` with 0 differing elements):
  mt_conv_wgrad random bf16: 6.4e-4 of n_acc u sum|products| (n_acc = 1168; median relative error 8.3e-8)
  mt_bn_act_bwd dz_hi: 0.85 .. 0.995 of tol_dz + 2^-8 |dz| (the bf16 rounding itself reaches its bound);  dz_hi + dz_lo: 0.35 .. 0.48 of its bound
  mt_bn_act_bwd gain of the second piece: 765 .. 803 measured, 25.6 .. 29.6 required (W.lo_gain);  the f32 restatement of the closed form on the
  CPU uses 0.28 of tol_dz (tests/test_wgrad_bn_ref_cpu.py); no bound was widened
  mt_bn_act_bwd dgamma: 0.03 .. 0.12 of its tolerance, dbeta: 0 .. 0.023;  two calls: sums, dgamma, dbeta 0 ulp apart, dz bit-identical

Run only this file:  python -m pytest tests/test_gpu_wgrad_bn.py -q -m gpu
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_bn_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1024
NAN, INF = float("nan"), float("inf")
F64 = torch.float64
BF, F32 = torch.bfloat16, torch.float32
U32, UB16 = W.U32, W.UB16
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_SENT = {2: 0x7BCD, 4: 0x7FC0BEEF, 8: 0x7FF8DEADBEEF1234}      # bf16 2e36; an f32 NaN; an f64 NaN
MT_EINVAL, MT_EWORKSPACE, MT_EUNSUPPORTED = -1, -2, -4


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


def _in(body, dtype, off=0):
    """`body` on the device between two NaN bands, sized exactly -> (owner, address); off: shift by that many elements (misalignment)"""
    g = torch.full((GUARD + off,), NAN, dtype=F64)
    full = torch.cat([g, body.reshape(-1).to(F64), g[:GUARD]]).to(dtype).cuda()
    return full, full.data_ptr() + (GUARD + off) * full.element_size()


class _Out:
    """n elements between two guard bands, all of it pre-filled with a sentinel; the checks run on the device (large buffers stay there)"""

    def __init__(self, n, dtype):
        self.n, self.dtype, self.size = n, dtype, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + n,), _SENT[self.size], dtype=_INT[self.size], device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.size

    def dev(self):
        return self.buf[GUARD:GUARD + self.n].view(self.dtype)

    def body(self):
        return self.dev().cpu()

    def untouched(self):
        return bool((self.buf == _SENT[self.size]).all().item())

    def guards_ok(self):
        return bool((self.buf[:GUARD] == _SENT[self.size]).all().item()) and bool((self.buf[GUARD + self.n:] == _SENT[self.size]).all().item())

    def rest_untouched(self, idx=None):
        """everything but the logical elements idx (positions in the body; None: the whole body) still holds the sentinel"""
        if idx is None:
            return self.guards_ok()
        pos = torch.as_tensor(np.ascontiguousarray(idx)).reshape(-1).cuda()
        assert int(pos.min()) >= 0 and int(pos.max()) < self.n
        other = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        other[pos + GUARD] = False
        assert int((~other).sum()) == pos.numel(), "the layout maps two logical elements to one slot"
        return bool((self.buf[other] == _SENT[self.size]).all().item())


def _say(what, **figs):
    print(f"MEASURED {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _pitched(v, pitch):
    """[..., C] -> flat [positions][pitch] with NaN / +Inf / -Inf in the pad channels, cut right behind the last logical element"""
    C = v.shape[-1]
    body = torch.full((v.numel() // C, pitch), NAN, dtype=F64)
    body[:, C + 1::3] = INF
    body[:, C + 2::3] = -INF
    body[:, :C] = v.reshape(-1, C)
    return body.reshape(-1)[:(body.shape[0] - 1) * pitch + C]


def _cl_index(npos, C, pitch):
    p, c = np.ogrid[:npos, :C]
    return p * pitch + c


def _x_index(B, Fo, T, C, ld):
    b, f, t, c = np.ogrid[:B, :Fo, :T, :C]
    return (t * B + b) * ld + f * C + c


def _first_bad(got, want):
    bad = torch.nonzero(~(got == want))
    return "" if bad.numel() == 0 else (f"{bad.shape[0]} of {got.numel()} differ; first at {tuple(bad[0].tolist())}: got {got[tuple(bad[0])].item()!r}, "
                                        f"want {want[tuple(bad[0])].item()!r}")


# ------------------------------------------------------------------ 1. mt_conv_wgrad
def _cw_call(P, dz_pad=0, x_pad=0, twice=True):
    lib, st = _lib()
    dp, xp = P.Cout + dz_pad, P.Cin + x_pad
    ohi, phi = _in(_pitched(P.hi, dp), BF)
    olo, plo = _in(_pitched(P.lo, dp), BF) if P.lo is not None else (None, None)
    ox, px = _in(_pitched(P.x, xp), BF)
    dims = (P.B, P.F, P.T, P.Cout, P.Cin, P.KH, P.KW)
    nws = lib.mt_conv_wgrad_ws_bytes(*dims)
    assert nws == W.cw_ws_bytes(*dims) and nws > 0
    outs = []
    for _ in range(2 if twice else 1):
        ws, out = _Out(nws // 4, F32), _Out(P.Cout * P.Cin * P.KH * P.KW, F32)          # the workspace starts as NaN
        _ok(lib.mt_conv_wgrad(phi, plo, dp, px, xp, *dims[:3], P.Cout, P.Cin, P.KH, P.KW, ws.ptr, nws, out.ptr, st))
        torch.cuda.synchronize()
        assert ws.guards_ok() and out.guards_ok(), "a guard band of the workspace or of dW was written"
        outs.append(out.body())
    if twice:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two calls differ"
    return outs[0].reshape(P.Cout, P.Cin, P.KH, P.KW)


@pytest.mark.parametrize("Cout,Cin", W.CW_TILINGS)
@pytest.mark.parametrize("B,F,T,KH,edge", W.CW_SHAPES)
def test_conv_wgrad_exact(mta, B, F, T, KH, edge, Cout, Cin):
    """dW == the integer reference for KW in {3, 1} x {two pieces, dz_lo = NULL}: with every tiling, all 24 instantiations.  dz_lo is an
    independent integer tensor; the borders of every chunk carry x16 values (a halo that leaves the chunk or wraps to the next frequency row
    would show); both pitches are wider than the channel counts with NaN / Inf behind the channels."""
    for KW in (3, 1):
        for lo in (True, False):
            P = W.conv_wgrad_case(B, F, T, Cout, Cin, KH, KW, lo=lo, edge=edge)
            W.assert_conv_wgrad_case(P)
            assert P.plan == W.cw_plan(Cout, Cin, KH, W.cw_tiles_max(B, F, T))
            got = _cw_call(P, dz_pad=8, x_pad=16).to(F64)
            msg = _first_bad(got, P.ref)
            _say(f"conv_wgrad {B}x{F}x{T} {Cout}x{Cin} KH={KH} KW={KW} lo={lo}", plan=P.plan, units=P.units, differing=int((got != P.ref).sum()))
            assert not msg, msg


@pytest.mark.parametrize("name", list(W.CW_SPLIT_CASES))
def test_conv_wgrad_k_split_exact(mta, name):
    """empty splits (fewer than 8 tiles), S at its shape-independent maximum, and a workgroup with at least 3 consecutive tiles"""
    P = W.conv_wgrad_case(*W.CW_SPLIT_CASES[name])
    W.assert_conv_wgrad_case(P)
    W.assert_cw_split_case(name, P)
    got = _cw_call(P).to(F64)
    msg = _first_bad(got, P.ref)
    _say(f"conv_wgrad split case {name}", plan=P.plan, tiles_per_wg=W.cw_max_tiles_per_workgroup(P.B, P.F, P.T, P.KH, P.S),
         empty=W.cw_empty_splits(P.B, P.F, P.T, P.KH, P.S), differing=int((got != P.ref).sum()))
    assert not msg, msg


def test_conv_wgrad_random_bf16_within_the_accumulation_bound(mta):
    P = W.conv_wgrad_rounding_case()
    got = _cw_call(P, dz_pad=8).to(F64)
    used = float(((got - P.ref).abs() / P.tol).max())
    _say("conv_wgrad random bf16", n_acc=P.n_acc, used_of_bound=used, max_rel_err=float(((got - P.ref).abs() / (P.ref.abs() + 1e-30)).median()))
    assert used <= 1


def test_conv_wgrad_refusals_leave_the_outputs_untouched(mta):
    lib, st = _lib()
    P = W.conv_wgrad_case(2, 3, 5, 64, 32, 3, 3)
    ohi, phi = _in(_pitched(P.hi, 72), BF)
    olo, plo = _in(_pitched(P.lo, 72), BF)
    ox, px = _in(_pitched(P.x, 40), BF)
    nws = lib.mt_conv_wgrad_ws_bytes(2, 3, 5, 64, 32, 3, 3)
    ws, out = _Out(nws // 4, F32), _Out(64 * 32 * 9, F32)

    def call(hi=phi, lo=plo, dp=72, x=px, xp=40, Cout=64, Cin=32, KH=3, KW=3, nb=nws):
        return lib.mt_conv_wgrad(hi, lo, dp, x, xp, 2, 3, 5, Cout, Cin, KH, KW, ws.ptr, nb, out.ptr, st)
    bad = {"Cout=96": call(Cout=96, dp=96), "Cin=48": call(Cin=48, xp=48), "KH=2": call(KH=2), "KW=2": call(KW=2), "dz_pitch=68": call(dp=68),
           "x_pitch=36": call(xp=36), "dz_hi+2B": call(hi=phi + 2), "dz_lo+2B": call(lo=plo + 2), "x+2B": call(x=px + 2)}
    short = call(nb=nws - 1)
    torch.cuda.synchronize()
    _say("conv_wgrad refusals", **bad, ws_short=short)
    assert all(rc < 0 for rc in bad.values()) and short == MT_EWORKSPACE
    assert ws.untouched() and out.untouched()
    for dims in ((2, 3, 5, 96, 32, 3, 3), (2, 3, 5, 64, 48, 3, 3), (2, 3, 5, 64, 32, 3, 2), (2, 3, 5, 0, 32, 3, 3)):
        assert lib.mt_conv_wgrad_ws_bytes(*dims) == 0 == W.cw_ws_bytes(*dims)
    _ok(call())                                                         # and the same arguments, untampered, are accepted
    torch.cuda.synchronize()
    assert not _first_bad(out.body().reshape(64, 32, 3, 3).to(F64), P.ref)


# ------------------------------------------------------------------ 2. mt_conv2_wgrad + mt_sum_slices_f32
@pytest.mark.parametrize("n_wg", W.CONV2_NWG)
@pytest.mark.parametrize("B,F,T", W.CONV2_SHAPES)
def test_conv2_wgrad_exact(mta, B, F, T, n_wg):
    """n_wg = 1: one workgroup walks every tile with its accumulators carried across; 3: unequal tile counts; 256: idle workgroups, which must
    write zero partials into the NaN-filled P / Pb.  dW over hi + lo and db over hi alone == the integer reference after mt_sum_slices_f32."""
    lib, st = _lib()
    P = W.conv2_wgrad_case(B, F, T)
    W.assert_exact(P.units, "mt_conv2_wgrad")
    (oa, pa), (oh, ph), (ol, pl) = _in(P.a1, BF), _in(P.hi, BF), _in(P.lo, BF)
    Pp, Pb = _Out(n_wg * 64 * 288, F32), _Out(n_wg * 64, F32)
    _ok(lib.mt_conv2_wgrad(pa, ph, pl, Pp.ptr, Pb.ptr, n_wg, B, F, T, st))
    dW, db = _Out(64 * 288, F32), _Out(64, F32)
    _ok(lib.mt_sum_slices_f32(Pp.ptr, 64 * 288, 288, n_wg, dW.ptr, 288, 64, 288, st))
    _ok(lib.mt_sum_slices_f32(Pb.ptr, 64, 64, n_wg, db.ptr, 64, 1, 64, st))
    torch.cuda.synchronize()
    nt = W.conv2_tiles(B, F, T)
    part = Pp.body().reshape(n_wg, 64 * 288)
    idle = part[min(nt, n_wg):]
    assert bool((idle == 0).all()) and bool((Pb.body().reshape(n_wg, 64)[min(nt, n_wg):] == 0).all()), "an idle workgroup left no zero partial"
    got, gotb = W.conv2_from_partials(dW.body().to(F64)), db.body().to(F64)
    _say(f"conv2_wgrad {B}x{F}x{T} n_wg={n_wg}", tiles=nt, units=P.units, dW_differing=int((got != P.dW).sum()), db_differing=int((gotb != P.db).sum()))
    msg = _first_bad(got, P.dW)
    assert not msg, msg
    assert torch.equal(gotb, P.db), "db differs (it is the sum of the hi piece alone)"
    for o in (Pp, Pb, dW, db):
        assert o.guards_ok()


# ------------------------------------------------------------------ 3. mt_bn_act_fwd
def _bn_fwd_call(P, out_mode):
    lib, st = _lib()
    B, F, T, C, Fo = P.B, P.F, P.T, P.C, P.Fo
    oza, pza = _in(P.za, BF)
    ozb, pzb = _in(P.zb, BF) if P.zb is not None else (None, None)
    pa = [_in(v, F32) for v in P.pa]
    pb = [_in(v, F32) for v in P.pb] if P.zb is not None else [(None, None)] * 4
    om, pm = _in(P.mask, F32) if P.mask is not None else (None, None)
    ldx = Fo * C + 8 if out_mode else 0
    out = _Out(T * B * ldx if out_mode else B * Fo * T * C, BF)
    _ok(lib.mt_bn_act_fwd(pza, *[p[1] for p in pa], pzb, *[p[1] for p in pb], pm, out.ptr, out_mode, ldx, B, F, T, C, P.relu, P.pool, st))
    torch.cuda.synchronize()
    if out_mode:
        idx = _x_index(B, Fo, T, C, ldx)
        got = out.body()[torch.from_numpy(idx.reshape(-1))].reshape(B, Fo, T, C)
        assert out.rest_untouched(idx), "pad columns of X or a guard band were written"
    else:
        got = out.body().reshape(B, Fo, T, C)
        assert out.guards_ok()
    return got


@pytest.mark.parametrize("B,F,T,C,two,relu,pool,mask,out_mode", W.BN_FWD_CASES)
def test_bn_act_fwd_exact(mta, B, F, T, C, two, relu, pool, mask, out_mode):
    """out == float64's result (itself a bf16 value: asserted), element for element.  The row an odd F drops under pool holds NaN."""
    P = W.bn_fwd_case(B, F, T, C, two, relu, pool, mask)
    W.assert_bn_fwd_exact(P)
    assert W.bn_fwd_grid(B, F, T, C, pool)[0] == B * P.Fo * T
    got = _bn_fwd_call(P, out_mode)
    want = P.ref.float().to(BF)
    _say(f"bn_act_fwd {B}x{F}x{T}x{C} two={two} relu={relu} pool={pool} mask={mask} mode={out_mode}", differing=int((~(got == want)).sum()))
    msg = _first_bad(got, want)
    assert not msg, msg


@pytest.mark.parametrize("C,pool,out_mode", [(32, 1, 0), (256, 0, 1), (64, 1, 1)])
def test_bn_act_fwd_rounds_to_nearest_even(mta, C, pool, out_mode):
    P = W.bn_fwd_case(2, 5, 9, C, False, 1, pool, True, ties=True)
    W.assert_bn_fwd_exact(P)
    got = _bn_fwd_call(P, out_mode)
    want = P.ref.float().to(BF)
    _say(f"bn_act_fwd ties C={C} pool={pool}", differing=int((~(got == want)).sum()))
    msg = _first_bad(got, want)
    assert not msg, msg


def test_bn_act_fwd_beyond_the_workgroup_cap(mta):
    """132117 positions at C = 256: 8192 workgroups, a second loop trip whose second position is out of range (W.bn_fwd_cap_case)"""
    lib, st = _lib()
    P = W.bn_fwd_cap_case()
    g = torch.full((GUARD,), NAN).to(BF)
    full = torch.cat([g, P.z.reshape(-1).to(BF), g]).cuda()
    par = [_in(v, F32) for v in P.p]
    out = _Out(P.z.numel(), BF)
    _ok(lib.mt_bn_act_fwd(full.data_ptr() + 2 * GUARD, *[p[1] for p in par], None, None, None, None, None, None, out.ptr, 0, 0,
                          P.B, P.F, P.T, P.C, 1, 0, st))
    torch.cuda.synchronize()
    want = P.ref.reshape(-1).to(BF).cuda()
    differing = int((~(out.dev() == want)).sum().item())
    _say("bn_act_fwd cap case", positions=P.B * P.F * P.T, differing=differing)
    assert differing == 0 and out.guards_ok()


# ------------------------------------------------------------------ 4. mt_bn_act_bwd
def _bn_bwd_call(P, src, lo=True):
    """-> dict of outputs; pitch_a = C + 8, pitch_b = C + 16, ldd_cl = C + 8, ldd_x = Fo C + 4; every pad column must keep the sentinel"""
    lib, st = _lib()
    B, F, T, C, Fo = P.B, P.F, P.T, P.C, P.Fo
    two = P.zb is not None
    oza, pza = _in(P.za, BF)
    ozb, pzb = _in(P.zb, BF) if two else (None, None)
    pa = [_in(v.float(), F32) for v in P.pa]
    pb = [_in(v.float(), F32) for v in P.pb] if two else [(None, None)] * 4
    om, pm = _in(P.mask, F32) if P.mask is not None else (None, None)
    ldd_cl, ldd_x = C + 8, Fo * C + 4
    if src == "cl":
        og, pg = _in(_pitched(P.g, ldd_cl), BF)
        gcl, gx = pg, None
    else:
        body = torch.full((T * B, ldd_x), NAN, dtype=F64)
        body[:, :Fo * C] = P.g.permute(2, 0, 1, 3).reshape(T * B, Fo * C)
        og, pg = _in(body.reshape(-1)[:(T * B - 1) * ldd_x + Fo * C], F32)
        gcl, gx = None, pg
    npos, pit = B * F * T, (C + 8, C + 16)
    o = {"sums": _Out(3 * C, F64), "dza": _Out(npos * pit[0], BF), "dza_lo": _Out(npos * pit[0], BF), "dzb": _Out(npos * pit[1], BF),
         "dzb_lo": _Out(npos * pit[1], BF), "dga": _Out(C, F32), "dba": _Out(C, F32), "dgb": _Out(C, F32), "dbb": _Out(C, F32)}
    q = lambda k, on=True: o[k].ptr if on else None
    _ok(lib.mt_bn_act_bwd(gcl, ldd_cl, gx, ldd_x, pza, *[p[1] for p in pa], pzb, *[p[1] for p in pb], pm, q("sums"), q("dza"), pit[0],
                          q("dza_lo", lo), q("dzb", two), pit[1], q("dzb_lo", two and lo), q("dga"), q("dba"), q("dgb", two), q("dbb", two),
                          B, F, T, C, P.relu, P.pool, st))
    torch.cuda.synchronize()
    res = {}
    for k, written in (("dza", True), ("dza_lo", lo), ("dzb", two), ("dzb_lo", two and lo)):
        p_ = pit[0] if k.startswith("dza") else pit[1]
        if written:
            idx = _cl_index(npos, C, p_)
            assert o[k].rest_untouched(idx), f"{k}: pad columns or a guard band were written"
            res[k] = o[k].body()[torch.from_numpy(idx.reshape(-1))].reshape(B, F, T, C)
        else:
            assert o[k].untouched(), f"{k} must not be written"
            res[k] = None
    for k, written in (("sums", True), ("dga", True), ("dba", True), ("dgb", two), ("dbb", two)):
        assert o[k].guards_ok() if written else o[k].untouched()
        res[k] = o[k].body() if written else None
    return res


def _check_bn_bwd(P, r, what):
    """see the header and W.bn_bwd_tolerances / hi_bound / sum_bound / lo_gain for the bounds"""
    C = P.C
    tols = W.bn_bwd_tolerances(P)
    figs = {}
    fails = []
    refs = {"a": P.cf.a, "b": P.cf.b}
    for br, tol in zip("ab", tols):
        v = refs[br]
        if v is None:
            continue
        t_dz, t_dg, t_db = tol
        hi = r["dz" + br].to(F64)
        figs[f"dz{br}_hi/bound"] = float(((hi - v.dz).abs() / (W.hi_bound(v.dz, t_dz) + 1e-300)).max())
        lo = r[f"dz{br}_lo"]
        if lo is not None:
            s = hi + lo.to(F64)
            figs[f"dz{br}_sum/bound"] = float(((s - v.dz).abs() / (W.sum_bound(v.dz, t_dz) + 1e-300)).max())
            if not bool(((s - hi).abs() <= (s - W.bf16_round(s)).abs()).all()):
                fails.append(f"dz{br}_hi is not a bf16 value nearest to hi + lo")
            if not P.exact:
                gain = float((hi - v.dz).abs().sum() / ((s - v.dz).abs().sum() + 1e-300))
                figs[f"dz{br}_gain"], figs[f"dz{br}_gain_required"] = gain, W.lo_gain(v.dz, t_dz)
                if gain < figs[f"dz{br}_gain_required"]:
                    fails.append(f"dz{br}: hi + lo is not closer than hi alone by the derived ratio")
        dg, db = r["dg" + br].to(F64), r["db" + br].to(F64)
        if P.exact:
            figs[f"dgamma_{br}_differing"] = int((dg != v.dgamma).sum())
            figs[f"dbeta_{br}_differing"] = int((db != v.dbeta).sum())
        else:
            figs[f"dgamma_{br}/tol"] = float(((dg - v.dgamma).abs() / (t_dg + U32 * v.dgamma.abs() + 1e-300)).max())
            figs[f"dbeta_{br}/tol"] = float(((db - v.dbeta).abs() / (t_db + U32 * v.dbeta.abs() + 1e-300)).max())
    want_sums = torch.cat([P.cf.dbeta, P.cf.a.dgamma, P.cf.b.dgamma if P.cf.b is not None else torch.zeros(C, dtype=F64)])
    if P.exact:
        figs["sums_differing"] = int((r["sums"] != want_sums).sum())
    else:
        assert bool((r["sums"][2 * C:] == 0).all()) or P.cf.b is not None
    _say(what, **figs)
    assert not fails, f"{what}: {fails}"
    for k, v in figs.items():
        if k.endswith("/bound") or k.endswith("/tol"):
            assert v <= 1, f"{what}: {k} = {v:.3g}"
        if k.endswith("_differing"):
            assert v == 0, f"{what}: {k} = {v}"


def _ulps(a, b, dtype):
    a, b = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    sp = np.spacing(np.abs(b).astype(dtype)).astype(np.float64)
    return float((np.abs(a - b) / sp).max())


@pytest.mark.parametrize("case", W.BN_BWD_CASES)
def test_bn_act_bwd_integer_data_parameter_gradients_exact(mta, case):
    B, F, T, C, two, relu, pool, mask, src = case
    P = W.bn_bwd_int_case(B, F, T, C, two, relu, pool, mask)
    W.assert_bn_bwd_int_case(P)
    _check_bn_bwd(P, _bn_bwd_call(P, src), f"bn_act_bwd int {case}")


@pytest.mark.parametrize("case", W.BN_BWD_CASES)
def test_bn_act_bwd_real_data_within_the_derived_bounds(mta, case):
    B, F, T, C, two, relu, pool, mask, src = case
    P = W.bn_bwd_real_case(B, F, T, C, two, relu, pool, mask)
    W.assert_bn_bwd_real_case(P)
    r = _bn_bwd_call(P, src)
    _check_bn_bwd(P, r, f"bn_act_bwd real {case}")
    # dz_lo = NULL: the first piece alone, unchanged; and a second call agrees
    r2 = _bn_bwd_call(P, src, lo=False)
    for k in ("dza", "dzb"):
        if r[k] is not None:
            assert torch.equal(r[k].view(torch.int16), r2[k].view(torch.int16)), f"{k} differs between two calls"
    figs = {"sums_ulp": _ulps(r2["sums"], r["sums"], np.float64)}
    for k in ("dga", "dba", "dgb", "dbb"):
        if r[k] is not None:
            figs[k + "_ulp"] = _ulps(r2[k], r[k], np.float32)
    _say(f"bn_act_bwd twice {case}", **figs)
    assert figs.pop("sums_ulp") <= 2 and all(v <= 1 for v in figs.values())


def test_bn_act_bwd_beyond_the_workgroup_cap(mta):
    B, F, T, C, two, relu, pool, mask, src = W.BN_BWD_CAP
    n, ppb, g, _ = W.bn_bwd_grid(B, F, T, C, pool)
    assert g == 2048 and n > 2 * g * ppb
    P = W.bn_bwd_int_case(B, F, T, C, two, relu, pool, mask)
    W.assert_bn_bwd_int_case(P)
    _check_bn_bwd(P, _bn_bwd_call(P, src), f"bn_act_bwd cap case, {n} row groups")


def test_bn_act_refusals_leave_the_outputs_untouched(mta):
    lib, st = _lib()
    B, F, T, C = 2, 4, 3, 64
    z = W.randint(torch.Generator().manual_seed(1), -3, 3, (B, F, T, C))
    oz, pz = _in(z, BF)
    par = [_in(torch.ones(C, dtype=F64), F32) for _ in range(4)]
    pp = [p[1] for p in par]
    og, pg = _in(z, BF)
    ogx, pgx = _in(z, F32)
    out, sums, dza, dzb = _Out(B * F * T * C, BF), _Out(3 * C, F64), _Out(B * F * T * C, BF), _Out(B * F * T * C, BF)
    grads = [_Out(C, F32) for _ in range(4)]
    none4 = [None] * 4

    def fwd(C_=C, F_=F, pool=0, zb=None, sb=none4, mode=0, ldx=0):
        return lib.mt_bn_act_fwd(pz, *pp, zb, *sb, None, out.ptr, mode, ldx, B, F_, T, C_, 1, pool, st)

    def bwd(C_=C, F_=F, pool=0, cl=pg, x=None, pa=C, pb=C, zb=None, sb=none4, ldd_cl=C, ldd_x=F * C):
        return lib.mt_bn_act_bwd(cl, ldd_cl, x, ldd_x, pz, *pp, zb, *sb, None, sums.ptr, dza.ptr, pa, None, dzb.ptr, pb, None,
                                 *[g_.ptr for g_ in grads], B, F_, T, C_, 1, pool, st)
    rcs = {"fwd C=48": fwd(C_=48), "fwd pool F=1": fwd(F_=1, pool=1), "fwd ldx%8": fwd(mode=1, ldx=F * C + 4), "fwd zb without stats": fwd(zb=pz),
           "bwd C=48": bwd(C_=48), "bwd pool F=1": bwd(F_=1, pool=1), "bwd both sources": bwd(x=pgx), "bwd no source": bwd(cl=None),
           "bwd pitch_a%8": bwd(pa=C + 4), "bwd pitch_b%8": bwd(zb=pz, sb=pp, pb=C + 4), "bwd ldd_cl%8": bwd(ldd_cl=C + 4),
           "bwd zb without stats": bwd(zb=pz)}
    torch.cuda.synchronize()
    _say("bn_act refusals", **rcs)
    assert all(rc < 0 for rc in rcs.values())
    for o in [out, sums, dza, dzb] + grads:
        assert o.untouched()
    assert fwd() == 0 and bwd() == 0                                    # the untampered arguments are accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. helpers
@pytest.mark.parametrize("R_,C,lds,ldd,Cd,off", [(63, 64, 64, 64, 64, 0), (64, 63, 64, 64, 64, 0), (65, 65, 72, 72, 72, 0), (129, 64, 64, 136, 65, 0),
                                                (127, 9, 16, 128, 16, 0), (64, 65, 65, 64, 65, 0), (65, 63, 64, 67, 64, 0), (63, 64, 64, 64, 64, 3)])
def test_transpose_bf16_exact(mta, R_, C, lds, ldd, Cd, off):
    """the 16-byte kernel (lds, ldd multiples of 8, aligned) and the scalar one (the last three cases: odd lds, odd ldd, a source 6 bytes off)"""
    lib, st = _lib()
    g = torch.Generator().manual_seed(R_ + C)
    src = torch.full((R_, lds), NAN, dtype=F64)
    src[:, :C] = W.randint(g, -100, 100, (R_, C))
    osrc, psrc = _in(src.reshape(-1)[:(R_ - 1) * lds + C], BF, off=off)
    dst = _Out((Cd - 1) * ldd + ldd, BF)
    _ok(lib.mt_transpose_bf16(psrc, lds, R_, C, dst.ptr, ldd, Cd, st))
    torch.cuda.synchronize()
    got = dst.body().reshape(Cd, ldd).to(F64)
    want = W.transpose_ref(torch.nan_to_num(src), R_, C, ldd, Cd)
    msg = _first_bad(got, want)
    _say(f"transpose {R_}x{C} lds={lds} ldd={ldd} Cd={Cd} off={off}", differing=int((got != want).sum()))
    assert not msg, msg
    assert dst.guards_ok()


@pytest.mark.parametrize("n,s,off", [((2, 3, 64, 65), (3 * 4160, 4160, 1, 64), 0), ((1, 2, 63, 64), (8000, 4032, 1, 63), 1), ((2, 5, 7, 3), (200, 30, 1, 7), 0),
                                     ((3, 4, 1, 16), (100, 20, 0, 1), 0), ((2, 2, 65, 63), (9000, 4200, 63, 1), 1)])
def test_gather4_f32_exact(mta, n, s, off):
    """the LDS-transposing kernel (s2 = 1, s3 = n2) and the generic one; alpha = 1/2 on integers: exact"""
    lib, st = _lib()
    need = sum((nk - 1) * sk for nk, sk in zip(n, s)) + 1
    src = W.randint(torch.Generator().manual_seed(need), -1000, 1000, (need,))
    osrc, psrc = _in(src, F32, off=off)
    dst = _Out(int(np.prod(n)), F32)
    _ok(lib.mt_gather4_f32(psrc, dst.ptr, *n, *s, 0.5, st))
    torch.cuda.synchronize()
    got, want = dst.body().reshape(n).to(F64), W.gather4_ref(src, n, s, 0.5)
    _say(f"gather4 {n} {s}", lds_kernel=W.gather4_takes_lds_kernel(n, s), differing=int((got != want).sum()))
    assert torch.equal(got, want) and dst.guards_ok()


@pytest.mark.parametrize("S,rows,cols,ldp,ldo", [(1, 3, 5, 5, 5), (7, 1, 63, 64, 72), (9, 2, 65, 65, 65), (256, 1, 64, 64, 64), (19, 10, 33, 40, 36)])
def test_sum_slices_f32_exact(mta, S, rows, cols, ldp, ldo):
    lib, st = _lib()
    v = W.randint(torch.Generator().manual_seed(S + cols), -1000, 1000, (S, rows, cols))
    body = torch.full((S, rows, ldp), NAN, dtype=F64)
    body[..., :cols] = v
    oP, pP = _in(body.reshape(-1)[:(S * rows - 1) * ldp + cols], F32)
    out = _Out((rows - 1) * ldo + cols, F32)
    _ok(lib.mt_sum_slices_f32(pP, rows * ldp, ldp, S, out.ptr, ldo, rows, cols, st))
    torch.cuda.synchronize()
    r, c = np.ogrid[:rows, :cols]
    idx = r * ldo + c
    got = out.body()[torch.from_numpy(idx.reshape(-1))].reshape(rows, cols).to(F64)
    _say(f"sum_slices S={S} {rows}x{cols}", differing=int((got != v.sum(0)).sum()))
    assert torch.equal(got, v.sum(0)) and out.rest_untouched(idx)


@pytest.mark.parametrize("H,Hp,C,F,dt,row0,pad", [(3, 16, 64, 5, 0, 0, 0), (5, 16, 32, 4, 1, 7, 8), (17, 32, 63, 3, 0, 2, 3)])
def test_pack_wih_cf_exact(mta, H, Hp, C, F, dt, row0, pad):
    """out[(row0 + p Hp + j) ldo + f C + c] = h16(w[(p H + j) C F + c F + f]), rows j >= H zero; rows before row0, columns behind C F and
    everything behind the last row keep the sentinel.  Multiples of 1/4 below 64: exact in bf16 and f16."""
    lib, st = _lib()
    K, ldo = C * F, C * F + pad
    w = W.randint(torch.Generator().manual_seed(H + C), -255, 255, (4 * H, K)) / 4
    ow, pw = _in(w, F32, off=1 if pad else 0)
    nrows = row0 + 4 * Hp
    out = _Out((nrows - 1) * ldo + K, BF)
    _ok(lib.mt_pack_wih_cf(pw, out.ptr, ldo, row0, H, Hp, C, F, dt, st))
    torch.cuda.synchronize()
    r, c = np.ogrid[row0:nrows, :K]
    idx = r * ldo + c
    raw = out.body()[torch.from_numpy(idx.reshape(-1))].reshape(4 * Hp, K)
    got = (raw.view(torch.float16) if dt == 1 else raw).to(F64)
    want = W.pack_wih_ref(w, H, Hp, C, F)
    _say(f"pack_wih_cf H={H} C={C} F={F} dt={dt}", differing=int((got != want).sum()))
    assert torch.equal(got, want) and out.rest_untouched(idx)


JOB_DTYPE = np.dtype([("src", "u8"), ("src2", "u8"), ("dst", "u8"), ("ld", "i8"), ("sr1", "i8"), ("sr2", "i8"), ("sc1", "i8"), ("sc2", "i8"),
                      ("dt", "i4"), ("Rp", "i4"), ("Cp", "i4"), ("Rn2", "i4"), ("R1v", "i4"), ("R2v", "i4"), ("Cn2", "i4"), ("C1v", "i4"),
                      ("C2v", "i4"), ("tr", "i4"), ("tile0", "i4"), ("reserved", "i4")])      # mt_pack_job (include/mt_hip.h)


def test_pack_jobs_exact(mta):
    """one table, four jobs: a padded bf16 copy (63 x 65 valid inside 65 x 70), a transposing f32 job with a second source added, a two-level
    f16 job with a negative stride (a flipped axis) and head padding, and a 1 x 1 job; 33-, 64- and 65-wide tile edges"""
    assert JOB_DTYPE.itemsize == 112
    lib, st = _lib()
    BIG = 1 << 30
    g = torch.Generator().manual_seed(7)
    specs = [dict(dt=0, Rp=65, Cp=70, ld=72, R1v=1, Rn2=BIG, R2v=63, sr1=0, sr2=65, C1v=1, Cn2=BIG, C2v=65, sc1=0, sc2=1, tr=0, n=63 * 65, base=0, two=False),
             dict(dt=2, Rp=33, Cp=64, ld=64, R1v=1, Rn2=BIG, R2v=33, sr1=0, sr2=1, C1v=1, Cn2=BIG, C2v=64, sc1=0, sc2=33, tr=1, n=33 * 64, base=0, two=True),
             dict(dt=1, Rp=3 * 24, Cp=40, ld=48, R1v=3, Rn2=24, R2v=20, sr1=20 * 33, sr2=33, C1v=1, Cn2=BIG, C2v=33, sc1=0, sc2=-1, tr=0, n=60 * 33, base=32, two=False),
             dict(dt=0, Rp=1, Cp=1, ld=8, R1v=1, Rn2=BIG, R2v=1, sr1=0, sr2=1, C1v=1, Cn2=BIG, C2v=1, sc1=0, sc2=1, tr=0, n=1, base=0, two=False)]
    jobs, keep, tile0 = [], [], 0
    for sp in specs:
        src = W.randint(g, -200, 200, (sp["n"],)) / 2
        src2 = W.randint(g, -200, 200, (sp["n"],)) / 2 if sp["two"] else None
        osrc, psrc = _in(src, F32)
        osrc2, psrc2 = _in(src2, F32) if sp["two"] else (None, 0)
        dtype = {0: BF, 1: BF, 2: F32}[sp["dt"]]
        dst = _Out((sp["Rp"] - 1) * sp["ld"] + sp["Cp"], dtype)
        job = np.zeros((), dtype=JOB_DTYPE)
        for k in ("ld", "sr1", "sr2", "sc1", "sc2", "dt", "Rp", "Cp", "Rn2", "R1v", "R2v", "Cn2", "C1v", "C2v", "tr"):
            job[k] = sp[k]
        job["src"], job["src2"], job["dst"], job["tile0"] = psrc + 4 * sp["base"], (psrc2 + 4 * sp["base"]) if sp["two"] else 0, dst.ptr, tile0
        tile0 += ((sp["Rp"] + 31) // 32) * ((sp["Cp"] + 31) // 32)
        jobs.append(job)
        keep.append((osrc, osrc2, dst, src, src2))
    table = torch.from_numpy(np.stack(jobs).view(np.uint8).reshape(-1).copy()).cuda()
    _ok(lib.mt_pack_jobs(table.data_ptr(), len(jobs), tile0, st))
    torch.cuda.synchronize()
    for i, (sp, (_, _, dst, src, src2)) in enumerate(zip(specs, keep)):
        r, c = np.ogrid[:sp["Rp"], :sp["Cp"]]
        idx = r * sp["ld"] + c
        raw = dst.body()[torch.from_numpy(idx.reshape(-1))].reshape(sp["Rp"], sp["Cp"])
        got = (raw.view(torch.float16) if sp["dt"] == 1 else raw).to(F64)
        want = W.pack_job_ref(src[sp["base"]:], src2[sp["base"]:] if src2 is not None else None, sp) if sp["sc2"] >= 0 else \
            W.pack_job_ref(_Shift(src, sp["base"]), None, sp)
        _say(f"pack_jobs job {i}", differing=int((got != want).sum()))
        assert torch.equal(got, want) and dst.rest_untouched(idx)


class _Shift:
    """src viewed from element `base`, negative offsets allowed"""

    def __init__(self, t, base):
        self.t, self.base = t, base

    def __getitem__(self, off):
        assert 0 <= self.base + off < self.t.numel()
        return self.t[self.base + off]
