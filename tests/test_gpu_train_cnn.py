"""The CNN training kernels of csrc/train.hip (and the two dlogits pack kernels), one by one through the C ABI against float64 references.

  mt_conv1_stats, mt_bn_stats_cl, mt_bn_relu_pool_apply, mt_rowsum_bf16, mt_dlogits_pack, mt_dlogits_pack_heads:   EXACT (==)
  mt_bn_finalize:                                       1 ulp (mean, rstd) / 2 ulp (running statistics, folded parameters) of float64
  mt_bn_pool_bwd, mt_bn_pool_bwd_tie, mt_conv1_bwd:     float64 autograd, within bounds derived from u = 2^-24 and the operation counts

Inputs and references come from tests/train_cnn_ref.py (CPU only; tests/test_train_cnn_ref_cpu.py checks them without a GPU).  Harness, as in
tests/test_gpu_conv.py: every output lies in a sentinel-filled buffer between two guard bands and everything that is not a logical element
(guard bands, pad columns of wide rows) must still hold the sentinel afterwards; every input is sized exactly and followed (and preceded) by
a NaN band, and input columns / channels that the contract leaves unused hold NaN.  Each exact test first asserts, on the CPU, the bound on
the largest f32 partial sum that makes `==` legitimate (R.assert_exact: an integer number of units below 2^24); each bounded test first
asserts that no routing decision can depend on f32 rounding (R.assert_separated).  The launch geometry that enters a bound (positions per
thread, additions per reduction) is restated from the wrappers in train.hip by the *_geometry functions of the helper.

Every test prints the figure it is about to assert (`-s` shows them).  Run only this file:  python -m pytest tests/test_gpu_train_cnn.py -q -m gpu
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_cnn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1024                               # elements of guard band on either side of every buffer
NAN = float("nan")
F64 = torch.float64
U32, UB16 = R.U32, R.UB16
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_SENT = {2: 0x7BCD, 4: 0x7FC0BEEF, 8: 0x7FF8DEADBEEF1234}      # bf16 2e36; an f32 NaN; an f64 NaN: garbage for whoever adds to it


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


def _in(body, dtype):
    """An input on the device: `body` between two NaN bands, sized exactly -> (owner, address of the body)"""
    g = torch.full((GUARD,), NAN, dtype=F64)
    full = torch.cat([g, body.reshape(-1).to(F64), g]).to(dtype).cuda()
    return full, full.data_ptr() + GUARD * full.element_size()


def _in_i32(body):
    g = torch.full((GUARD,), -1, dtype=torch.int32)
    full = torch.cat([g, body.reshape(-1), g]).cuda()
    return full, full.data_ptr() + 4 * GUARD


class _Out:
    """n elements of `size` bytes between two guard bands, all of it pre-filled with a sentinel (the body too: garbage for calls that zero it)"""

    def __init__(self, n, dtype):
        self.n, self.dtype, self.size = n, dtype, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + n,), _SENT[self.size], dtype=_INT[self.size], device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.size

    def preset(self, values):
        self.buf[GUARD:GUARD + self.n] = values.reshape(-1).to(self.dtype).view(_INT[self.size]).cuda()

    def body(self):
        return self.buf[GUARD:GUARD + self.n].cpu().view(self.dtype)

    def untouched(self):
        return bool((self.buf == _SENT[self.size]).all().item())

    def rest_untouched(self, idx=None):
        """everything but the logical elements idx (positions in the body; None: the whole body) still holds the sentinel"""
        full = self.buf.cpu()
        other = torch.ones(full.numel(), dtype=torch.bool)
        pos = torch.arange(self.n) if idx is None else torch.as_tensor(np.ascontiguousarray(idx)).reshape(-1)
        assert pos.numel() == 0 or (int(pos.min()) >= 0 and int(pos.max()) < self.n)
        other[pos + GUARD] = False
        assert int((~other).sum()) == pos.numel(), "the layout maps two logical elements to one slot"
        return bool((full[other] == _SENT[self.size]).all())


def _x_index(B, Fo, T, C, ld):
    """GEMM rows: element (b, fo, t, c) at (t B + b) ld + fo C + c"""
    b, f, t, c = np.ogrid[:B, :Fo, :T, :C]
    return (t * B + b) * ld + f * C + c


def _rows_body(v, ld, fill=NAN):
    """v [B][Fo][T][C] -> GEMM-row storage [(t B + b)][ld] with `fill` in the pad columns"""
    B, Fo, T, C = v.shape
    body = torch.full((T * B * ld,), fill, dtype=F64)
    body[torch.from_numpy(_x_index(B, Fo, T, C, ld).reshape(-1))] = v.reshape(-1).to(F64)
    return body


def _say(what, **figs):
    print(f"MEASURED {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


# ------------------------------------------------------------------ 1. mt_conv1_stats, exact
@pytest.mark.parametrize("shape", R.CONV1_STATS_SHAPES)
def test_conv1_stats_exact(mta, shape):
    """sums64 == the float64 sums of conv2d(x, w, padding=1) + bias and of its square, element for element.  x: non-zero integers, w and
    bias: non-zero multiples of 1/2: z (units of 1/2) and z^2 (units of 1/4) are exact, and no thread, wave or workgroup partial -- each at
    most its workgroup's sum of |z| or z^2 -- reaches 2^24 units; the f64 atomics then add integers below 2^53."""
    lib, st = _lib()
    P = R.conv1_stats_case(*shape)
    R.assert_exact(P.units, "mt_conv1_stats")
    assert P.grid == R.conv1_stats_grid(*shape)
    (ox, px), (ow, pw), (ob, pb) = _in(P.x, torch.float32), _in(P.w, torch.float32), _in(P.bias, torch.float32)
    sums = _Out(64, F64)                                        # garbage: the call zeroes it
    _ok(lib.mt_conv1_stats(px, pw, pb, sums.ptr, P.B, P.F, P.T, st))
    torch.cuda.synchronize()
    got = sums.body()
    bad = torch.nonzero(got != P.sums).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} of 64 sums differ; first [{int(bad[0])}]: got {got[bad[0]].item()!r}, want {P.sums[bad[0]].item()!r}"
    assert sums.rest_untouched()


# ------------------------------------------------------------------ 2. mt_bn_finalize, against float64
@pytest.mark.parametrize("C,count,momentum,fold,running", R.BN_FINALIZE_CASES)
def test_bn_finalize_within_ulps_of_float64(mta, C, count, momentum, fold, running):
    """mean, rstd: the kernel computes them in f64 (a contracted multiply-add may move the variance by an f64 rounding) and rounds once:
    at most 1 ulp from the f32 rounding of the float64 value.
    running statistics r' = (1 - m) r + m s, s = f32(mean) or f32(var count/(count-1)): with (1.0f - m) one IEEE f32 operation taken as
    given, the roundings are a = (1-m) r (1/2 ulp), s (relative 2^-24, so at most 2^-24 |m s|), b = m s (1/2 ulp(b)), a + b (1/2 ulp).  The
    generator keeps a and b of one sign with |b| <= |a|, so |b| <= |r'|/2, ulp(a) <= ulp(r'), ulp(b) <= ulp(r')/2, 2^-24 |b| <= ulp(r')/2:
    1/2 + 1/2 + 1/4 + 1/2 < 2 ulp.  A biased variance is off by a factor count/(count-1).
    w_folded = w (gamma rstd32): two roundings of relative 2^-24 <= 1 ulp each: 2 ulp.  b_folded = (b - mean32) (gamma rstd32) + beta: three
    roundings on p = (b - mean32) gamma rstd32 (3 2^-24 |p|) and one of the sum (1/2 ulp); |beta| >= 3 |p| of the same sign makes
    |p| <= |b_folded| / 4: 3/4 + 1/2 < 2 ulp.  (The folded references take the kernel's f32 mean and rstd as inputs: the same expression.)"""
    lib, st = _lib()
    P = R.bn_finalize_case(C, count, momentum)
    R.assert_bn_finalize_conditions(P)
    taps = 9
    osu, psu = _in(torch.from_numpy(P.sums), F64)
    (og, pg), (obe, pbe) = _in(torch.from_numpy(P.gamma), torch.float32), _in(torch.from_numpy(P.beta), torch.float32)
    (ow, pw), (ob, pb) = _in(torch.from_numpy(P.w), torch.float32), _in(torch.from_numpy(P.b), torch.float32)
    rm, rv = _Out(C, torch.float32), _Out(C, torch.float32)
    mean, rstd, wf, bf = _Out(C, torch.float32), _Out(C, torch.float32), _Out(C * taps, torch.float32), _Out(C, torch.float32)
    if running:
        rm.preset(torch.from_numpy(P.rmean))
        rv.preset(torch.from_numpy(P.rvar))
    _ok(lib.mt_bn_finalize(psu, float(count), pg, pbe, rm.ptr if running else None, rv.ptr, P.momentum, P.eps, mean.ptr, rstd.ptr, C,
                           pw, pb, wf.ptr if fold else None, bf.ptr, taps if fold else 0, st))
    torch.cuda.synchronize()
    gm, gr = mean.body().numpy(), rstd.body().numpy()
    u_mean, u_rstd = R.ulps32(gm, P.mean.astype(np.float32)).max(), R.ulps32(gr, P.rstd.astype(np.float32)).max()
    figs = dict(mean_ulp=float(u_mean), rstd_ulp=float(u_rstd))
    if running:
        figs["rmean_ulp"] = float(R.ulps32(rm.body().numpy(), P.rmean_ref).max())
        figs["rvar_ulp"] = float(R.ulps32(rv.body().numpy(), P.rvar_ref).max())
    if fold:
        # the same expression in float64 on the kernel's own f32 mean / rstd
        sc = P.gamma.astype(np.float64) * gr.astype(np.float64)
        p = (P.b.astype(np.float64) - gm.astype(np.float64)) * sc
        figs["wf_ulp"] = float(R.ulps32(wf.body().numpy().reshape(C, taps), P.w.astype(np.float64) * sc[:, None]).max())
        figs["bf_ulp"] = float(R.ulps32(bf.body().numpy(), p + P.beta.astype(np.float64)).max())
        assert np.all(np.abs(P.beta) >= 2.9 * np.abs(p))
    _say(f"bn_finalize C={C} count={count}", **figs)
    assert u_mean <= 1 and u_rstd <= 1
    if count > 1 and P.const is not None:
        assert gr[0] == np.float32(1.0 / np.sqrt(np.float64(np.float32(R.EPS)))), "a variance that rounds below zero must clamp to rstd = 1/sqrt(eps)"
    for k in ("rmean_ulp", "rvar_ulp", "wf_ulp", "bf_ulp"):
        assert figs.get(k, 0.0) <= 2, f"{k} = {figs[k]}"
    for o in (mean, rstd):
        assert o.rest_untouched()
    for o, written in ((rm, running), (rv, running), (wf, fold), (bf, fold)):
        assert o.rest_untouched() if written else o.untouched(), "an output that the call must not write was written"


# ------------------------------------------------------------------ 3. mt_bn_stats_cl, exact
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_bn_stats_cl_exact(mta, C):
    """Integer bf16 values in [-8, 8]: every partial sum is an integer of at most sum z^2 < 2^24 (asserted).  N = 1, R-1, R+1, 3R+5 (the
    fourth row in flight out of range) and 16R+3 (two workgroups); the row behind N-1 is NaN."""
    lib, st = _lib()
    for N in R.bn_stats_ns(C):
        P = R.bn_stats_case(N, C)
        R.assert_exact(P.units, "mt_bn_stats_cl")
        oz, pz = _in(P.z, torch.bfloat16)
        sums = _Out(2 * C, F64)
        _ok(lib.mt_bn_stats_cl(pz, N, C, sums.ptr, st))
        torch.cuda.synchronize()
        got = sums.body()
        bad = torch.nonzero(got != P.sums).reshape(-1)
        assert bad.numel() == 0, f"N={N} C={C}: {bad.numel()} sums differ; first [{int(bad[0])}]: got {got[bad[0]].item()!r}, want {P.sums[bad[0]].item()!r}"
        assert sums.rest_untouched()


# ------------------------------------------------------------------ 4. mt_bn_relu_pool_apply, exact
@pytest.mark.parametrize("ties", [False, True], ids=["exact", "rne_ties"])
@pytest.mark.parametrize("B,F,T,pad", R.BN_APPLY_SHAPES)
def test_bn_relu_pool_apply_bit_exact(mta, B, F, T, pad, ties):
    """X == bf16(max over the row pair of relu(gamma (z - mean) rstd + beta)) in float64, bit for bit, in the row order t*B + b.  The
    parameters are powers of two and small integers, so gamma*rstd, the shift and the fused multiply-add are exact in f32 (asserted); the
    first case's results are bf16 values, the second case's sit on and beside round-to-nearest-even ties."""
    lib, st = _lib()
    P = R.bn_apply_case(B, F, T, ties=ties)
    R.assert_bn_apply_exact(P)
    Fo = F // 2
    ldx = Fo * 64 + pad
    oz, pz = _in(P.z, torch.bfloat16)
    par = [_in(v, torch.float32) for v in (P.mean, P.rstd, P.gamma, P.beta)]
    X = _Out(T * B * ldx, torch.bfloat16)
    _ok(lib.mt_bn_relu_pool_apply(pz, par[0][1], par[1][1], par[2][1], par[3][1], X.ptr, ldx, B, F, T, st))
    torch.cuda.synchronize()
    idx = _x_index(B, Fo, T, 64, ldx)
    got = X.body()[torch.from_numpy(idx.reshape(-1))].reshape(B, Fo, T, 64)
    want = P.ref.to(torch.float32).to(torch.bfloat16)
    bad = torch.nonzero(~(got == want))
    assert bad.numel() == 0, (f"{bad.shape[0]} of {got.numel()} differ; first at (b, fo, t, c) = {tuple(bad[0].tolist())}: "
                              f"got {got[tuple(bad[0])].item()}, want {want[tuple(bad[0])].item()}")
    assert X.rest_untouched(idx), "pad columns of X or a guard band were written"


# ------------------------------------------------------------------ 5. mt_bn_pool_bwd / mt_bn_pool_bwd_tie, against float64 autograd
def _pool_bwd_call(P, ldd_pad=0, tie=False, lo=True, grads=True, entry="tie"):
    lib, st = _lib()
    B, F, T = P.B, P.F, P.T
    Fo = F // 2
    ldd = Fo * 64 + ldd_pad
    odx, pdx = _in(_rows_body(P.dX, ldd), torch.float32)                       # pad columns of dX: NaN, unused by contract
    oz, pz = _in(P.z, torch.bfloat16)
    mean32, rstd32 = P.R.mean.float(), P.R.rstd.float()                        # the f32 roundings of the reference's statistics
    par = [_in(v, torch.float32) for v in (mean32, rstd32, P.gamma, P.beta)]
    sums = _Out(128, F64)
    dz, dzl = _Out(B * F * T * 64, torch.bfloat16), _Out(B * F * T * 64, torch.bfloat16)
    dg, db = _Out(64, torch.float32), _Out(64, torch.float32)
    a = [pdx, ldd, pz, par[0][1], par[1][1], par[2][1], par[3][1], sums.ptr, dz.ptr, dzl.ptr if lo else None, dg.ptr if grads else None, db.ptr]
    if entry == "tie":
        ot, pt = _in_i32(R.pack_tie_words(P.tie)) if tie else (None, None)
        _ok(lib.mt_bn_pool_bwd_tie(*a, pt, B, F, T, st))
    else:
        _ok(lib.mt_bn_pool_bwd(*a, B, F, T, st))
    torch.cuda.synchronize()
    for o, written in ((dz, True), (dzl, lo), (dg, grads), (db, grads), (sums, True)):
        assert o.rest_untouched() if written else o.untouched(), "an output that the call must not write was written, or a guard band"
    shape = (B, F, T, 64)
    return (dz.body().reshape(shape), dzl.body().reshape(shape) if lo else None, dg.body() if grads else None, db.body() if grads else None)


def _check_pool_bwd(P, out, ref, what):
    """ref = (dz, dgamma, dbeta) in float64.  Tolerances (R.dz_tolerance holds the derivation of the f32 part):
      n_acc    additions on the way of a pass-1 addend: one per position of the thread (the other row's term is an exact zero), 16 across
               the workgroup's rows in LDS, one f32 cast after the f64 atomics
      dz_hi + dz_lo   |.| <= tol_dz + 2^-16 |dz|: both pieces round to bf16 (8 bits: relative 2^-8), the second the remainder of the first
      dz_hi           |.| <= tol_dz + 2^-8 |dz|, and dz_hi must be a bf16 value nearest to dz_hi + dz_lo
      dgamma, dbeta   their tolerances, relative to the sums of |addends|, plus the f32 rounding of the result
      sum (hi + lo), sum (hi + lo) xhat over a channel: equal to 0 and to k dgamma eps rstd^2 (R.dz_xhat_residual; zero but for eps) within
               the sum of the element tolerances (times |xhat|): the accumulation bound"""
    dzh, dzl, dg, db = out
    dz_ref, dg_ref, db_ref = ref
    t_dz, t_dg, t_db = R.dz_tolerance(P.R, P.gamma, R.pool_bwd_geometry(P.B, P.F, P.T)[1] + 17)
    hi = dzh.to(F64)
    figs = {}
    e_hi = (hi - dz_ref).abs() - ((1 + UB16) * t_dz + UB16 * dz_ref.abs())
    figs["hi_err/2^-8|dz|"] = float(((hi - dz_ref).abs() / (UB16 * dz_ref.abs() + t_dz + 1e-300)).max())
    ok = bool((e_hi <= 0).all())
    if dzl is not None:
        s = hi + dzl.to(F64)
        tol = (1 + UB16 * UB16) * t_dz + UB16 * UB16 * dz_ref.abs()
        err = (s - dz_ref).abs()
        figs["sum_err/tol"] = float((err / (tol + 1e-300)).max())
        nz = dz_ref.abs() > 1e-3 * float(dz_ref.abs().max())
        figs["sum_relerr_max"] = float((err[nz] / dz_ref.abs()[nz]).max())
        near = R.bf16_round(s)
        nearest = bool(((s - hi).abs() <= (s - near).abs()).all())
        c0 = s.sum((0, 1, 2)).abs()
        c1 = ((s * P.R.xhat).sum((0, 1, 2)) - R.dz_xhat_residual(P.R)).abs()
        b0, b1 = tol.sum((0, 1, 2)), (tol * P.R.xhat.abs()).sum((0, 1, 2))
        figs["sum_dz/bound"] = float((c0 / (b0 + 1e-300)).max())
        figs["sum_dz_xhat/bound"] = float((c1 / (b1 + 1e-300)).max())
    if dg is not None:
        tg = t_dg + U32 * dg_ref.abs()
        tb = t_db + U32 * db_ref.abs()
        figs["dgamma_err/tol"] = float(((dg.to(F64) - dg_ref).abs() / (tg + 1e-300)).max())
        figs["dbeta_err/tol"] = float(((db.to(F64) - db_ref).abs() / (tb + 1e-300)).max())
    _say(what, **figs)
    assert ok, f"{what}: dz_hi is further from dz than its tolerance + 2^-8 |dz|"
    if dzl is not None:
        assert figs["sum_err/tol"] <= 1, f"{what}: dz_hi + dz_lo off by {figs['sum_err/tol']:.3g} times the tolerance"
        assert nearest, f"{what}: dz_hi is not a bf16 value nearest to dz_hi + dz_lo"
        assert figs["sum_dz/bound"] <= 1 and figs["sum_dz_xhat/bound"] <= 1, f"{what}: the channel sums of dz are off"
    if dg is not None:
        assert figs["dgamma_err/tol"] <= 1 and figs["dbeta_err/tol"] <= 1, f"{what}: dgamma / dbeta off"


@pytest.mark.parametrize("B,F,T", R.POOL_BWD_SHAPES)
def test_bn_pool_bwd_against_float64_autograd(mta, B, F, T):
    P = R.pool_bwd_case(B, F, T)
    R.assert_pool_bwd_case(P)
    ref = R.pool_bwd_autograd(P.z, P.dX, P.gamma, P.beta)
    full = _pool_bwd_call(P, ldd_pad=4 if T % 2 else 0, entry="plain")
    _check_pool_bwd(P, full, ref, f"bn_pool_bwd {B}x{F}x{T}")
    # dz_lo == NULL: the first piece alone, unchanged;  dgamma == NULL: no parameter gradient is written, dz unchanged
    no_lo = _pool_bwd_call(P, lo=False, entry="plain")
    assert torch.equal(no_lo[0].view(torch.int16), full[0].view(torch.int16)) and torch.equal(no_lo[2], full[2]) and torch.equal(no_lo[3], full[3])
    _check_pool_bwd(P, no_lo, ref, f"bn_pool_bwd {B}x{F}x{T} dz_lo=NULL")
    no_g = _pool_bwd_call(P, grads=False, entry="plain")
    assert torch.equal(no_g[0].view(torch.int16), full[0].view(torch.int16)) and torch.equal(no_g[1].view(torch.int16), full[1].view(torch.int16))
    # mt_bn_pool_bwd_tie with tie == NULL is the same call, bit for bit
    nt = _pool_bwd_call(P, ldd_pad=4 if T % 2 else 0, entry="tie", tie=False)
    for a, b in zip(nt, full):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b)


@pytest.mark.parametrize("B,F,T", R.POOL_BWD_SHAPES)
def test_bn_pool_bwd_tie_routes_by_the_tie_words(mta, B, F, T):
    """Rows whose bf16 z are equal but whose tie bits say greater or less, in channels with gamma*rstd positive, negative and zero: the
    reference is the closed form routed by the words (checked against autograd on the unrounded values in the CPU tests)."""
    P = R.pool_bwd_case(B, F, T, with_tie=True)
    R.assert_pool_bwd_case(P)
    out = _pool_bwd_call(P, ldd_pad=8, tie=True, entry="tie")
    _check_pool_bwd(P, out, (P.R.dz, P.R.dgamma, P.R.dbeta), f"bn_pool_bwd_tie {B}x{F}x{T}")


# ------------------------------------------------------------------ 6. mt_conv1_bwd, against float64 autograd
@pytest.mark.parametrize("ldc", [64, 32])
@pytest.mark.parametrize("B,F,T", R.CONV1_BWD_SHAPES)
def test_conv1_bwd_against_float64_autograd(mta, B, F, T, ldc):
    """dW, dgamma, dbeta within their bounds relative to the sums of |addends| (R.conv1_bwd_tolerances, plus the f32 rounding of the result);
    db, analytically zero, within its absolute bound of the order 2^-24 (operations) sum |dz|.  Integer x and dyadic w, bias make the
    recomputed z exact in f32 (asserted), and the generator keeps every post-BN value exactly tied or 1e-3 away (asserted)."""
    lib, st = _lib()
    P = R.conv1_bwd_case(B, F, T)
    R.assert_conv1_bwd_case(P)
    dW_ref, db_ref, dg_ref, dbeta_ref = R.conv1_bwd_autograd(P)
    Fo = F // 2
    da = torch.full((B, Fo, T, ldc), NAN, dtype=F64)                            # channels 32 .. ldc-1: unused by contract
    da[..., :32] = P.da
    oda, pda = _in(da, torch.bfloat16)
    par = [_in(v, torch.float32) for v in (P.x, P.w, P.bias, P.R.mean.float(), P.R.rstd.float(), P.gamma, P.beta)]
    scratch = _Out(384, F64)                                                    # garbage: the call zeroes it
    dW, db, dg, dbe = _Out(288, torch.float32), _Out(32, torch.float32), _Out(32, torch.float32), _Out(32, torch.float32)
    _ok(lib.mt_conv1_bwd(*[p[1] for p in par], pda, ldc, scratch.ptr, dW.ptr, db.ptr, dg.ptr, dbe.ptr, B, F, T, st))
    torch.cuda.synchronize()
    t_dW, t_db, t_dg, t_dbeta, sabs = R.conv1_bwd_tolerances(P, R.conv1_bwd_geometry(B, F, T)[1])
    gW = dW.body().to(F64).reshape(32, 9)
    sW = torch.einsum("bftc,bftk->ck", P.R.dz.abs(), P.taps.abs())
    figs = {
        "dW_err/tol": float(((gW - dW_ref).abs() / (t_dW + U32 * dW_ref.abs() + 1e-300)).max()),
        "dW_err/sum|addends|": float(((gW - dW_ref).abs() / (sW + 1e-300)).max()),
        "db_abs/tol": float(((db.body().to(F64) - db_ref).abs() / (t_db + 1e-300)).max()),
        "db_abs/sum|dz|": float((db.body().to(F64).abs() / (sabs + 1e-300)).max()),
        "dgamma_err/tol": float(((dg.body().to(F64) - dg_ref).abs() / (t_dg + U32 * dg_ref.abs() + 1e-300)).max()),
        "dbeta_err/tol": float(((dbe.body().to(F64) - dbeta_ref).abs() / (t_dbeta + U32 * dbeta_ref.abs() + 1e-300)).max()),
    }
    _say(f"conv1_bwd {B}x{F}x{T} ldc={ldc}", **figs)
    for k in ("dW_err/tol", "db_abs/tol", "dgamma_err/tol", "dbeta_err/tol"):
        assert figs[k] <= 1, f"{k} = {figs[k]:.3g}"
    for o in (dW, db, dg, dbe, scratch):
        assert o.rest_untouched()


# ------------------------------------------------------------------ 7. mt_rowsum_bf16, exact
@pytest.mark.parametrize("n", R.ROWSUM_NS)
def test_rowsum_bf16_exact(mta, n):
    """Non-zero integers in [-4, 4]: every partial sum is an integer below 2^24 (asserted), the f32 atomics across a row's chunks add
    integers.  ld > n with NaN between n and ld; `out` starts as garbage."""
    lib, st = _lib()
    ld = (n + 7) // 8 * 8 + 8
    for rows in R.ROWSUM_ROWS:
        P = R.rowsum_case(rows, n)
        R.assert_exact(P.units, "mt_rowsum_bf16")
        body = torch.full((rows, ld), NAN, dtype=F64)
        body[:, :n] = P.a
        body = body.reshape(-1)[:(rows - 1) * ld + n]                            # sized exactly: the last row ends at its n-th element
        oa, pa = _in(body, torch.bfloat16)
        out = _Out(rows, torch.float32)
        _ok(lib.mt_rowsum_bf16(pa, ld, n, out.ptr, rows, st))
        torch.cuda.synchronize()
        got = out.body().to(F64)
        bad = torch.nonzero(got != P.sums).reshape(-1)
        assert bad.numel() == 0, f"rows={rows} n={n}: {bad.numel()} sums differ; first row {int(bad[0])}: got {got[bad[0]].item()}, want {P.sums[bad[0]].item()}"
        assert out.rest_untouched()


# ------------------------------------------------------------------ 8. mt_dlogits_pack / mt_dlogits_pack_heads, exact
def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("B,T", [(1, 5), (3, 67), (1, 130), (3, 130)])
def test_dlogits_pack_exact(mta, B, T):
    """dL[(t B + b) 128 + p] and dLT[p ldt + t B + b] hold torch's round-to-nearest-even bf16 of dlogits[b][p][t] (a third of the inputs on
    ties), zero for p in P..127; columns T B .. ldt-1 of dLT keep the sentinel."""
    lib, st = _lib()
    Pn, M = 88, T * B
    ldt = M + 8
    v = R.rounding_values((B, Pn, T), seed=B + T)
    assert int(R.on_bf16_tie(v).sum()) > v.numel() // 4
    ov, pv = _in(v, torch.float32)
    dL, dLT = _Out(M * 128, torch.bfloat16), _Out(128 * ldt, torch.bfloat16)
    _ok(lib.mt_dlogits_pack(pv, dL.ptr, dLT.ptr, ldt, B, Pn, T, st))
    torch.cuda.synchronize()
    want = torch.zeros(T, B, 128, dtype=torch.bfloat16)
    want[:, :, :Pn] = v.to(torch.bfloat16).permute(2, 0, 1)
    assert torch.equal(_bits(dL.body().reshape(T, B, 128)), _bits(want)), "dL differs from the bf16 rounding of dlogits"
    got_t = dLT.body().reshape(128, ldt)
    assert torch.equal(_bits(got_t[:, :M]), _bits(want.reshape(M, 128).t()))
    p, m = np.ogrid[:128, :M]
    assert dL.rest_untouched() and dLT.rest_untouched(p * ldt + m)


@pytest.mark.parametrize("B,T", [(1, 5), (3, 67), (3, 130)])
def test_dlogits_pack_heads_exact(mta, B, T):
    """dL[(t B + b) ldl + head P + p], dLT[(head P + p) ldt + t B + b]; entries beyond NH*P are not written."""
    lib, st = _lib()
    NH, Pn, M, ldl = 3, 88, T * B, 384
    ldt = M + 8
    v = R.rounding_values((NH, B, Pn, T), seed=100 + B + T)
    ov, pv = _in(v, torch.float32)
    dL, dLT = _Out(M * ldl, torch.bfloat16), _Out(ldl * ldt, torch.bfloat16)
    _ok(lib.mt_dlogits_pack_heads(pv, dL.ptr, ldl, dLT.ptr, ldt, NH, B, Pn, T, st))
    torch.cuda.synchronize()
    want = v.to(torch.bfloat16).permute(3, 1, 0, 2).reshape(M, NH * Pn)          # [t][b][head][p]
    assert torch.equal(_bits(dL.body().reshape(M, ldl)[:, :NH * Pn]), _bits(want))
    assert torch.equal(_bits(dLT.body().reshape(ldl, ldt)[:NH * Pn, :M]), _bits(want.t()))
    m, c = np.ogrid[:M, :NH * Pn]
    assert dL.rest_untouched(m * ldl + c) and dLT.rest_untouched((c * ldt + m))
