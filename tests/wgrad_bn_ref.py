"""Input builders, float64 / exact references and launch-geometry restatements for the weight-gradient and BatchNorm-activation kernels
(tests/test_gpu_wgrad_bn.py): mt_conv_wgrad (csrc/conv_wgrad.hip), mt_conv2_wgrad (csrc/train.hip), mt_bn_act_fwd / mt_bn_act_bwd
(csrc/train_large.hip) and the helpers mt_transpose_bf16, mt_gather4_f32, mt_sum_slices_f32, mt_pack_wih_cf, mt_pack_jobs.

CPU only: torch on the CPU and numpy; nothing of the package's GPU side is imported and no library kernel enters a reference.  Every builder is
deterministic (seeded) and returns a SimpleNamespace with the inputs as the kernel takes them (bf16 / f32 values held in float64 tensors), the
reference, and the figure behind the test's precondition (`units` for an EXACT test: the largest possible partial sum in units, asserted below
2^24 by assert_exact; the separation of every routing decision for a BOUNDED one).  Every builder takes `wrong=`: one subtle fault applied to
the REFERENCE; tests/test_wgrad_bn_ref_cpu.py shows that each fault of FAULTS moves at least one case beyond that case's acceptance rule.

Layouts (include/mt_hip.h): channels-last tensors [b][f][t][pitch]; GEMM rows X[(t*B + b)*ld + fo*C + c]; dW [Cout][Cin][KH][KW];
mt_conv2_wgrad partials P[wg][co][tap*32 + ci], tap = kh*3 + kw.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_cnn_ref as R  # noqa: E402

U32, UB16, SEP, EPS, F64 = R.U32, R.UB16, R.SEP, R.EPS, R.F64
bf16_round, is_bf16, assert_exact, randint, rounding_values, on_bf16_tie = (R.bf16_round, R.is_bf16, R.assert_exact, R.randint,
                                                                            R.rounding_values, R.on_bf16_tie)

FAULTS = ["lo_dropped", "lo_from_hi", "kw_shift", "kh_flip", "halo_wrap", "split_lost", "tie_second", "relu_ge", "oddF_pooled",
          "xhat_b_from_a", "mask_before_pool", "invN_Fo"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ 1. mt_conv_wgrad
def cw_plan(Cout, Cin, KH, n_tiles_max):
    """cw_plan of csrc/conv_wgrad.hip -> (co_w, ci_w, ks, nc, S)"""
    co_w = 2 if Cout % 128 == 0 else 1
    ci_w = 4 if Cin % 128 == 0 else 2 if Cin % 64 == 0 else 1
    ks = 8 // (co_w * ci_w)
    nc = (Cout // (64 * co_w)) * (Cin // (32 * ci_w)) * KH
    S = 256 // nc // 8 * 8
    S = max(S, 8)
    while S > 8 and S > n_tiles_max:
        S -= 8
    return co_w, ci_w, ks, nc, S


CW_S_MAX = 256                 # nc = 1 (one class): the largest S any shape can get


def cw_tiles_max(B, F, T):
    return B * F * ((T + 63) // 64)


def cw_ws_bytes(B, F, T, Cout, Cin, KH, KW):
    if Cout <= 0 or Cin <= 0 or Cout % 64 or Cin % 32 or KH <= 0 or KW not in (1, 3):
        return 0
    _, _, ks, _, S = cw_plan(Cout, Cin, KH, cw_tiles_max(B, F, T))
    return S * ks * KH * KW * Cout * Cin * 4


def cw_row_tiles(B, F, T, KH, kh):
    """K tiles of kernel row kh: (first dz row, number of dz rows nf, tiles)"""
    dfx = kh - KH // 2
    flo, fhi = max(-dfx, 0), (F - dfx if dfx > 0 else F)
    nf = max(fhi - flo, 0)
    return flo, nf, B * nf * ((T + 63) // 64)


def cw_split_ranges(B, F, T, KH, kh, S):
    n = cw_row_tiles(B, F, T, KH, kh)[2]
    return [(n * s // S, n * (s + 1) // S) for s in range(S)]


def cw_max_tiles_per_workgroup(B, F, T, KH, S):
    return max(hi - lo for kh in range(KH) for lo, hi in cw_split_ranges(B, F, T, KH, kh, S))


def cw_empty_splits(B, F, T, KH, S):
    return sum(hi == lo for kh in range(KH) for lo, hi in cw_split_ranges(B, F, T, KH, kh, S))


def _shifted(x, KH, KW, kh, kw, wrap=False):
    """x[b][f + kh - KH/2][t + kw - KW/2][c], zero outside the image (wrap: the flat neighbour in memory instead: the fault)"""
    B, F, T, C = x.shape
    df, dt = kh - KH // 2, kw - KW // 2
    if wrap:
        flat = x.reshape(B * F * T, C)
        out = torch.zeros_like(flat)
        s = df * T + dt
        n = flat.shape[0]
        lo, hi = max(0, -s), min(n, n - s)
        if hi > lo:
            out[lo:hi] = flat[lo + s:hi + s]
        return out.reshape(B, F, T, C)
    xp = TF.pad(x, (0, 0, KW // 2, KW // 2, KH // 2, KH // 2))
    return xp[:, kh:kh + F, kw:kw + T]


def conv_wgrad_ref(hi, lo, x, KH, KW, wrong=None, S=None):
    """dW[co][ci][kh][kw] = sum (hi + lo)[b][f][t][co] x[b][f + kh - KH/2][t + kw - KW/2][ci] in float64"""
    B, F, T, Cout = hi.shape
    Cin = x.shape[-1]
    dz = hi + (lo if lo is not None else 0)
    if wrong == "lo_dropped":
        dz = hi
    elif wrong == "lo_from_hi" and lo is not None:
        dz = hi + hi
    out = torch.zeros(Cout, Cin, KH, KW, dtype=F64)
    for kh in range(KH):
        d = dz
        if wrong == "split_lost":                     # the tiles of the last non-empty split of this kernel row contribute nothing
            flo, nf, n = cw_row_tiles(B, F, T, KH, kh)
            ntt = (T + 63) // 64
            rng = [r for r in cw_split_ranges(B, F, T, KH, kh, S) if r[1] > r[0]]
            if rng:
                keep = torch.ones(B, F, T, 1, dtype=F64)
                for it in range(*rng[-1]):
                    b, r = divmod(it, nf * ntt)
                    keep[b, flo + r // ntt, (r % ntt) * 64:(r % ntt) * 64 + 64] = 0
                d = dz * keep
        dm = d.reshape(-1, Cout).t()
        for kw in range(KW):
            xs = _shifted(x, KH, KW, kh, kw, wrap=(wrong == "halo_wrap"))
            out[:, :, kh, kw] = dm @ xs.reshape(-1, Cin)
    if wrong == "kw_shift":
        out = out.roll(1, 3)
    if wrong == "kh_flip":
        out = out.flip(2)
    return out


def _edge_scale(B, F, T):
    """x16 on every chunk's first / last frame and first / last frequency row"""
    s = torch.ones(B, F, T, 1, dtype=F64)
    s[:, :, 0] = 16
    s[:, :, T - 1] = 16
    s[:, 0] = 16
    s[:, F - 1] = 16
    return s


def conv_wgrad_case(B, F, T, Cout, Cin, KH, KW, lo=True, edge=False, wrong=None, seed=0):
    """Non-zero integers: dz_hi in [-3, 3], dz_lo (INDEPENDENT of hi, not a remainder) in [-2, 2], x in [-3, 3]; edge: x16 on the border
    frames and rows of every chunk.  Every product and every partial sum is an integer; `units` bounds the largest."""
    g = _gen(11000 + seed + 3 * B + 5 * F + 7 * T + Cout + 11 * Cin + 13 * KH + KW + (1 if edge else 0))
    hi = randint(g, -3, 3, (B, F, T, Cout), nonzero=True)
    lo_t = randint(g, -2, 2, (B, F, T, Cout), nonzero=True) if lo else None
    x = randint(g, -3, 3, (B, F, T, Cin), nonzero=True)
    if edge:
        e = _edge_scale(B, F, T)
        hi, x = hi * e, x * e
        lo_t = lo_t * e if lo else None
    S = cw_plan(Cout, Cin, KH, cw_tiles_max(B, F, T))[4]
    ref = conv_wgrad_ref(hi, lo_t, x, KH, KW, wrong=wrong, S=S)
    a = hi.abs() + (lo_t.abs() if lo else 0)
    units = int((a.amax(-1).sum()) * float(x.abs().max()))
    return SimpleNamespace(B=B, F=F, T=T, Cout=Cout, Cin=Cin, KH=KH, KW=KW, hi=hi, lo=lo_t, x=x, ref=ref, units=units, S=S,
                           plan=cw_plan(Cout, Cin, KH, cw_tiles_max(B, F, T)))


def assert_conv_wgrad_case(P):
    assert_exact(P.units, "mt_conv_wgrad")
    for v in (P.hi, P.x) + ((P.lo,) if P.lo is not None else ()):
        assert is_bf16(v) and torch.equal(v, v.round())


CW_TILINGS = [(64, 32), (64, 64), (64, 128), (128, 32), (128, 64), (128, 128), (256, 128)]
# (B, F, T, KH, edge) for every tiling x KW in {3, 1} x lo in {True, False}: all T of the issue, KH = 7 with F < 4, KH = 3 with F = 1
CW_SHAPES = [(2, 3, 65, 7, True), (2, 1, 64, 3, True), (3, 3, 1, 7, False), (2, 2, 63, 1, True), (2, 5, 129, 3, True)]


# K-split cases (B, F, T, Cout, Cin, KH, KW); assert_cw_split_case holds what each claims
CW_SPLIT_CASES = {"few_tiles": (1, 2, 5, 64, 64, 3, 3), "max_S": (4, 64, 5, 128, 128, 1, 1), "three_tiles": (2, 192, 65, 64, 32, 1, 1)}


def assert_cw_split_case(name, P):
    args = (P.B, P.F, P.T, P.KH, P.S)
    if name == "few_tiles":
        assert cw_tiles_max(P.B, P.F, P.T) < 8 and P.S == 8 and cw_empty_splits(*args) >= P.KH, "no empty split"
    elif name == "max_S":
        assert P.S == CW_S_MAX and cw_max_tiles_per_workgroup(*args) == 1
    else:
        assert cw_max_tiles_per_workgroup(*args) >= 3, "no workgroup flips its double buffer more than once"


def conv_wgrad_rounding_case(B=2, F=4, T=70, Cout=128, Cin=64, KH=3, KW=3, seed=0):
    """random bf16 operands, dz as value + remainder: against float64 within n_acc u sum |piece * x| (n_acc: the products one output
    accumulates, both pieces, plus the slices the reduce kernel adds and its 16-way tree)"""
    g = _gen(12000 + seed)
    v = torch.randn(B, F, T, Cout, generator=g, dtype=F64)
    hi = bf16_round(v)
    lo = bf16_round(v - hi)
    x = bf16_round(torch.randn(B, F, T, Cin, generator=g, dtype=F64))
    _, _, ks, _, S = cw_plan(Cout, Cin, KH, cw_tiles_max(B, F, T))
    ref = conv_wgrad_ref(hi, lo, x, KH, KW)
    sabs = conv_wgrad_ref(hi.abs(), lo.abs(), x.abs(), KH, KW)
    n_acc = 2 * B * F * T + S * ks + 16
    return SimpleNamespace(B=B, F=F, T=T, Cout=Cout, Cin=Cin, KH=KH, KW=KW, hi=hi, lo=lo, x=x, ref=ref, tol=n_acc * U32 * sabs + U32 * ref.abs(),
                           n_acc=n_acc)


def conv_wgrad_autograd(hi, lo, x, KH, KW):
    """float64 conv2d autograd: padding (KH/2, KW/2)"""
    Cout, Cin = hi.shape[-1], x.shape[-1]
    w = torch.zeros(Cout, Cin, KH, KW, dtype=F64, requires_grad=True)
    dz = hi + (lo if lo is not None else 0)
    TF.conv2d(x.permute(0, 3, 1, 2), w, padding=(KH // 2, KW // 2)).backward(dz.permute(0, 3, 1, 2))
    return w.grad


# ------------------------------------------------------------------ 2. mt_conv2_wgrad
def conv2_tiles(B, F, T):
    return B * ((F + 15) // 16) * ((T + 15) // 16)


def conv2_tiles_of(wg, n_wg, B, F, T):
    return len(range(wg, conv2_tiles(B, F, T), n_wg))


CONV2_SHAPES = [(2, 1, 1), (2, 5, 17), (2, 16, 33), (2, 17, 5), (2, 33, 16), (3, 33, 33), (2, 33, 100)]     # 2 .. 42 tiles
CONV2_NWG = [1, 3, 256]


def conv2_wgrad_case(B, F, T, wrong=None, seed=0):
    """a1 [B][F][T][32], dz_hi / dz_lo [B][F][T][64]: non-zero integers with the chunk borders x16; dW over hi + lo, db over hi alone (every
    channel sum of lo is made non-zero: it would show in db)"""
    g = _gen(13000 + seed + B + 5 * F + 7 * T)
    e = _edge_scale(B, F, T)
    a1 = randint(g, -3, 3, (B, F, T, 32), nonzero=True) * e
    hi = randint(g, -3, 3, (B, F, T, 64), nonzero=True) * e
    lo = randint(g, -2, 2, (B, F, T, 64), nonzero=True)
    s = lo.sum((0, 1, 2))
    lo[0, 0, 0] = torch.where(s == 0, lo[0, 0, 0] + 1, lo[0, 0, 0])
    dW = conv_wgrad_ref(hi, lo, a1, 3, 3, wrong=wrong, S=8)
    db = hi.sum((0, 1, 2))
    units = int(((hi.abs() + lo.abs()).amax(-1).sum()) * float(a1.abs().max()))
    return SimpleNamespace(B=B, F=F, T=T, a1=a1, hi=hi, lo=lo, dW=dW, db=db, units=units)


def conv2_from_partials(out288):
    """[64][tap*32 + ci] -> [64][32][3][3]"""
    return out288.reshape(64, 9, 32).permute(0, 2, 1).reshape(64, 32, 3, 3)


# ------------------------------------------------------------------ 3. mt_bn_act_fwd
def bn_fwd_grid(B, F, T, C, pool):
    """(positions, positions per workgroup and pass, workgroups): a thread = 8 channels, two positions per loop trip, at most 8192 workgroups"""
    n = B * (F // 2 if pool else F) * T
    ppb = 256 // (C // 8)
    return n, ppb, min((n + 2 * ppb - 1) // (2 * ppb), 8192)


def bn_bwd_grid(B, F, T, C, pool):
    """(row groups, ppb, workgroups, additions per pass-1 addend): a thread = 4 channels, two positions per trip, at most 2048 workgroups"""
    n = B * ((F + 1) // 2 if pool else F) * T
    ppb = 256 // (C // 4)
    g = min((n + 2 * ppb - 1) // (2 * ppb), 2048)
    trips = -(-n // (2 * g * ppb))
    return n, ppb, g, 2 * trips * (2 if pool else 1) + ppb + 1


def _exact_params(g, C):
    """gamma*rstd in {+-1, +-2, +-1/2, 0}, rstd a power of two, integer mean, half-integer beta (zero in channels c % 8 == 5)"""
    sc = torch.tensor([1, -1, 2, -2, 0.5, 1, 0, -0.5])[torch.arange(C) % 8].to(F64)
    rstd = torch.tensor([0.5, 1, 2, 0.25])[(torch.arange(C) // 8) % 4].to(F64)
    mean = randint(g, -2, 2, (C,))
    beta = randint(g, -6, 6, (C,)) / 2
    beta[torch.arange(C) % 8 == 5] = 0.0
    return mean, rstd, sc / rstd, beta


def _mask_table(g, B, C, negative):
    """Dropout2d's table for p = 0.5: 0 or exactly 2.  negative: a fifth of the entries are -2 -- not a value the dropout kernel writes, but
    the table is an argument, and only a negative scale makes the order of pool and mask observable (max(s a, s b) = s max(a, b) for s >= 0)"""
    m = torch.where(torch.rand(B, C, generator=g) < 0.5, 0.0, 2.0).to(F64)
    if negative:
        m = torch.where(torch.rand(B, C, generator=g) < 0.2, -2.0, m.double()).to(F64)
    return m


def bn_act_forward(za, pa, zb, pb, mask, relu, pool, wrong=None):
    """float64: Dropout2d(MaxPool((2,1))(ReLU(BN_a(za) [+ BN_b(zb)]))) with the GIVEN mean / rstd; p = (mean, rstd, gamma, beta)"""
    y = pa[2] * ((za - pa[0]) * pa[1]) + pa[3]
    if zb is not None:
        y = y + pb[2] * ((zb - pb[0]) * pb[1]) + pb[3]
    if relu:
        y = torch.relu(y)
    m = None if mask is None else mask[:, None, None, :]
    if wrong == "mask_before_pool" and m is not None:
        y, m = y * m, None
    if pool:
        Fo = y.shape[1] // 2
        y = torch.maximum(y[:, 0:2 * Fo:2], y[:, 1:2 * Fo:2])
    return y if m is None else y * m


def bn_fwd_case(B, F, T, C, two, relu, pool, mask, ties=False, wrong=None, seed=0):
    """exact: integer z in [-7, 7], parameters of _exact_params: gamma*rstd, beta - mean*gamma*rstd and every fma are exact, results are
    multiples of 1/2 below 2^7 (bf16 values), the mask scales by 0 / +-2.  ties (single branch): |z| in 128..255, gamma = rstd = 1,
    mean = 0, beta in {1/2, 1/4, ...}: results on and beside bf16 round-to-nearest-even ties.  The row that an odd F drops holds NaN."""
    g = _gen(14000 + seed + B + 3 * F + 5 * T + 7 * C + (1 if two else 0) + 2 * relu + 4 * pool + (8 if mask else 0) + (16 if ties else 0))
    if ties:
        assert not two
        za = randint(g, 128, 255, (B, F, T, C)) * torch.where(torch.rand(B, F, T, C, generator=g) < 0.25, -1.0, 1.0).to(F64)
        one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
        pa = (zero, one, one, torch.tensor([0.5, 0.25, 0.75, -0.5, 0.5, -0.25, 0.0, -0.75])[torch.arange(C) % 8].to(F64))
    else:
        za = randint(g, -7, 7, (B, F, T, C), nonzero=True)
        pa = _exact_params(g, C)
    zb = randint(g, -7, 7, (B, F, T, C), nonzero=True) if two else None
    pb = _exact_params(g, C) if two else None
    mk = _mask_table(g, B, C, negative=True) if mask else None
    ref = bn_act_forward(za, pa, zb, pb, mk, relu, pool, wrong=wrong)
    if pool and F % 2:
        za = za.clone()
        za[:, F - 1] = float("nan")
        if two:
            zb = zb.clone()
            zb[:, F - 1] = float("nan")
    return SimpleNamespace(B=B, F=F, T=T, C=C, za=za, pa=pa, zb=zb, pb=pb, mask=mk, relu=relu, pool=pool, ref=ref, ties=ties,
                           Fo=F // 2 if pool else F)


def assert_bn_fwd_exact(P):
    """gamma*rstd, mean*(gamma*rstd), the shift and z*(gamma*rstd) + shift are dyadic numbers of few bits; off the tie case the result is bf16"""
    Fu = 2 * P.Fo if P.pool else P.F
    for z, p in ((P.za, P.pa),) + (((P.zb, P.pb),) if P.zb is not None else ()):
        sc = p[2] * p[1]
        sh = p[3] - p[0] * sc
        a = z[:, :Fu] * sc + sh
        for v in (sc, p[0] * sc, sh, a):
            assert torch.equal((v * 16).round(), v * 16) and float(v.abs().max()) * 16 < 2 ** 24
        assert is_bf16(z[:, :Fu])
    if not P.ties:
        assert is_bf16(P.ref), "a result is not a bf16 value"
    else:
        r = P.ref[P.ref > 0]
        on_tie = (r * 2 == (r * 2).round()) & (r != r.round())
        assert int(on_tie.sum()) > r.numel() // 8 and int((~on_tie).sum()) > r.numel() // 8


def bn_fwd_cap_case():
    """just beyond the 8192-workgroup cap at C = 256: B Fo T = 3 x 47 x 937 = 132117 > 2 x 8192 x 8 positions, so some workgroups take a second
    loop trip whose second position is out of range.  Kept in f32 integers: z int8 in [-7, 7], y = relu(z sc + sh), all small dyadics."""
    B, F, T, C = 3, 47, 937, 256
    n, ppb, grid = bn_fwd_grid(B, F, T, C, 0)
    assert grid == 8192 and 2 * grid * ppb < n < 3 * grid * ppb
    g = _gen(14999)
    z = torch.randint(-7, 8, (B, F, T, C), generator=g, dtype=torch.int8).float()
    mean, rstd, gamma, beta = (v.float() for v in _exact_params(g, C))
    sc = gamma * rstd
    ref = torch.relu(z * sc + (beta - mean * sc))
    assert float(ref.max()) < 128 and bool(torch.equal(ref * 2, (ref * 2).round()))
    return SimpleNamespace(B=B, F=F, T=T, C=C, z=z, p=(mean, rstd, gamma, beta), ref=ref)


# ------------------------------------------------------------------ 4. mt_bn_act_bwd
def bn_act_bwd_closed(za, pa, zb, pb, mask, g, relu, pool, wrong=None):
    """Closed form of d/dz_a, d/dz_b, d/dgamma, d/dbeta of sum(g * bn_act_forward(...)) in float64 WITH mean / rstd as given (the true batch
    statistics make it autograd's result).  Routing: the larger post-ReLU value of a row pair takes the gradient, a tie goes to the FIRST row;
    ReLU passes it where y > 0; the last row of an odd F under pool gets none (only the mean terms); N = B F T."""
    B, F, T, C = za.shape
    Fo = F // 2 if pool else F
    xa = (za - pa[0]) * pa[1]
    y = pa[2] * xa + pa[3]
    xb = None
    if zb is not None:
        xb = (zb - pb[0]) * pb[1]
        y = y + pb[2] * xb + pb[3]
    act = (y >= 0) if wrong == "relu_ge" else (y > 0)
    if not relu:
        act = torch.ones_like(act)
    r = torch.relu(y) if relu else y
    gm = g if mask is None else g * mask[:, None, None, :]
    dy = torch.zeros_like(za)
    if pool:
        r0, r1 = r[:, 0:2 * Fo:2], r[:, 1:2 * Fo:2]
        if wrong == "mask_before_pool" and mask is not None:
            r0, r1 = r0 * mask[:, None, None, :], r1 * mask[:, None, None, :]
        second = (r1 >= r0) if wrong == "tie_second" else (r1 > r0)
        dy[:, 0:2 * Fo:2] = torch.where(~second & act[:, 0:2 * Fo:2], gm, torch.zeros_like(gm))
        dy[:, 1:2 * Fo:2] = torch.where(second & act[:, 1:2 * Fo:2], gm, torch.zeros_like(gm))
        if wrong == "oddF_pooled" and F % 2:
            dy[:, F - 1] = torch.where(act[:, F - 1], gm[:, Fo - 1], torch.zeros_like(gm[:, 0]))
    else:
        dy = torch.where(act, gm, torch.zeros_like(gm))
    N = B * (Fo if wrong == "invN_Fo" else F) * T
    out = SimpleNamespace(N=N, y=y, dy=dy, dbeta=dy.sum((0, 1, 2)), a=None, b=None)
    for name, x, p in (("a", xa, pa), ("b", xb, pb)):
        if x is None:
            continue
        xg = xa if (wrong == "xhat_b_from_a" and name == "b") else x
        dgamma = (dy * xg).sum((0, 1, 2))
        k = p[2] * p[1]
        dz = k * (dy - out.dbeta / N - x * dgamma / N)
        setattr(out, name, SimpleNamespace(N=N, mean=p[0], rstd=p[1], xhat=x, dy=dy, dbeta=out.dbeta, dgamma=dgamma, k=k, dz=dz))
    return out


def bn_act_bwd_autograd(za, ga, ba, zb, gb, bb, mask, g, relu, pool):
    """the same by float64 torch autograd with batch statistics as functions of z -> (dza, dgamma_a, dbeta_a, dzb, dgamma_b, dbeta_b)"""
    leaves = [v.clone().requires_grad_(True) if v is not None else None for v in (za, ga, ba, zb, gb, bb)]
    za_, ga_, ba_, zb_, gb_, bb_ = leaves
    m, r = R.batch_stats(za_)
    y = ga_ * (za_ - m) * r + ba_
    if zb is not None:
        m, r = R.batch_stats(zb_)
        y = y + gb_ * (zb_ - m) * r + bb_
    if relu:
        y = torch.relu(y)
    if pool:
        y = TF.max_pool2d(y.permute(0, 3, 1, 2), (2, 1)).permute(0, 2, 3, 1)
    if mask is not None:
        y = y * mask[:, None, None, :]
    (y * g).sum().backward()
    return [v.grad if v is not None else None for v in leaves]


def bn_bwd_int_case(B, F, T, C, two, relu, pool, mask, wrong=None, seed=0):
    """Integer data, parameters of _exact_params (arguments of the call, not statistics): xhat is a multiple of 1/8, dy an integer, every
    pass-1 partial sum an integer number of eighths (units: asserted below 2^24), so sums, dgamma and dbeta are exact.  A fifth of the row
    pairs are duplicated rows (exact pool ties); in the channels with beta = 0 a z equal to the mean gives y = 0 exactly (single branch)."""
    g = _gen(15000 + seed + B + 3 * F + 5 * T + 7 * C + (1 if two else 0) + 2 * relu + 4 * pool + (8 if mask else 0))
    za = randint(g, -6, 6, (B, F, T, C))
    zb = randint(g, -6, 6, (B, F, T, C)) if two else None
    Fo = F // 2 if pool else F
    if pool:
        dup = torch.rand(B, Fo, T, C, generator=g) < 0.2
        za[:, 1:2 * Fo:2] = torch.where(dup, za[:, 0:2 * Fo:2], za[:, 1:2 * Fo:2])
        if two:
            zb[:, 1:2 * Fo:2] = torch.where(dup, zb[:, 0:2 * Fo:2], zb[:, 1:2 * Fo:2])
    pa = _exact_params(g, C)
    pb = _exact_params(g, C) if two else None
    mk = _mask_table(g, B, C, negative=True) if mask else None
    gd = randint(g, -3, 3, (B, Fo, T, C), nonzero=True)
    cf = bn_act_bwd_closed(za, pa, zb, pb, mk, gd, relu, pool, wrong=wrong)
    units = 8 * int(max(float((cf.dy.abs() * v.xhat.abs()).sum((0, 1, 2)).max()) for v in (cf.a, cf.b) if v is not None))
    units = max(units, int(cf.dy.abs().sum((0, 1, 2)).max()))
    return SimpleNamespace(B=B, F=F, T=T, C=C, Fo=Fo, za=za, pa=pa, zb=zb, pb=pb, mask=mk, g=gd, relu=relu, pool=pool, cf=cf, units=units,
                           exact=True)


def assert_bn_bwd_int_case(P):
    assert_exact(P.units, "mt_bn_act_bwd")
    for v in (P.cf.a, P.cf.b):
        if v is not None:
            assert torch.equal(v.xhat * 8, (v.xhat * 8).round())
    assert torch.equal(P.cf.y * 16, (P.cf.y * 16).round()) and float(P.cf.y.abs().max()) * 16 < 2 ** 24       # y exact in f32: routing is too
    if P.pool and P.B * P.Fo * P.T >= 20:
        Fo = P.Fo
        tied = P.cf.y[:, 0:2 * Fo:2] == P.cf.y[:, 1:2 * Fo:2]
        assert bool((tied & (P.cf.dy[:, 0:2 * Fo:2] != 0)).any()), "no tied pair with a gradient"
    if P.relu and P.zb is None and P.B * P.F * P.T >= 20:
        assert bool((P.cf.y == 0).any()), "no y that is exactly zero"


def bn_bwd_real_case(B, F, T, C, two, relu, pool, mask, wrong=None, seed=0):
    """bf16-rounded randn with the TRUE batch statistics.  Channels 0..3: negative gamma_a, channel 8: gamma_a = 0.  A fifth of the row pairs
    are duplicated rows (exact ties: the first row wins).  Values within 2 SEP of zero (ReLU) or of their partner (pool) are redrawn."""
    g = _gen(16000 + seed + B + 3 * F + 5 * T + 7 * C + (1 if two else 0) + 2 * relu + 4 * pool + (8 if mask else 0))
    Fo = F // 2 if pool else F
    za = bf16_round(torch.randn(B, F, T, C, generator=g, dtype=F64) * 1.5 + 0.3)
    zb = bf16_round(torch.randn(B, F, T, C, generator=g, dtype=F64)) if two else None
    dup = torch.rand(B, Fo, T, C, generator=g) < 0.2 if pool else None

    def par(neg):
        ga = (0.5 + torch.rand(C, generator=g, dtype=F64)).float().to(F64)
        be = (torch.randn(C, generator=g, dtype=F64) * 0.3).float().to(F64)
        if neg:
            ga[:4] = -ga[:4]
            ga[8] = 0.0
        return ga, be
    (ga, ba), (gb, bb) = par(True), (par(False) if two else (None, None))
    mk = _mask_table(g, B, C, negative=True) if mask else None
    for _ in range(60):
        if pool:
            za[:, 1:2 * Fo:2] = torch.where(dup, za[:, 0:2 * Fo:2], za[:, 1:2 * Fo:2])
            if two:
                zb[:, 1:2 * Fo:2] = torch.where(dup, zb[:, 0:2 * Fo:2], zb[:, 1:2 * Fo:2])
        ma, ra = R.batch_stats(za)
        y = ga * (za - ma) * ra + ba
        if two:
            mb, rb = R.batch_stats(zb)
            y = y + gb * (zb - mb) * rb + bb
        bad = (y.abs() < 2 * SEP) if relu else torch.zeros_like(y, dtype=torch.bool)
        if pool:
            r = torch.relu(y) if relu else y
            near = ((r[:, 0:2 * Fo:2] - r[:, 1:2 * Fo:2]).abs() < 2 * SEP) & ~dup & ~((r[:, 0:2 * Fo:2] == 0) & (r[:, 1:2 * Fo:2] == 0))
            if not two:
                near &= (ga != 0)
            bad[:, 1:2 * Fo:2] |= near
        if not bool(bad.any()):
            break
        za = torch.where(bad, bf16_round(torch.randn(B, F, T, C, generator=g, dtype=F64) * 1.5 + 0.3), za)
    pa = (ma, ra, ga, ba)
    pb = (mb, rb, gb, bb) if two else None
    gd = bf16_round(torch.randn(B, Fo, T, C, generator=g, dtype=F64))
    cf = bn_act_bwd_closed(za, pa, zb, pb, mk, gd, relu, pool, wrong=wrong)
    return SimpleNamespace(B=B, F=F, T=T, C=C, Fo=Fo, za=za, pa=pa, zb=zb, pb=pb, mask=mk, g=gd, relu=relu, pool=pool, cf=cf, dup=dup,
                           exact=False)


def bn_bwd_separation(P):
    """smallest distance of a ReLU input to zero and of two pool candidates that are neither duplicated rows nor both clamped to zero (nor,
    with a single branch, in a gamma = 0 channel: y = fma(0, xhat, beta) = beta in any arithmetic)"""
    y = P.cf.y
    d0 = float(y.abs().min()) if P.relu else float("inf")
    dp = float("inf")
    if P.pool:
        Fo = P.Fo
        r = torch.relu(y) if P.relu else y
        r0, r1 = r[:, 0:2 * Fo:2], r[:, 1:2 * Fo:2]
        ne = ~P.dup & ~((r0 == 0) & (r1 == 0))
        if P.zb is None:
            ne = ne & (P.pa[2] != 0)
        if bool(ne.any()):
            dp = float((r0 - r1).abs()[ne].min())
    return d0, dp


def assert_bn_bwd_real_case(P):
    """no ReLU or pool decision depends on f32 rounding: every one is SEP wide, and the kernel's y = fma(ga, xa, ba) [+ fma(gb, xb, bb)] is
    within u (|gamma| (|mean| rstd + 3 |xhat|) per branch + 2 |y|) of the float64 value: far inside"""
    d0, dp = bn_bwd_separation(P)
    assert d0 >= SEP and dp >= SEP, f"{d0:.2e} from zero / {dp:.2e} from the partner: routing could depend on f32 rounding"
    err = 2 * P.cf.y.abs()
    for v, p in ((P.cf.a, P.pa), (P.cf.b, P.pb)):
        if v is not None:
            err = err + p[2].abs() * (p[0].abs() * p[1] + 3 * v.xhat.abs())
    assert float(err.max()) * U32 < SEP / 4
    assert is_bf16(P.za) and is_bf16(P.g)
    if P.pool and P.B * P.Fo * P.T >= 20:
        assert bool((P.dup & (P.cf.dy[:, 0:2 * P.Fo:2] != 0)).any()), "no tied pair with a gradient"
        assert bool((P.cf.dy[:, 1:2 * P.Fo:2] != 0).any())


def bn_bwd_tolerances(P):
    """per branch (tol_dz, tol_dgamma, tol_dbeta) by R.dz_tolerance (the derivation is there: u = 2^-24 times the operations on the path) with
    the additions of this kernel's pass 1: a thread's positions, the ppb rows added in LDS, the f32 cast behind the f64 atomics"""
    n_acc = bn_bwd_grid(P.B, P.F, P.T, P.C, P.pool)[3]
    return [R.dz_tolerance(v, p[2], n_acc) if v is not None else None for v, p in ((P.cf.a, P.pa), (P.cf.b, P.pb))]


def hi_bound(dz, t_dz):
    """|dz_hi - dz|: the f32 value is within t_dz, its bf16 rounding moves it by at most 2^-8 of itself"""
    return (1 + UB16) * t_dz + UB16 * dz.abs()


def sum_bound(dz, t_dz):
    """|dz_hi + dz_lo - dz|: the second piece is the bf16 rounding of the remainder, itself at most 2^-8 of the value"""
    return (1 + UB16 * UB16) * t_dz + UB16 * UB16 * dz.abs()


def lo_gain(dz, t_dz):
    """How much closer hi + lo must be than hi alone, as a ratio of summed absolute errors.  A bf16 rounding of a value whose mantissa is spread
    evenly errs by a quarter spacing on average, and the spacing is at least 2^-8 |v|: sum |hi - dz| >= 2^-10 sum |dz| less fluctuation, for
    which half is allowed: 2^-11 sum |dz|.  sum |hi + lo - dz| <= sum of sum_bound.  The ratio of the two is what two pieces buy over one:
    about 2^-11 / (2^-16 + a few 2^-24 times the cancellation)."""
    return float((2.0 ** -11 * dz.abs()).sum() / sum_bound(dz, t_dz).sum())


def bn_bwd_detected(P, Pw):
    """Does the acceptance rule of P's test reject the (wrong) reference Pw?  exact case: any of sums / dgamma / dbeta differs; any case: a dz
    further than twice the bound on hi + lo from the true one (a kernel within the bound of the wrong value is beyond it from the true one)"""
    hit = False
    for v, w, tol in zip((P.cf.a, P.cf.b), (Pw.cf.a, Pw.cf.b), bn_bwd_tolerances(P)):
        if v is None:
            continue
        if P.exact and (not torch.equal(v.dgamma, w.dgamma) or not torch.equal(v.dbeta, w.dbeta)):
            hit = True
        if bool(((v.dz - w.dz).abs() > 2 * sum_bound(v.dz, tol[0])).any()):
            hit = True
    return hit


# (B, F, T, C, two, relu, pool, mask, src): the four (TWO, POOL) instantiations with ReLU on and off, odd F under pool, mask + pool + second
# branch together, both gradient sources; src: "cl" (bf16 channels-last, ldd_cl > C) or "x" (f32 GEMM rows, ldd_x > Fo C)
BN_BWD_CASES = [(2, 4, 7, 32, False, 1, 0, False, "cl"), (2, 5, 9, 64, False, 1, 1, False, "x"), (3, 3, 11, 128, True, 1, 0, True, "x"),
                (2, 7, 13, 64, True, 1, 1, True, "cl"), (2, 6, 5, 256, True, 0, 1, True, "x"), (2, 5, 6, 32, False, 0, 1, True, "cl"),
                (1, 2, 65, 128, False, 0, 0, False, "cl"), (2, 3, 17, 256, True, 0, 0, False, "cl")]
BN_BWD_CAP = (3, 13, 937, 256, False, 1, 1, False, "cl")        # 3 x 7 x 937 = 19677 row groups > 2 x 2048 x 4

# forward: (B, F, T, C, two, relu, pool, mask, out_mode)
BN_FWD_CASES = [(2, 3, 1, 32, False, 1, 0, False, 0), (2, 5, 7, 64, True, 1, 1, True, 1), (1, 4, 64, 128, False, 0, 1, False, 0),
                (3, 2, 65, 256, True, 0, 0, True, 1), (1, 3, 937, 64, False, 1, 1, True, 0), (2, 2, 937, 32, True, 1, 0, False, 1),
                (2, 7, 7, 256, False, 0, 1, True, 1), (1, 5, 65, 128, True, 1, 1, False, 0)]


# ------------------------------------------------------------------ 5. helpers
def transpose_ref(src, R_, C, ldd, Cd):
    """dst[c][r] = src[r][c] for r < R, c < C; rows c < Cd, columns r < ldd all written, zero outside the source"""
    out = torch.zeros(Cd, ldd, dtype=src.dtype)
    out[:C, :R_] = src[:R_, :C].t()
    return out


def gather4_ref(src, n, s, alpha):
    idx = sum(np.arange(nk).reshape([-1 if i == k else 1 for i in range(4)]) * sk for k, (nk, sk) in enumerate(zip(n, s)))
    return alpha * src[torch.from_numpy(np.ascontiguousarray(idx))]


def gather4_takes_lds_kernel(n, s):
    return s[2] == 1 and s[3] == n[2] and n[2] > 1 and n[3] > 1 and n[3] * (n[2] + 1) * 4 <= 48 * 1024 and n[0] < 65536


def pack_wih_ref(w, H, Hp, C, F):
    """w f32 [4H][C F] (feature c F + f) -> [4 Hp][F C] (feature f C + c), rows j >= H of each gate zero"""
    out = torch.zeros(4, Hp, F, C, dtype=w.dtype)
    out[:, :H] = w.reshape(4, H, C, F).permute(0, 1, 3, 2)
    return out.reshape(4 * Hp, F * C)


def pack_job_ref(src, src2, job):
    """one mt_pack_job (include/mt_hip.h) on CPU tensors -> [Rp][Cp] float64"""
    out = torch.zeros(job["Rp"], job["Cp"], dtype=F64)
    for r in range(job["Rp"]):
        r1, r2 = divmod(r, job["Rn2"])
        if r1 >= job["R1v"] or r2 >= job["R2v"]:
            continue
        for c in range(job["Cp"]):
            c1, c2 = divmod(c, job["Cn2"])
            if c1 >= job["C1v"] or c2 >= job["C2v"]:
                continue
            off = r1 * job["sr1"] + r2 * job["sr2"] + c1 * job["sc1"] + c2 * job["sc2"]
            out[r, c] = float(src[off]) + (float(src2[off]) if src2 is not None else 0.0)
    return out
