"""Input generators and float64 references for the CNN training kernels of csrc/train.hip (tests/test_gpu_train_cnn.py).

CPU only: torch on the CPU and numpy; nothing of the package's GPU side is imported.  Every generator is deterministic (seeded) and returns a
SimpleNamespace that holds the inputs as the kernel takes them (f32 / bf16 values kept in f32 or f64 tensors), the float64 reference, and the
figures behind the test's precondition:

  * an EXACT test needs every f32 partial sum of the kernel to be an integer multiple of one unit below 2^24 units; the generators return the
    data's largest possible partial sum in units (`*_units`) and the test asserts it against 2^24 (`assert_exact`);
  * a BOUNDED test needs every routing decision (pool winner, ReLU sign) to be the same in f32 and in float64; the generators keep every
    post-BN value either exactly tied with its partner or at least SEP away from it and from zero (`assert_separated`).

Layouts (include/mt_hip.h): channels-last activations z[b][f][t][c]; pooled GEMM rows X[(t*B + b)*ld + fo*C + c].
tests/test_train_cnn_ref_cpu.py runs every generator, asserts every condition and checks the closed forms against torch autograd.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as TF

U32 = 2.0 ** -24                 # f32 unit roundoff (round to nearest)
UB16 = 2.0 ** -8                 # bf16 unit roundoff: 8 significant bits
SEP = 1e-3                       # separation of post-BN values that are not exactly tied
EPS = 1e-5                       # nn.BatchNorm2d's eps
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def bf16_round(x):
    """round-to-nearest-even to bf16, returned in the dtype of x"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def is_bf16(x):
    return bool(torch.equal(bf16_round(x.to(F64)), x.to(F64)))


def assert_exact(units, what):
    """Every f32 partial sum is an integer number of units; below 2^24 of them it is exact in any order."""
    assert units < 2 ** 24, f"{what}: a partial sum can reach {units} units >= 2^24: the comparison would not be exact"


def randint(g, lo, hi, shape, nonzero=False):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    if nonzero:
        v = torch.where(v == 0, torch.full_like(v, float(hi)), v)
    return v


# ------------------------------------------------------------------ 1. mt_conv1_stats
CONV1_STATS_SHAPES = [(1, 1, 1), (1, 1, 5), (2, 5, 1), (1, 4, 7), (2, 2, 6), (1, 3, 87), (3, 37, 41)]


def conv1_stats_grid(B, F, T):
    """mt_conv1_stats: workgroups of 256 threads, 16 positions per thread, at most 512 workgroups"""
    n = B * F * T
    return max(1, min((n + 4095) // 4096, 512))


def conv1_stats_case(B, F, T, seed=0):
    """x: non-zero integers in [-3, 3]; w, bias: non-zero multiples of 1/2 in [-2, 2].  z is a multiple of 1/2 and z^2 of 1/4, both exact in
    f32.  No weight and no input is zero, so each of the nine taps changes z wherever it is inside the image."""
    g = _gen(1000 + seed + 7 * B + 11 * F + 13 * T)
    x = randint(g, -3, 3, (B, F, T), nonzero=True)
    w = randint(g, -4, 4, (32, 9), nonzero=True) / 2
    bias = randint(g, -4, 4, (32,), nonzero=True) / 2
    z = TF.conv2d(x[:, None], w.reshape(32, 1, 3, 3), bias, padding=1)               # [B][32][F][T], float64: exact
    sums = torch.cat([z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))])
    # largest partial sum a workgroup can form: position i belongs to workgroup (i // 256) % grid
    grid = conv1_stats_grid(B, F, T)
    wg = (torch.arange(B * F * T) // 256) % grid
    zp = z.permute(1, 0, 2, 3).reshape(32, -1)
    a1 = torch.zeros(32, grid, dtype=F64).index_add_(1, wg, zp.abs())
    a2 = torch.zeros(32, grid, dtype=F64).index_add_(1, wg, zp * zp)
    units = int(max(float(a1.max()) * 2, float(a2.max()) * 4))
    assert torch.equal(z * 2, (z * 2).round())
    return SimpleNamespace(B=B, F=F, T=T, x=x, w=w, bias=bias, z=z, sums=sums, units=units, grid=grid)


# ------------------------------------------------------------------ 2. mt_bn_finalize
def ulps32(got, ref64):
    """|got - ref| in units of the f32 spacing at ref (got: f32 values, ref: float64)"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    sp = np.spacing(np.abs(ref64.astype(np.float32))).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) / sp


BN_FINALIZE_CASES = [  # (C, count, momentum, fold, running)
    (32, 2, 0.1, True, True), (32, 7, 0.1, True, True), (64, 1, 0.1, False, True), (64, 7, 0.25, True, True),
    (256, 2, 0.03, False, True), (256, 1000, 0.1, True, False), (32, 7, 0.1, False, False),
]


def bn_finalize_case(C, count, momentum, seed=0):
    """sums of `count` random values per channel (channel 0: a constant whose E[z^2] - E[z]^2 rounds below zero in float64), and parameters
    chosen so that no sum in the kernel cancels: running_mean has the sign of the batch mean and at least its size, likewise running_var, and
    beta has the sign of (b - mean)*gamma*rstd and three times its size.  The ulp bounds in tests/test_gpu_train_cnn.py rest on that."""
    g = _gen(2000 + seed + C + 17 * count)
    data = torch.randn(C, count, generator=g, dtype=F64) * (0.5 + torch.rand(C, 1, generator=g, dtype=F64) * 3) \
        + torch.randn(C, 1, generator=g, dtype=F64) * 2
    const = None
    for k in range(1, 400):                                                       # a constant channel whose raw variance is negative
        v = 3.0 + k / 97.0
        s, q = math.fsum([v] * count), math.fsum([v * v] * count)
        if q / count - (s / count) * (s / count) < 0.0:
            const = v
            break
    sums = np.zeros(2 * C)
    for c in range(C):
        row = [const] * count if (c == 0 and const is not None) else data[c].tolist()
        sums[c], sums[C + c] = math.fsum(row), math.fsum(v * v for v in row)
    m32 = np.float32(momentum)
    eps32 = np.float32(EPS)
    mean = sums[:C] / count
    raw_var = sums[C:] / count - mean * mean
    var = np.maximum(raw_var, 0.0)
    rstd = 1.0 / np.sqrt(var + np.float64(eps32))
    unb = var * count / (count - 1.0) if count > 1 else var
    mean32, rstd32 = mean.astype(np.float32), rstd.astype(np.float32)
    r = torch.rand(6, C, generator=g, dtype=F64).numpy()
    sgn = np.where(mean < 0, -1.0, 1.0)
    rmean = (sgn * (np.abs(mean) * (1 + r[0]) + 0.1)).astype(np.float32)
    rvar = (unb * (1 + r[1]) + 0.1).astype(np.float32)
    om32 = np.float32(1.0) - m32                                                  # the kernel's (1.0f - momentum): one IEEE f32 operation
    rmean_ref = np.float64(om32) * rmean.astype(np.float64) + np.float64(m32) * mean
    rvar_ref = np.float64(om32) * rvar.astype(np.float64) + np.float64(m32) * unb
    gamma = ((0.5 + r[2]) * np.where(r[3] < 0.3, -1.0, 1.0)).astype(np.float32)
    w = ((r[4][:, None] - 0.5) * 2 + np.linspace(-1, 1, 9)[None, :]).astype(np.float32)      # [C][9]
    b = ((r[5] - 0.5) * 4).astype(np.float32)
    # folded parameters: "the same expression in float64" takes the kernel's own f32 mean / rstd as its inputs
    sc = gamma.astype(np.float64) * rstd32.astype(np.float64)
    p = (b.astype(np.float64) - mean32.astype(np.float64)) * sc
    beta = (np.where(p < 0, -1.0, 1.0) * (3 * np.abs(p) + 0.25)).astype(np.float32)
    wf_ref = w.astype(np.float64) * sc[:, None]
    bf_ref = p + beta.astype(np.float64)
    return SimpleNamespace(C=C, count=count, momentum=float(m32), eps=float(eps32), sums=sums, const=const, raw_var=raw_var, mean=mean, rstd=rstd,
                           unb=unb, rmean=rmean, rvar=rvar, rmean_ref=rmean_ref, rvar_ref=rvar_ref, gamma=gamma, beta=beta, w=w, b=b,
                           wf_ref=wf_ref, bf_ref=bf_ref, p=p, om32=om32)


def assert_bn_finalize_conditions(P):
    """what the 2-ulp bounds need (see the derivation in tests/test_gpu_train_cnn.py)"""
    if P.count in (7, 1000):                  # (with a count of 1 or 2 the sums of a constant are exact and the raw variance is exactly zero)
        assert P.const is not None and P.raw_var[0] < 0.0, "channel 0 was meant to have a raw variance below zero"
        assert P.rstd[0] == 1.0 / np.sqrt(np.float64(np.float32(EPS)))
    a, b = np.float64(P.om32) * P.rmean.astype(np.float64), P.momentum * P.mean
    assert np.all(a * b >= 0) and np.all(np.abs(b) <= np.abs(a)), "running_mean update would cancel"
    a, b = np.float64(P.om32) * P.rvar.astype(np.float64), P.momentum * P.unb
    assert np.all(a > 0) and np.all(b >= 0) and np.all(b <= a), "running_var update would cancel"
    assert np.all(P.p * P.beta >= 0) and np.all(np.abs(P.beta) >= 3 * np.abs(P.p)), "b_folded would cancel"
    if P.count in (2, 7):
        assert np.all(P.unb[1:] >= P.raw_var[1:] * 1.16), "biased and unbiased variance were meant to differ by a large factor"


# ------------------------------------------------------------------ 3. mt_bn_stats_cl
def bn_stats_rows(C):
    return 256 // (C // 8)


def bn_stats_ns(C):
    R = bn_stats_rows(C)
    return [1, R - 1, R + 1, 3 * R + 5, 16 * R + 3]          # 3R + 5: one workgroup, the fourth row in flight is out of range for most threads


def bn_stats_case(N, C, seed=0):
    g = _gen(3000 + seed + N + 31 * C)
    z = randint(g, -8, 8, (N, C))
    sums = torch.cat([z.sum(0), (z * z).sum(0)])
    return SimpleNamespace(N=N, C=C, z=z, sums=sums, units=int((z * z).sum(0).max()))


# ------------------------------------------------------------------ 4. mt_bn_relu_pool_apply
BN_APPLY_SHAPES = [(1, 2, 1, 0), (3, 5, 7, 0), (1, 4, 9, 8), (3, 7, 11, 24)]     # (B, F, T, extra columns of ldx)


def bn_apply_reference(z, mean, rstd, gamma, beta):
    """z [B][F][T][64] float64 -> float64 [B][F/2][T][64]: max over the row pair of relu(gamma*(z - mean)*rstd + beta)"""
    Fo = z.shape[1] // 2
    y = torch.relu(gamma * (z - mean) * rstd + beta)
    return torch.maximum(y[:, 0:2 * Fo:2], y[:, 1:2 * Fo:2])


def bn_apply_case(B, F, T, ties=False, seed=0):
    """exact case: integer z in [-15, 15], rstd a power of two, gamma in {0, +-1, +-2, +-1/2} / rstd-compatible, integer mean, half-integer
    beta: gamma*rstd, mean*gamma*rstd, the shift and the fused multiply-add are exact and the result is a multiple of 1/2 below 2^7.
    ties: z integers of magnitude 128..255 (bf16 spacing 1), gamma = rstd = 1, mean = 0, beta in {1/2, 1/4, 3/4, -1/2, ...}: results on and
    next to round-to-nearest-even ties of bf16.  The dropped last row of an odd F holds NaN."""
    g = _gen(4000 + seed + B + 5 * F + 7 * T + (100 if ties else 0))
    C = 64
    if not ties:
        z = randint(g, -15, 15, (B, F, T, C), nonzero=True)
        sc = torch.tensor([1, -1, 2, -2, 0.5, -0.5, 0, 1])[torch.arange(C) % 8].to(F64)          # gamma * rstd
        rstd = torch.tensor([0.5, 1, 2, 0.25])[(torch.arange(C) // 8) % 4].to(F64)
        gamma = sc / rstd
        mean = randint(g, -3, 3, (C,))
        beta = randint(g, -8, 8, (C,)) / 2
        beta[40:48] = -40.0                                                                         # eight channels where both rows are negative
    else:
        z = randint(g, 128, 255, (B, F, T, C)) * torch.where(torch.rand(B, F, T, C, generator=g) < 0.25, -1.0, 1.0).to(F64)
        gamma, rstd, mean = torch.ones(C, dtype=F64), torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
        beta = torch.tensor([0.5, 0.25, 0.75, -0.5, 0.5, -0.25, 0.0, -0.75])[torch.arange(C) % 8].to(F64)
    ref = bn_apply_reference(z, mean, rstd, gamma, beta)
    if F % 2:
        z = z.clone()
        z[:, F - 1] = float("nan")
    return SimpleNamespace(B=B, F=F, T=T, z=z, mean=mean, rstd=rstd, gamma=gamma, beta=beta, ref=ref, ties=ties)


def assert_bn_apply_exact(P):
    """the affine map is exact in f32: gamma*rstd, mean*(gamma*rstd), beta - that and z*(gamma*rstd) + shift are all dyadic numbers of fewer
    than 24 bits; outside the tie case the result is a bf16 value already"""
    sc = P.gamma * P.rstd
    sh = P.beta - P.mean * sc
    Fo = P.F // 2
    zz = P.z[:, :2 * Fo]
    a = zz * sc + sh
    for v in (sc, P.mean * sc, sh, a):
        assert torch.equal((v * 8).round(), v * 8) and float(v.abs().max()) * 8 < 2 ** 24
    assert is_bf16(zz)
    if not P.ties:
        assert is_bf16(P.ref), "a result is not a bf16 value"
        neg = (a[:, 0::2] < 0) & (a[:, 1::2] < 0)
        assert bool(neg[..., 40:48].all()) and bool((sc < 0).any()) and bool((sc == 0).any())
        assert float((P.ref > 0).double().mean()) > 0.25
    else:
        r = P.ref[P.ref > 0]
        on_tie = (r * 2 == (r * 2).round()) & (r != r.round())
        assert int(on_tie.sum()) > r.numel() // 8 and int((~on_tie).sum()) > r.numel() // 8


# ------------------------------------------------------------------ 5 / 6. BN + ReLU + pool backward
def batch_stats(z):
    """z [B][F][T][C] float64 -> per-channel mean and 1/sqrt(biased variance + eps)"""
    mean = z.mean((0, 1, 2))
    var = ((z - mean) ** 2).mean((0, 1, 2))
    return mean, 1.0 / torch.sqrt(var + float(np.float32(EPS)))


def pool_bwd_closed(z, g, gamma, beta, tie=None):
    """Closed form of d/dz of sum(g * MaxPool2d((2,1))(ReLU(BN_batch(z)))) in float64.  z [B][F][T][C], g [B][F/2][T][C].
    Routing: the pair's larger post-BN value takes g if it is positive; a tie goes to the FIRST row.  tie = (gt, lt), boolean [B][F/2][T][C]:
    the order of the rows' pre-BN values before they were rounded to bf16; the second row wins where gamma*rstd > 0 and lt, or gamma*rstd < 0
    and gt.  Returns every intermediate: the tolerances of the GPU tests are computed from them."""
    B, F, T, C = z.shape
    Fo, N = F // 2, B * F * T
    mean, rstd = batch_stats(z)
    xhat = (z - mean) * rstd
    y = gamma * xhat + beta
    y0, y1 = y[:, 0:2 * Fo:2], y[:, 1:2 * Fo:2]
    if tie is None:
        second = y1 > y0
    else:
        k = (gamma * rstd).expand_as(y0)
        second = torch.where(k > 0, tie[1], torch.where(k < 0, tie[0], torch.zeros_like(tie[0])))
    dy = torch.zeros_like(z)
    dy[:, 0:2 * Fo:2] = torch.where(~second & (y0 > 0), g, torch.zeros_like(g))
    dy[:, 1:2 * Fo:2] = torch.where(second & (y1 > 0), g, torch.zeros_like(g))
    dbeta = dy.sum((0, 1, 2))
    dgamma = (dy * xhat).sum((0, 1, 2))
    k = gamma * rstd
    dz = k * (dy - dbeta / N - xhat * dgamma / N)
    return SimpleNamespace(N=N, mean=mean, rstd=rstd, xhat=xhat, y=y, dy=dy, dbeta=dbeta, dgamma=dgamma, k=k, dz=dz, second=second)


def dz_xhat_residual(R):
    """sum dz*xhat per channel.  BatchNorm makes it k dgamma (1 - sum xhat^2 / N), and sum xhat^2 / N = var / (var + eps): the sum is
    k dgamma eps rstd^2 -- zero but for eps, and known exactly."""
    return R.k * R.dgamma * float(np.float32(EPS)) * R.rstd * R.rstd


def pool_bwd_autograd(z, g, gamma, beta):
    """The same by torch autograd in float64: BatchNorm with batch statistics (functions of z), ReLU, MaxPool2d((2, 1)), contracted with g."""
    z = z.clone().requires_grad_(True)
    gamma = gamma.clone().requires_grad_(True)
    beta = beta.clone().requires_grad_(True)
    mean, rstd = batch_stats(z)
    y = torch.relu(gamma * (z - mean) * rstd + beta)                              # [B][F][T][C]
    pooled = TF.max_pool2d(y.permute(0, 3, 1, 2), (2, 1)).permute(0, 2, 3, 1)     # [B][F/2][T][C]
    (pooled * g).sum().backward()
    return z.grad, gamma.grad, beta.grad


def separation(y, z, gamma):
    """smallest distance of a post-BN value to zero, and to its pool partner where the two are not exactly tied (equal z, or gamma = 0 where
    y = fma(0, xhat, beta) = beta: tied in any arithmetic)"""
    Fo = y.shape[1] // 2
    d0 = float(y.abs().min())
    dy = (y[:, 0:2 * Fo:2] - y[:, 1:2 * Fo:2]).abs()
    ne = (z[:, 0:2 * Fo:2] != z[:, 1:2 * Fo:2]) & (gamma != 0)
    return d0, (float(dy[ne].min()) if bool(ne.any()) else float("inf"))


def assert_separated(R, z, gamma):
    d0, dp = separation(R.y, z, gamma)
    assert d0 >= SEP and dp >= SEP, f"post-BN values {d0:.2e} from zero / {dp:.2e} from their partner: routing could depend on f32 rounding"
    # the kernel's y = fma(gamma, xhat32, beta) with xhat32 = (z - mean32)*rstd32: |d xhat| <= u (|mean| rstd + 3 |xhat|) (see dz_tolerance) and
    # one rounding of y itself: far inside the separation
    err = U32 * (gamma.abs() * (R.mean.abs() * R.rstd + 3 * R.xhat.abs()) + R.y.abs())
    assert float(err.max()) < SEP / 4


def dz_tolerance(R, gamma, n_acc):
    """First-order bound on |dz_kernel - dz| per element, from u = 2^-24 times the operations on the path (R: pool_bwd_closed's result;
    n_acc: the number of f32 additions an addend of the pass-1 sums goes through, from the launch geometry).

      xhat = (z - mean32)*rstd32:  mean32 and rstd32 are roundings (u each), the subtraction and the product round once each:
                                   |d xhat| <= u (|mean| rstd + 3 |xhat|) =: u X
      dbeta  = sum dy:             |d| <= n_acc u sum|dy|                              (f64 atomics and the f32 cast: in n_acc)
      dgamma = sum dy*xhat:        |d| <= u sum|dy| X + (n_acc + 1) u sum|dy xhat|     (+1: the product inside the fma is exact, its sum rounds)
      m1 = f32(dbeta / N), m2 = f32(dgamma / N): the above / N plus u |m|
      dz = k (dy - m1 - xhat m2), k = gamma*rstd32 rounded (2 u), three roundings inside the bracket (each at most u times the sum of the
           absolute terms A = |dy| + |m1| + |xhat m2|), one for the product with k:
           |d dz| <= |k| (d m1 + |xhat| d m2 + |m2| u X + 3 u A) + 3 u |dz|
    Returns (tol_dz, tol_dgamma, tol_dbeta)."""
    X = R.mean.abs() * R.rstd + 3 * R.xhat.abs()
    ady = R.dy.abs()
    t_dbeta = n_acc * U32 * ady.sum((0, 1, 2))
    t_dgamma = U32 * (ady * X).sum((0, 1, 2)) + (n_acc + 1) * U32 * (ady * R.xhat.abs()).sum((0, 1, 2))
    m1, m2 = R.dbeta / R.N, R.dgamma / R.N
    dm1, dm2 = t_dbeta / R.N + U32 * m1.abs(), t_dgamma / R.N + U32 * m2.abs()
    A = ady + m1.abs() + (R.xhat * m2).abs()
    t_dz = R.k.abs() * (dm1 + R.xhat.abs() * dm2 + m2.abs() * U32 * X + 3 * U32 * A) + 3 * U32 * R.dz.abs()
    return t_dz, t_dgamma, t_dbeta


POOL_BWD_SHAPES = [(1, 2, 3), (3, 5, 7), (2, 6, 37)]      # (B, F, T): the last one makes every thread loop four times over two workgroups


def pool_bwd_geometry(B, F, T):
    """mt_bn_pool_bwd: 16 positions per workgroup and half pass; -> (workgroups, positions per thread)"""
    n = B * ((F + 1) // 2) * T
    g = min((n + 127) // 128, 4096)
    return g, -(-n // (16 * g))


def pool_bwd_case(B, F, T, with_tie=False, seed=0):
    """z: bf16 values; a fifth of the row pairs have equal z (a tie: first row); channels 0..7 have negative gamma, channel 8 gamma = 0,
    channels 16..23 a beta that puts most outputs below zero.  Values that land within SEP of zero or of their partner are redrawn until none
    is left.  with_tie: order bits as mt_conv_cl_tie writes them -- the bf16 order where the rows differ, a random one of >, <, = where they
    are equal."""
    g = _gen(5000 + seed + B + 5 * F + 7 * T + (100 if with_tie else 0))
    C, Fo = 64, F // 2
    z = bf16_round(torch.randn(B, F, T, C, generator=g, dtype=F64) * 1.5 + 0.3)
    eq = torch.rand(B, Fo, T, C, generator=g) < 0.2
    eq[..., 8] = torch.rand(B, Fo, T, generator=g) < 0.7                           # the gamma = 0 channel: enough equal rows for every order bit
    z[:, 1:2 * Fo:2] = torch.where(eq, z[:, 0:2 * Fo:2], z[:, 1:2 * Fo:2])
    gamma = (0.5 + torch.rand(C, generator=g, dtype=F64)).float().to(F64)
    gamma[:8] = -gamma[:8]
    gamma[8] = 0.0
    beta = (torch.randn(C, generator=g, dtype=F64) * 0.3).float().to(F64)
    beta[8] = 0.5
    beta[16:24] = -1.5
    for _ in range(50):
        mean, rstd = batch_stats(z)
        y = gamma * (z - mean) * rstd + beta
        bad = y.abs() < 2 * SEP
        near = ((y[:, 0:2 * Fo:2] - y[:, 1:2 * Fo:2]).abs() < 2 * SEP) & (z[:, 0:2 * Fo:2] != z[:, 1:2 * Fo:2]) & (gamma != 0)
        bad[:, 1:2 * Fo:2] |= near
        if not bool(bad.any()):
            break
        z = torch.where(bad, bf16_round(torch.randn(B, F, T, C, generator=g, dtype=F64) * 1.5 + 0.3), z)
    dX = torch.randn(B, Fo, T, C, generator=g, dtype=F64).float().to(F64)
    tie = None
    if with_tie:
        z0, z1 = z[:, 0:2 * Fo:2], z[:, 1:2 * Fo:2]
        r = torch.randint(0, 3, z0.shape, generator=g)
        gt = (z0 > z1) | ((z0 == z1) & (r == 1))
        lt = (z0 < z1) | ((z0 == z1) & (r == 2))
        tie = (gt, lt)
    R = pool_bwd_closed(z, dX, gamma, beta, tie)
    return SimpleNamespace(B=B, F=F, T=T, z=z, dX=dX, gamma=gamma, beta=beta, tie=tie, R=R)


def assert_pool_bwd_case(P):
    R, Fo = P.R, P.F // 2
    assert is_bf16(P.z)
    assert_separated(R, P.z, P.gamma)
    z0, z1 = P.z[:, 0:2 * Fo:2], P.z[:, 1:2 * Fo:2]
    y0, y1 = R.y[:, 0:2 * Fo:2], R.y[:, 1:2 * Fo:2]
    if P.B * Fo * P.T >= 20:
        assert bool(((z0 == z1) & (y0 > 0))[..., 9:].any()), "no tied pair with a gradient"
        assert bool(((y0 < 0) & (y1 < 0)).any()), "no pair without a gradient"
        assert bool((R.dy[:, 1:2 * Fo:2] != 0).any()) and bool((R.dy[:, 0:2 * Fo:2] != 0).any())
    assert bool((P.gamma < 0).any()) and bool((P.gamma == 0).any())
    if P.tie is not None:
        gt, lt = P.tie
        assert not bool((gt & lt).any())
        assert bool(torch.equal(gt | (z0 == z1), z0 >= z1)) and bool(torch.equal(lt | (z0 == z1), z0 <= z1))
        if P.B * Fo * P.T >= 20:
            for sel in (P.R.k > 0, P.R.k < 0, P.R.k == 0):                         # every branch of the select, on rows of equal bf16 z
                for bits in (gt, lt):
                    assert bool(((z0 == z1) & bits)[..., sel].any())


def pack_tie_words(tie):
    """(gt, lt) boolean [B][Fo][T][C] -> int32 words tie[(((b*Fo + fo)*T + t)*(C/32) + c/32)*2 + {0, 1}], bit c % 32"""
    out = []
    for bits in tie:
        B, Fo, T, C = bits.shape
        b = bits.reshape(B, Fo, T, C // 32, 32).numpy().astype(np.uint64)
        out.append((b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32))
    return torch.from_numpy(np.stack(out, axis=-1).view(np.int32).copy())           # [B][Fo][T][C/32][2]


# ------------------------------------------------------------------ 6. mt_conv1_bwd
CONV1_BWD_SHAPES = [(1, 2, 1), (1, 2, 2), (1, 3, 1), (3, 5, 7), (2, 9, 150)]      # (B, F, T); the last: 1500 positions, six per thread


def conv1_bwd_geometry(B, F, T):
    """mt_conv1_bwd: 256 threads, 8 positions per thread, at most 512 workgroups -> (workgroups, positions per thread)"""
    n = B * ((F + 1) // 2) * T
    g = max(1, min((n + 2047) // 2048, 512))
    return g, -(-n // (256 * g))


def conv1_forward(x, w, bias):
    """x [B][F][T] -> z [B][F][T][32] channels-last (float64)"""
    return TF.conv2d(x[:, None], w.reshape(32, 1, 3, 3), bias, padding=1).permute(0, 2, 3, 1).contiguous()


def conv1_bwd_case(B, F, T, seed=0):
    """x: integers in [-3, 3]; w, bias: multiples of 1/8 in [-1, 1]: z is a multiple of 1/8 below 2^5, exact in f32 whatever the order of the
    nine fused multiply-adds.  Post-BN values of a channel are gamma*rstd*(z - z*) with z* = mean - beta/(gamma*rstd): |gamma| >= 1/2 keeps
    partners with different z at least |gamma| rstd / 8 apart, and beta is chosen so that z* lies half way between two multiples of 1/8, which
    keeps every value |gamma| rstd / 16 from zero.  Channel 5 has gamma = 0 (every pair tied at y = beta > 0); channels 0..3 negative gamma.
    With F >= 5 rows 1..4 of sample 0 are copies of one row, so the pair (2, 3) is tied in every channel."""
    g = _gen(6000 + seed + B + 5 * F + 7 * T)
    x = randint(g, -3, 3, (B, F, T))
    if F >= 5:
        x[0, 1:5] = x[0, 1]
    w = randint(g, -8, 8, (32, 9), nonzero=True) / 8
    bias = randint(g, -8, 8, (32,)) / 8
    z = conv1_forward(x, w, bias)
    mean, rstd = batch_stats(z)
    gamma = (0.5 + torch.rand(32, generator=g, dtype=F64)).float().to(F64)
    gamma[:4] = -gamma[:4]
    gamma[5] = 0.0
    zstar = (torch.floor(8 * mean + torch.randint(-3, 4, (32,), generator=g)) + 0.5) / 8
    k = gamma * rstd
    beta = (k * (mean - zstar)).float().to(F64)
    beta[5] = 0.5
    da = bf16_round(torch.randn(B, F // 2, T, 32, generator=g, dtype=F64))
    R = pool_bwd_closed(z, da, gamma, beta)
    # dW[c][kh*3+kw] = sum dz[b][f][t][c] x[b][f+kh-1][t+kw-1]; the sums of absolute addends go with the tolerances
    xp = TF.pad(x, (1, 1, 1, 1))
    taps = torch.stack([xp[:, kh:kh + F, kw:kw + T] for kh in range(3) for kw in range(3)], -1)       # [B][F][T][9]
    return SimpleNamespace(B=B, F=F, T=T, x=x, w=w, bias=bias, z=z, gamma=gamma, beta=beta, da=da, R=R, taps=taps)


def conv1_bwd_autograd(P):
    """conv(1 -> 32, 3x3, pad 1), BatchNorm with batch statistics, ReLU, MaxPool2d((2,1)), contracted with da: float64 autograd"""
    w, bias, gamma, beta = (v.clone().requires_grad_(True) for v in (P.w, P.bias, P.gamma, P.beta))
    z = conv1_forward(P.x, w, bias)
    mean, rstd = batch_stats(z)
    y = torch.relu(gamma * (z - mean) * rstd + beta)
    pooled = TF.max_pool2d(y.permute(0, 3, 1, 2), (2, 1)).permute(0, 2, 3, 1)
    (pooled * P.da).sum().backward()
    return w.grad, bias.grad, gamma.grad, beta.grad


def assert_conv1_bwd_case(P):
    z8 = P.z * 8
    assert torch.equal(z8, z8.round()) and float(z8.abs().max()) < 2 ** 24, "the recomputed z would not be exact in f32"
    assert is_bf16(P.da)
    assert_separated(P.R, P.z, P.gamma)
    if P.F >= 5:
        Fo = P.F // 2
        tied = (P.z[:, 0:2 * Fo:2] == P.z[:, 1:2 * Fo:2]) & (P.R.y[:, 0:2 * Fo:2] > 0) & (P.da != 0)
        assert bool(tied[..., 6:].any()), "no tied pair with a gradient"
        assert bool((P.R.dy[:, 1:2 * Fo:2] != 0).any())


def conv1_bwd_tolerances(P, n_pos):
    """(tol_dW [32][9], tol_db, tol_dgamma, tol_dbeta, sum|dz|).  n_pos: positions per thread.  Pass-1 sums go through n_pos additions in the
    thread, 6 in the wave, 2 across the waves and the f32 cast: n_acc = n_pos + 9.  dW and db accumulate two terms per position (2 n_pos + 9
    roundings): |d dW| <= sum tol_dz |x_tap| + (2 n_pos + 9) u sum |dz x_tap|, and db likewise with x_tap = 1."""
    t_dz, t_dgamma, t_dbeta = dz_tolerance(P.R, P.gamma, n_pos + 9)
    n2 = (2 * n_pos + 9) * U32
    at = P.taps.abs()
    t_dW = torch.einsum("bftc,bftk->ck", t_dz, at) + n2 * torch.einsum("bftc,bftk->ck", P.R.dz.abs(), at)
    sabs = P.R.dz.abs().sum((0, 1, 2))
    t_db = t_dz.sum((0, 1, 2)) + n2 * sabs
    return t_dW, t_db, t_dgamma, t_dbeta, sabs


# ------------------------------------------------------------------ 7. mt_rowsum_bf16
ROWSUM_NS = [1, 7, 8, 9, 511, 512, 513, 16384, 16385, 2 * 16384 + 5]
ROWSUM_ROWS = [1, 4, 5, 88]


def rowsum_case(rows, n, seed=0):
    g = _gen(7000 + seed + rows + 3 * n)
    a = randint(g, -4, 4, (rows, n), nonzero=True)
    return SimpleNamespace(rows=rows, n=n, a=a, sums=a.sum(1), units=int(a.abs().sum(1).max()))


# ------------------------------------------------------------------ 8. mt_dlogits_pack / _heads
def rounding_values(shape, seed=0):
    """f32 values (as float32 tensor) of which a third sit exactly on bf16 round-to-nearest-even ties, a third one f32 step beside a tie and a
    third anywhere; both signs"""
    g = _gen(8000 + seed + int(np.prod(shape)))
    n = int(np.prod(shape))
    base = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).float()
    bits = base.view(torch.int32)
    kind = torch.randint(0, 3, (n,), generator=g)
    step = torch.randint(0, 2, (n,), generator=g) * 2 - 1
    tied = bits + 0x8000                                                            # half a bf16 step above |base|: a tie
    v = torch.where(kind == 0, tied, torch.where(kind == 1, tied + step, bits + torch.randint(0, 0x10000, (n,), generator=g).int()))
    out = v.int().view(torch.float32).reshape(shape).clone()
    assert bool(torch.isfinite(out).all())
    return out


def on_bf16_tie(v):
    return (v.view(torch.int32) & 0xFFFF) == 0x8000
