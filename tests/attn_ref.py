"""Input generators, float64 references, bound functions and float32 emulations for the attention, LayerNorm and head kernels of
csrc/attn.hip, csrc/attn_fused.hip and csrc/train_large.hip (tests/test_gpu_attn.py).

CPU only: torch on the CPU and numpy; nothing of the package's GPU side is imported.  Every generator is deterministic (seeded) and returns
a SimpleNamespace with the inputs as the kernel takes them (16-bit and f32 values kept in float64 tensors that hold representable values),
and the float64 reference.  The bound functions return one bound PER OUTPUT ELEMENT, built from the unit roundoffs of the formats
(u16 = 2^-11 for f16, 2^-8 for bf16, u32 = 2^-24) and from the operation counts of the kernels; DESIGN 6i holds the derivations.
The `emulate_*` functions redo the kernels' arithmetic in float32 with the kernels' order of operations where it matters, and take a
`mutate=` switch that plants one wrong line each (tests/test_attn_ref_cpu.py runs the table: the plain emulation must fit the bounds, every
mutation must break one).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

U32 = 2.0 ** -24
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUB16 = {"f16": 2.0 ** -25, "bf16": 0.0}          # half the f16 subnormal spacing: the absolute rounding error of a tiny f16 result
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
F64, F32 = torch.float64, torch.float32
GRID_CAP = 16384 * 256                            # threads of the element-wise kernels' largest grid (grid_for in train_large.hip)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def r16(x, dt):
    """round-to-nearest-even to the 16-bit type, returned in float64"""
    return x.to(F32).to(TDT[dt]).to(F64)


def r32(x):
    return x.to(F32).to(F64)


def ru(a, b):
    return (a + b - 1) // b * b


def ulps32(got, ref64):
    """|got - ref| in units of the f32 spacing at ref"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    sp = np.spacing(np.abs(ref64.astype(np.float32))).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) / sp


def ulps16(got, ref64, dt):
    """|got - ref| in units of the 16-bit type's spacing at ref (torch tensors, float64)"""
    a = r16(ref64, dt).abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126)))
    bits = 10 if dt == "f16" else 7
    sp = torch.pow(torch.tensor(2.0, dtype=F64), torch.clamp(e, min=-14.0 if dt == "f16" else -126.0) - bits)
    return (got.to(F64) - ref64).abs() / sp


# ------------------------------------------------------------------ dropout_keep of csrc/mt_common.h
def dropout_keep(seed, layer, idx, p):
    """vectorised uint64 replica: idx an integer array -> bool array (True: the element is kept)"""
    G, MASK = 0x9E3779B97F4A7C15, (1 << 64) - 1
    c = (((((seed << 8) ^ layer) & MASK) * G) + G) & MASK
    with np.errstate(over="ignore"):
        z = np.asarray(idx).astype(np.uint64) + np.uint64(c)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0) >= np.float32(p)


def dropout_keep_scalar(seed, layer, idx, p):
    """the same in Python integers, one element: the check of the vectorised form"""
    G, MASK = 0x9E3779B97F4A7C15, (1 << 64) - 1
    z = (idx + ((((seed << 8) ^ layer) & MASK) * G) + G) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return np.float32(z >> 40) * np.float32(1.0 / 16777216.0) >= np.float32(p)


# ================================================================== 1. fused attention
def af_pi(r):
    return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)


FUSED_TS = [1, 5, 8, 12, 31, 32, 33, 40, 56, 63, 64, 65, 97, 129, 255, 256, 257, 513]
_BH = [(3, 2), (1, 2), (3, 1), (1, 1)]


def fused_cases():
    """(dt, dp, T, B, heads): every T with dp = 192 in both types, every dp with T in {1, 40, 65, 257}; B in {1, 3}, heads in {1, 2}"""
    out = []
    for dt in ("f16", "bf16"):
        for i, T in enumerate(FUSED_TS):
            out.append((dt, 192, T) + (_BH[0] if T == 1 else _BH[i % 4]))
        for dp in (64, 128):
            for i, T in enumerate((1, 40, 65, 257)):
                out.append((dt, dp, T) + (_BH[0] if T == 1 else _BH[(i + dp // 64) % 4]))
    return out


def pi_mask_differs(T):
    """does {r : af_pi(r) < kleft} differ from {r : r < kleft} in the last sub-block of a T-key row?"""
    kleft = T % 32
    return kleft != 0 and {r for r in range(32) if af_pi(r) < kleft} != set(range(kleft))


def fused_case(dt, dp, T, B, heads, seed=0):
    """q, k, v [T][B][heads][dp] (16-bit values).  The score of (query i, key j) is c_i + noise: c_i = +clip, -clip or 0 by
    (i + b + head) % 3, noise of standard deviation 1/6 -- so the probabilities of one row stay within a small factor of each other (every
    key of every row carries weight: `fused_key_visibility`) while a third of the rows straddle each clamp.  v: columns d < dp/2 dense,
    magnitude in [0.5, 1.5) with random sign; columns d >= dp/2 hold +-1 at d = dp/2 + j % (dp/2) and 0 elsewhere, so that the bound of such
    an output column (a sum over the few keys that reach it) stays below what any one of those keys contributes."""
    g = _gen(1000 * T + dp + 7 * B + heads + seed + (0 if dt == "f16" else 500000))
    scale, clip = dp ** -0.5, 10.0
    Ca = heads * dp + 8
    shp = (T, B, heads, dp)
    q = (torch.rand(shp, generator=g, dtype=F64) - 0.5)
    k = (torch.rand(shp, generator=g, dtype=F64) * 2 - 1)
    t, b, h = np.ogrid[:T, :B, :heads]
    kind = torch.from_numpy(((t + b + h) % 3).astype(np.int64))
    c = torch.where(kind == 0, clip, torch.where(kind == 1, -clip, 0.0)).to(F64)
    q[..., 0] = c / scale
    k[..., 0] = 1.0
    h2 = dp // 2
    v = torch.zeros(shp, dtype=F64)
    sign = torch.randint(0, 2, shp, generator=g).to(F64) * 2 - 1
    v[..., :h2] = (torch.rand((T, B, heads, h2), generator=g, dtype=F64) + 0.5) * sign[..., :h2]
    j = torch.arange(T)
    v[j, :, :, h2 + j % h2] = sign[j, :, :, 0]
    q, k, v = r16(q, dt), r16(k, dt), r16(v, dt)
    P = SimpleNamespace(dt=dt, dp=dp, T=T, B=B, heads=heads, scale=scale, clip=clip, Ca=Ca, ld3=2 * Ca + heads * dp + 8, ldo=heads * dp + 8,
                        Tp=ru(T, 64), dpr=ru(dp, 128), q=q, k=k, v=v)
    fused_reference(P)
    return P


def fused_reference(P):
    """float64: scale, clamp at +-clip, softmax over exactly T keys, P V.  Also the pieces the bound needs."""
    q, k, v = (x.permute(1, 2, 0, 3) for x in (P.q, P.k, P.v))                    # [B][heads][T][dp]
    s = torch.matmul(q, k.transpose(-1, -2)) * P.scale
    P.s = s
    x = torch.clamp(s, -P.clip, P.clip)
    e = torch.exp(x)
    p = e / e.sum(-1, keepdim=True)
    P.p, P.x = p, x
    P.ref = torch.matmul(p, v)                                                     # [B][heads][T][dp]
    P.absref = torch.matmul(p, v.abs())
    P.sabs = torch.matmul(q.abs(), k.abs().transpose(-1, -2)) * P.scale            # sum_k |q_ik k_jk| scale
    return P


def fused_bound(P, w32=1.0):
    """per output element [B][heads][T][dp]; A = sum_j p_ij |v_jd|
      u16 A                 P is rounded to 16 bits before P V (each p_j relatively by u16), the row sum is taken from the unrounded p
      u16 |ref| (+ SUB16)   the output's rounding
      (eps_i + (2T + 4) u32)(A + |ref|)   f32: eps_i = max_j [dp u32 sabs_ij + 4 u32 (|x_ij| log2e + 2) + 4 u32], the relative error of p_ij --
                            the score's dp-term f32 accumulation, the roundings of (s c + 1) in the exponent (absolute error in the exponent
                            = relative error behind exp), 2 ulp for v_exp_f32; T u32 for the row sum, T u32 for the P V accumulation, and
                            the division and product at the end"""
    u16 = U16[P.dt]
    eps = (P.dp * U32 * P.sabs + 4 * U32 * (P.x.abs() * 1.4427 + 2) + 4 * U32).amax(-1, keepdim=True)
    return u16 * P.absref + u16 * P.ref.abs() + SUB16[P.dt] + w32 * (eps + (2 * P.T + 4) * U32) * (P.absref + P.ref.abs())


def fused_key_visibility(P, rows=None):
    """min over (row, key) of max_d |change of output (row, d) when key j is left out| / bound(row, d); rows: a sample (None: all).
    Leaving key j out of row i turns ref_id into (ref_id - p_ij v_jd) / (1 - p_ij): a change of p_ij |v_jd - ref_id| / (1 - p_ij)."""
    bound = fused_bound(P)
    v = P.v.permute(1, 2, 0, 3)
    rows = range(P.T) if rows is None else rows
    worst = math.inf
    for i in rows:
        p = P.p[:, :, i, :, None]                                                 # [B][heads][T][1]
        d = p * (v - P.ref[:, :, i, None, :]).abs() / (1 - p)                     # [B][heads][T keys][dp]
        bd = bound[:, :, i, None, :]
        worst = min(worst, float(torch.where(bd > 0, d / bd.clamp(min=1e-300), torch.zeros_like(d)).amax(-1).min()))
    return worst


def fused_sample_rows(T):
    return None if T <= 65 else sorted({0, 1, 2, 31, 32, 33, T // 2, T - 3, T - 2, T - 1})


def clamp_fractions(P):
    return float((P.s > P.clip).double().mean()), float((P.s < -P.clip).double().mean())


def emulate_fused(P, mutate=None):
    """attn_fused_kernel in float32, sub-block by sub-block: row rho of a 32-key sub-block holds key min(kb + af_pi(rho), T-1) and meets
    column kb + af_pi(rho) of V^T (zero from T on); it counts if af_pi(rho) < kleft.  -> [B][heads][T][dp] float64 (16-bit values)
    mutate: 'mask_rho' (rho < kleft), 'skip_partial' (a sub-block with kleft < 32 is skipped), 'count_past_T' (no mask),
            'clamp_after_exp', 'no_clamp', 'sum_rounded_p'"""
    T, dp = P.T, P.dp
    q, k, v = (x.permute(1, 2, 0, 3).to(F32) for x in (P.q, P.k, P.v))
    kkey, vkey, keep = [], [], []
    for kb in range(0, T, 32):
        kleft = T - kb
        if mutate == "skip_partial" and kleft < 32:
            continue
        for rho in range(32):
            kkey.append(min(kb + af_pi(rho), T - 1))
            vkey.append(kb + af_pi(rho))
            keep.append(True if mutate == "count_past_T" else (rho < kleft if mutate == "mask_rho" else af_pi(rho) < kleft))
    if not kkey:
        return torch.full(P.ref.shape, float("nan"), dtype=F64)
    kkey, vkey, keep = torch.tensor(kkey), torch.tensor(vkey), torch.tensor(keep)
    vz = torch.cat([v, torch.zeros(v.shape[:2] + (ru(T, 64) + 64 - T, dp), dtype=F32)], 2)
    s = torch.matmul(q, k.transpose(-1, -2))[..., kkey]                            # f32 accumulation over dp
    log2e = np.float32(1.4426950408889634)
    c, cl = np.float32(np.float32(P.scale) * log2e), np.float32(np.float32(P.clip) * log2e)
    a = s * c
    if mutate == "clamp_after_exp":
        pr = torch.clamp(torch.exp2(a + 1.0), -float(cl), float(cl))
    elif mutate == "no_clamp":
        pr = torch.exp2(a + 1.0)
    else:
        pr = torch.exp2(torch.clamp(a, -float(cl), float(cl)) + 1.0)
    pr = torch.where(keep, pr, torch.zeros_like(pr))
    p16 = pr.to(TDT[P.dt]).to(F32)
    lsum = (p16 if mutate == "sum_rounded_p" else pr).sum(-1, keepdim=True)
    o = torch.matmul(p16, vz[:, :, vkey, :])
    return (o * (1.0 / lsum)).to(TDT[P.dt]).to(F64)


# ------------------------------------------------------------------ mt_attn_transpose_v
TRANSPOSE_V_CASES = [  # (B, T, Tp, heads, dp, use): use 'qkv' (voff = 2 Ca, ld3 > 2 Ca + heads dp), 'v0' (voff 0), 'vca' (voff Ca), 'plain' (ld3 = Ca)
    (1, 1, 64, 1, 24, "qkv"), (3, 65, 128, 2, 96, "qkv"), (1, 130, 192, 2, 64, "v0"), (3, 63, 64, 1, 192, "vca"), (2, 64, 192, 2, 24, "plain"),
    (1, 40, 128, 2, 128, "qkv"),
]


def transpose_v_case(B, T, Tp, heads, dp, use):
    """the 16-bit WORDS encode the position (t, b, head, d) -- a copy may carry any word -- so a misplaced element differs from the right one"""
    Ca = heads * dp if use == "plain" else heads * dp + 8
    ld3 = Ca if use == "plain" else 2 * Ca + heads * dp + 8
    voff = {"qkv": 2 * Ca, "v0": 0, "vca": Ca, "plain": 0}[use]
    t, b, h, d = np.ogrid[:T, :B, :heads, :dp]
    lin = ((t * B + b) * heads + h) * dp + d
    words = (lin * 7919 % 30011 + 1).astype(np.int16)               # 1 .. 30011: never zero, never the sentinel; distinct within 30011 positions
    dpr = ru(dp, 128)
    want = np.zeros((B, heads, dp, Tp), dtype=np.int16)
    want[:, :, :, :T] = words.transpose(1, 2, 3, 0)
    return SimpleNamespace(B=B, T=T, Tp=Tp, heads=heads, dp=dp, dpr=dpr, ld3=ld3, voff=voff, words=words, want=want)


def emulate_transpose_v(P, prefill, mutate=None):
    """-> [B][heads][dpr][Tp] int16 words over `prefill`; mutate: 'no_zero_fill' (columns T..Tp-1 are left alone)"""
    out = np.full((P.B, P.heads, P.dpr, P.Tp), prefill, dtype=np.int16)
    out[:, :, :P.dp, :P.T] = P.words.transpose(1, 2, 3, 0)
    if mutate != "no_zero_fill":
        out[:, :, :P.dp, P.T:] = 0
    return out


# ================================================================== 2. unfused softmax: forward, train forward, backward
SOFTMAX_SHAPES = [(1, 1, 0), (5, 63, 0), (9, 64, 64), (1, 65, 0), (9, 130, 0), (5, 130, 64), (5, 1, 64)]       # (rows, T, Tp - roundup(T, 64))
SOFTMAX_PS = [0.0, 0.25, 0.5]
CLIP_SEP = 1e-4


def _nacc_row(T):
    return (T + 63) // 64 + 6            # additions on the way of one addend: the lane's strided loop, six shuffle steps


def softmax_case(rows, T, extra, scale=0.125, clip=10.0, edge=False, seed=0):
    """S f32 [rows][T] with S*scale in about +-(clip + 4): both clamps are reached (asserted by the CPU tests for T > 1); dPd f32 of order 1.
    edge (scale 0.25, clip 10): row 0 starts with S = 40, -40, nextafter(40, inf), nextafter(-40, -inf)"""
    g = _gen(77 * rows + T + extra + seed + (9000 if edge else 0))
    S = ((torch.rand((rows, T), generator=g, dtype=F64) * 2 - 1) * (clip + 4) / scale)
    if T > 1:
        S[:, 0], S[:, 1] = (clip + 3) / scale, -(clip + 3) / scale
    S = r32(S)
    if edge:
        assert scale == 0.25 and clip == 10.0 and T >= 8
        e = np.float32(40.0)
        S[0, :4] = torch.tensor([40.0, -40.0, float(np.nextafter(e, np.float32(np.inf))), float(np.nextafter(-e, np.float32(-np.inf)))], dtype=F64)
        S[0, 4:8] = torch.tensor([39.0, -39.0, 38.5, 37.0], dtype=F64)            # so that row 0's probabilities at the edge are not negligible
    dP = r32(torch.randn((rows, T), generator=g, dtype=F64))
    return SimpleNamespace(rows=rows, T=T, Tp=ru(T, 64) + extra, lds=T + 3, ldp=T + 5, scale=scale, clip=clip, S=S, dP=dP, edge=edge)


def softmax_reference(P):
    x = torch.clamp(P.S * float(np.float32(P.scale)), -P.clip, P.clip)
    e = torch.exp(x)
    return e / e.sum(-1, keepdim=True)


def softmax_keep(P, p, seed, layer, stride=None):
    """the mask of element (row, j): dropout_keep(seed, layer, row T + j, p)"""
    r, j = np.ogrid[:P.rows, :P.T]
    return torch.from_numpy(dropout_keep(seed, layer, r * (P.T if stride is None else stride) + j, p))


def _eps_p(P):
    """relative f32 error of one probability: the product s*scale (u32 |x|) and the scaling by log2 e inside __expf (2 u32 |x|) act as
    absolute errors of the exponent, 2 ulp (4 u32) for the hardware exponential; the same again for the row sum's addends, plus its
    n_acc additions, the reciprocal (IEEE, u32; 3 u32 allowed) and the product (u32)"""
    one = 3 * P.clip * U32 + 4 * U32
    return 2 * one + (_nacc_row(P.T) + 4) * U32


def softmax_fwd_bound(P, ref, dt, p=0.0, w32=1.0):
    """u16 ref + f32 term (+ the f16 subnormal rounding 2^-25); ref: the kept values ref / (1 - p) when dropout is on (two more roundings)"""
    return U16[dt] * ref + w32 * (_eps_p(P) + (2 * U32 if p > 0 else 0)) * ref + SUB16[dt]


def softmax_bwd_reference(P, p, keep):
    """float64 autograd of dropout(softmax(clamp(S scale))) with the replica's mask -> dS"""
    S = P.S.clone().requires_grad_(True)
    x = torch.clamp(S * float(np.float32(P.scale)), -P.clip, P.clip)
    pr = torch.softmax(x, -1)
    out = pr * keep.to(F64) / (1 - float(np.float32(p))) if p > 0 else pr
    out.backward(P.dP)
    return S.grad


def softmax_bwd_bound(P, ref, p, keep, w32=1.0):
    """u_bf16 |ref| + c u32 p_j (|dP_j| + sum_k |dP_k| p_k) scale: dP_j - dot cancels, so the error is relative to the addends.
    c = eps_p / u32 (p_j and the p_k inside dot) + n_acc + 1 (dot's additions and fma) + 6 (dropout scaling, difference, two products, ks)"""
    pr = softmax_reference(P)
    dP = P.dP * keep.to(F64) / (1 - p) if p > 0 else P.dP
    D = (dP.abs() * pr).sum(-1, keepdim=True)
    c = 2 * _eps_p(P) / U32 + _nacc_row(P.T) + 7
    return U16["bf16"] * ref.abs() + w32 * c * U32 * pr * (dP.abs() + D) * P.scale


def assert_clip_separated(P):
    """but for the entries planted exactly at the edge, no |S scale| within CLIP_SEP of clip: the clamp's gradient mask is the same in f32 and
    in float64"""
    near = ((P.S * float(np.float32(P.scale))).abs() - P.clip).abs() < CLIP_SEP
    if P.edge:
        near[0, :4] = False
    assert not bool(near.any()), "a score within 1e-4 of the clamp"


def emulate_softmax(P, dt="bf16", p=0.0, seed=0, layer=0, mutate=None):
    """attn_softmax_kernel / attn_softmax_train_kernel in float32 -> [rows][Tp] float64 over zeros; mutate: 'index_Tp' (mask index row Tp + j)"""
    s = P.S.to(F32)
    e = torch.exp(torch.clamp(s * np.float32(P.scale), -P.clip, P.clip))
    v = e * (1.0 / e.sum(-1, keepdim=True))
    if p > 0:
        keep = softmax_keep(P, p, seed, layer, stride=P.Tp if mutate == "index_Tp" else None)
        v = torch.where(keep, v * (np.float32(1.0) / (np.float32(1.0) - np.float32(p))), torch.zeros_like(v))
    out = torch.zeros((P.rows, P.Tp), dtype=F64)
    out[:, :P.T] = v.to(TDT[dt]).to(F64)
    return out


def emulate_softmax_bwd(P, p=0.0, seed=0, layer=0, mutate=None):
    """attn_softmax_bwd_kernel in float32; mutate: 'index_Tp', 'clamp_exclusive' (a > -clip && a < clip)"""
    s = P.S.to(F32)
    a = s * np.float32(P.scale)
    e = torch.exp(torch.clamp(a, -P.clip, P.clip))
    pr = e * (1.0 / e.sum(-1, keepdim=True))
    dp = P.dP.to(F32)
    if p > 0:
        keep = softmax_keep(P, p, seed, layer, stride=P.Tp if mutate == "index_Tp" else None)
        dp = torch.where(keep, dp * (np.float32(1.0) / (np.float32(1.0) - np.float32(p))), torch.zeros_like(dp))
    dot = (dp * pr).sum(-1, keepdim=True)
    inside = (a > -P.clip) & (a < P.clip) if mutate == "clamp_exclusive" else (a >= -P.clip) & (a <= P.clip)
    v = torch.where(inside, pr * (dp - dot) * np.float32(P.scale), torch.zeros_like(pr))
    out = torch.zeros((P.rows, P.Tp), dtype=F64)
    out[:, :P.T] = v.to(torch.bfloat16).to(F64)
    return out


# ================================================================== 3. LayerNorm(resid + proj)
LN_NS = [1, 48, 63, 64, 65, 1024, 2047, 2048]
LN_ROWS = [1, 6]
LN_EPS = 1e-5
LN_BWD_SHAPES = [(1, 48), (1024, 48), (1025, 48), (2500, 48), (6, 65), (6, 2048)]            # (rows, n)
LN_SLICES = 1024                                                                             # mt_layernorm_residual_bwd_slices()


def ln_case(rows, n, seed=0, big_mean=True):
    """resid, proj f32 [rows][n], gamma, beta [n].  Even rows (forward cases): mean near 1000, spread near 1 -- a one-pass variance
    E[v^2] - mean^2 loses everything there; odd rows: mean near 3.  gamma in +-[0.5, 1.5], beta of order 1."""
    g = _gen(31 * rows + n + seed)
    z = torch.randn((rows, n), generator=g, dtype=F64)
    m = torch.where(torch.arange(rows) % 2 == 0, 1000.0 if big_mean else -2.0, 3.0).to(F64)[:, None]
    proj = r32(torch.randn((rows, n), generator=g, dtype=F64) * 0.5)
    resid = r32(z + m - proj)
    sg = torch.randint(0, 2, (n,), generator=g).to(F64) * 2 - 1
    gamma = r32((torch.rand(n, generator=g, dtype=F64) + 0.5) * sg)
    beta = r32(torch.randn(n, generator=g, dtype=F64))
    dy = r32(torch.randn((rows, n), generator=g, dtype=F64))
    P = SimpleNamespace(rows=rows, n=n, resid=resid, proj=proj, gamma=gamma, beta=beta, dy=dy, eps=LN_EPS, ldr=n + 1, ldp=n + 2, ldy=n + 3)
    v = resid + proj
    P.v, P.mean = v, v.mean(1, keepdim=True)
    P.var = ((v - P.mean) ** 2).mean(1, keepdim=True)
    P.rstd = 1.0 / torch.sqrt(P.var + float(np.float32(LN_EPS)))
    P.xhat = (v - P.mean) * P.rstd
    P.y = P.xhat * gamma + beta
    return P


def _ln_nacc(n):
    return (n + 63) // 64 + 6


def ln_error_terms(P):
    """first-order f32 error of the kernel's pieces:
      v = fl(a + p): u32 |v|;  mean: (n_acc + 1) u32 mean|v| + u32 |mean| =: dm  (n_acc additions, the inputs' rounding, the division)
      d = v - mean: Delta_j = u32 |v_j| + dm + u32 |d_j|            <- the term in |mean| 2^-24 (times rstd once it reaches y)
      var + eps: relative r_v = [2 sigma rms(Delta) + rms(Delta)^2 + (n_acc + 2) u32 var] / (var + eps) + u32   (Cauchy-Schwarz on sum d_j delta_j)
      rstd: relative r_r = r_v / 2 (1 + r_v) + 4 u32   (rsqrtf within 2 ulp)"""
    na = _ln_nacc(P.n)
    v, d = P.v, P.v - P.mean
    dm = (na + 1) * U32 * v.abs().mean(1, keepdim=True) + U32 * P.mean.abs()
    Delta = U32 * v.abs() + dm + U32 * d.abs()
    rms = torch.sqrt((Delta ** 2).mean(1, keepdim=True))
    eps = float(np.float32(P.eps))
    r_v = (2 * torch.sqrt(P.var) * rms + rms ** 2 + (na + 2) * U32 * P.var) / (P.var + eps) + U32
    r_r = r_v / 2 * (1 + r_v) + 4 * U32
    return dm, Delta, r_v, r_r


def ln_fwd_bound(P, dt, w32=1.0):
    """|gamma_j| rstd [Delta_j + |d_j| (r_r + 2 u32)] + u32 |y_j| + u16 |y_j| (+ the f16 subnormal rounding)"""
    dm, Delta, r_v, r_r = ln_error_terms(P)
    assert float(r_v.max()) < 0.1
    d = (P.v - P.mean).abs()
    return w32 * (P.gamma.abs() * P.rstd * (Delta + d * (r_r + 2 * U32)) + U32 * P.y.abs()) + U16[dt] * P.y.abs() + SUB16[dt]


def ln_stats_ulps(P):
    """allowed distance of stats from the float64 mean and rstd in f32 ulps, per row: an ulp is at least u32 |x|, so a relative error r is
    at most r / u32 ulps; + 1/2 for the rounding of the result itself"""
    dm, Delta, r_v, r_r = ln_error_terms(P)
    return (dm / (U32 * P.mean.abs()) + 0.5).reshape(-1), (r_r / U32 + 0.5).reshape(-1)


def emulate_ln(P, dt="bf16", mutate=None):
    """ln_residual_kernel in float32, the lane-strided partial sums and the shuffle tree included -> (y [rows][n] float64, mean, rstd f32)
    mutate: 'one_pass' (var = E[v^2] - mean^2)"""
    n = P.n
    v = np.zeros((P.rows, 2048), dtype=np.float32)
    v[:, :n] = (P.resid.to(F32) + P.proj.to(F32)).numpy()

    def wave_sum(a):                                    # a [rows][2048]: lane l adds a[l], a[l + 64], ... in order; then the xor tree
        part = np.zeros((a.shape[0], 64), dtype=np.float32)
        for i in range(32):
            part = part + a[:, 64 * i:64 * i + 64]
        for o in (32, 16, 8, 4, 2, 1):
            part = part + part[:, np.arange(64) ^ o]
        return part[:, :1]

    mean = wave_sum(v) / np.float32(n)
    valid = (np.arange(2048) < n)[None, :]
    if mutate == "one_pass":
        var = wave_sum(v * v) / np.float32(n) - mean * mean
    else:
        dl = np.where(valid, v - mean, np.float32(0))
        var = wave_sum(dl * dl) / np.float32(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (np.float32(1) / np.sqrt(var + np.float32(P.eps), dtype=np.float32)).astype(np.float32)
        y = (v[:, :n] - mean) * rstd * P.gamma.to(F32).numpy() + P.beta.to(F32).numpy()
    return torch.from_numpy(y).to(TDT[dt]).to(F64), mean.reshape(-1), rstd.reshape(-1)


def ln_bwd_reference(P):
    """float64 autograd of LayerNorm(resid + proj) -> dx [rows][n], dgamma, dbeta [n]"""
    v = P.v.clone().requires_grad_(True)
    g, b = P.gamma.clone().requires_grad_(True), P.beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(v, (P.n,), g, b, float(np.float32(P.eps)))
    y.backward(P.dy)
    return v.grad, g.grad, b.grad


def ln_bwd_bounds(P, w32=1.0):
    """stats = f32 roundings of the float64 mean / rstd.  X_j = u32 (rstd (|v_j| + |mean|) + 3 |xhat_j|): the error of xhat (v's rounding, the
    rounded mean, the difference, the rounded rstd, the product).  gg = dy gamma (u32 |gg|); s1 = sum gg: n_acc u32 sum|gg|;
    s2 = sum gg xhat: sum |gg| X + (n_acc + 1) u32 sum |gg xhat|; m = s / n (+ u32 |m|);
    dx = rstd (gg - m1 - xhat m2): rstd [u32 |gg| + dm1 + |xhat| dm2 + |m2| X + 3 u32 (|gg| + |m1| + |xhat m2|)] + 2 u32 |dx|.
    dgamma = sum over rows of dy xhat: sum |dy| X + r_max u32 sum |dy xhat| + u32 |.|, r_max = ceil(rows / slices) additions per wave (the
    slices themselves are summed in float64 by the test); dbeta: (r_max - 1) u32 sum |dy|."""
    na = _ln_nacc(P.n)
    X = U32 * (P.rstd * (P.v.abs() + P.mean.abs()) + 3 * P.xhat.abs())
    gg = P.dy * P.gamma
    m1, m2 = gg.mean(1, keepdim=True), (gg * P.xhat).mean(1, keepdim=True)
    dm1 = (na + 1) * U32 * gg.abs().mean(1, keepdim=True) + U32 * m1.abs()
    dm2 = (gg.abs() * X).mean(1, keepdim=True) + (na + 2) * U32 * (gg * P.xhat).abs().mean(1, keepdim=True) + U32 * m2.abs()
    dx = P.rstd * (gg - m1 - P.xhat * m2)
    A = gg.abs() + m1.abs() + (P.xhat * m2).abs()
    b_dx = w32 * P.rstd * (U32 * gg.abs() + dm1 + P.xhat.abs() * dm2 + m2.abs() * X + 3 * U32 * A) + 2 * U32 * dx.abs()
    rmax = (P.rows + LN_SLICES - 1) // LN_SLICES
    b_dg = w32 * (P.dy.abs() * X).sum(0) + rmax * U32 * (P.dy * P.xhat).abs().sum(0)
    b_db = (rmax - 1) * U32 * P.dy.abs().sum(0)
    return b_dx, b_dg, b_db


def emulate_ln_bwd(P, mutate=None):
    """ln_residual_bwd_kernel in float32 (row sums by numpy's pairwise f32 sum: within the bound's n_acc) -> dx, part [slices][2][n]
    mutate: 'no_xhat_m2'"""
    f = np.float32
    v = P.resid.to(F32).numpy() + P.proj.to(F32).numpy()
    mean, rstd = P.mean.to(F32).numpy(), P.rstd.to(F32).numpy()
    xh = (v - mean) * rstd
    d = P.dy.to(F32).numpy()
    gg = d * P.gamma.to(F32).numpy()
    m1 = gg.sum(1, keepdims=True, dtype=f) / f(P.n)
    m2 = (gg * xh).sum(1, keepdims=True, dtype=f) / f(P.n)
    dx = rstd * ((gg - m1) if mutate == "no_xhat_m2" else (gg - m1 - xh * m2))
    part = np.zeros((LN_SLICES, 2, P.n), dtype=f)
    for r in range(P.rows):
        part[r % LN_SLICES, 0] += d[r] * xh[r]
        part[r % LN_SLICES, 1] += d[r]
    return torch.from_numpy(dx).to(F64), torch.from_numpy(part).to(F64)


# ================================================================== 4. element-wise and layout helpers
ELEMENTWISE_SHAPES = [(1, 1, 1), (3, 7, 9), (5, 65, 72), (4100, 1025, 1025)]     # (M, N, ld): the last one: M N = 4 202 500 > 16384 * 256
DROPOUT_F32_NS = [1, 1001, 4195304]
TRANSPOSE_RC = [(1, 1), (63, 130), (64, 64), (65, 63), (130, 65), (1, 130), (65, 1)]


def position_words(M, N):
    """int16 words that encode (m, n), never zero and never the sentinel 0x7BCD: 1 .. 30011"""
    m, n = np.ogrid[:M, :N]
    return ((m.astype(np.int64) * N + n) * 7919 % 30011 + 1).astype(np.int16)


def rows_index(M, N, ld):
    m, n = np.ogrid[:M, :N]
    return m * ld + n


def emulate_rowwise(fn, M, N, prefill, mutate=None):
    """an element-wise kernel's grid-stride loop over M N elements: fn(m, n, i) -> values for the flat element indices i it is given.
    mutate 'one_pass': elements from 16384 * 256 on are never reached (the loop body runs once per thread) -> they keep `prefill`"""
    i = np.arange(M * N, dtype=np.int64)
    out = fn(i // N, i % N, i)
    if mutate == "one_pass" and M * N > GRID_CAP:
        out = out.copy()
        out[GRID_CAP:] = prefill
    return out.reshape(M, N)


def dropout_rows_keep(M, N, p, seed, layer, ld=None, mutate=None):
    """keep mask [M][N]: index m N + n; mutate 'index_ld': m ld + n"""
    m, n = np.ogrid[:M, :N]
    return dropout_keep(seed, layer, m.astype(np.int64) * (ld if mutate == "index_ld" else N) + n, p)


def tie_words_f32(n, seed=0):
    """f32 values a third of which sit exactly on bf16 round-to-nearest-even ties, a third one f32 step beside one, a third anywhere"""
    g = _gen(8000 + seed + n)
    base = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).float()
    bits = base.view(torch.int32)
    kind = torch.randint(0, 3, (n,), generator=g)
    step = torch.randint(0, 2, (n,), generator=g) * 2 - 1
    tied = bits + 0x8000
    v = torch.where(kind == 0, tied, torch.where(kind == 1, tied + step, bits + torch.randint(0, 0x10000, (n,), generator=g).int()))
    out = v.int().view(torch.float32).clone()
    assert bool(torch.isfinite(out).all())
    return out


SPECIALS_F32 = [float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-45, 1.1754942e-38, 0.0, -0.0]
# (the canonical quiet NaN 0x7FC00000 is inside the contract of f32_to_bf16: its carry turns only NaNs whose mantissa bits 15..22 are all
#  ones -- words 0x7FFF8000 and above -- into something else.  DESIGN 6i.)


def f32_to_bf16_reference(src32, alpha):
    """torch's round-to-nearest-even bf16 of the f32 product alpha * src (one f32 rounding, exact for the alphas used: powers of two)"""
    return (src32 * np.float32(alpha)).to(torch.bfloat16)


def bf16_bits(t):
    return t.contiguous().view(torch.int16)
