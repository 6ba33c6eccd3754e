"""Float64 / integer references, input generators, tolerance rules and float32 restatements for the loss, metric and optimizer kernels of
csrc/post.hip and csrc/optim.hip (numpy only).  tests/test_post_optim_ref_cpu.py checks all of it without a GPU; tests/test_gpu_post_optim.py
feeds the same inputs to the kernels through the C ABI.  DESIGN 6j holds the derivations.

A "restatement" below is the kernel's expression written again in numpy float32, operation by operation.  It is not the kernel (numpy's
exp / log1p are not the device's, and numpy does not contract a*b + c), it is the yardstick for a tolerance: a rule that the restatement
needs more than half of is raised to twice what the restatement needs, and the code under test never sets a tolerance."""
import numpy as np

U = 2.0 ** -24                               # half an ulp of a float32 in [1, 2): the unit every rule is stated in
F32, F64 = np.float32, np.float64

BPT = [(1, 1, 1), (2, 5, 7), (3, 88, 501), (9, 88, 33)]          # (3,88,501): 132 264 elements > the loss kernel's 512 x 256 threads
ROWS_T = [(1, 1), (3, 2), (10, 7), (264, 501), (300, 901)]       # 300 x 901 = 270 300 > the 1024 x 256 threads of targets / threshold
PLANTED = [0.0, 1e-7, -1e-7, 20.0, -20.0, 100.0, -100.0]
# |loss - loss64| <= LOSS_K U (weight sum|bce| / denom) and |grad - grad64| <= GRAD_K U |weight / denom|.  The issue's starting values were 8 and
# 4.  The float32 restatement needs 4.4 U of the first (one soft-target element, where max(x,0) - x y cancels and the roundings of its terms
# do not) and 2.7 U of the second (1 + e, the quotient, s - y, the cast of weight / denom and the product round once each), more than half
# of either, so both stand at twice what the restatement needs.
LOSS_K = 9
GRAD_K = 5.5
PREDICT_K = 4                                # cells with |sigmoid64(x) - thr| <= PREDICT_K U are left out
THRESHOLDS = (0.3, 0.5, 0.7)


def f32(x):
    """the float32 nearest to x, as a Python float (what a C `float` argument receives)"""
    return float(F32(x))


def sigmoid64(x):
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(np.isnan(x), np.nan, np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))


# ------------------------------------------------------------------ masked BCE
def valid_mask(lengths, B, P, T):
    if lengths is None:
        return np.ones((B, P, T), dtype=bool)
    L = np.asarray(lengths, dtype=np.int64)
    return np.broadcast_to(np.arange(T)[None, None, :] < L[:, None, None], (B, P, T))


def n_valid_frames(lengths, B, T):
    """as ops.py: sum of clamp(lengths, 0, T), or B T without lengths"""
    return B * T if lengths is None else int(np.clip(np.asarray(lengths, dtype=np.int64), 0, T).sum())


def bce_ref(x, y, lengths, n_valid, weight):
    """-> (loss64, grad64, scale): bce = max(x,0) - x y + log1p(exp(-|x|)) over frames t < lengths[b]; denom = max(n_valid P, 1);
    grad = weight (sigmoid(x) - y) mask / denom; scale = weight sum|bce| / denom, what the loss tolerance is relative to."""
    x, y = np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)
    B, P, T = x.shape
    mask = valid_mask(lengths, B, P, T)
    denom = max(float(n_valid) * P, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        bce = np.where(mask, np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x))), 0.0)
        grad = np.where(mask, weight * (sigmoid64(x) - y) / denom, 0.0)
    return float(weight * bce.sum() / denom), grad, float(weight * np.abs(bce).sum() / denom)


def bce_f32(x, y, lengths, n_valid, weight):
    """the kernel's expressions restated in float32 -> (loss f32, grad f32)"""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    B, P, T = x.shape
    mask = valid_mask(lengths, B, P, T)
    d = max(float(n_valid) * P, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        l = np.maximum(x, F32(0)) - x * y + np.log1p(np.exp(-np.abs(x)))
        s = np.where(mask, l.astype(F64), 0.0).sum()
        gs = F32(float(F32(weight)) / d)
        grad = np.where(mask, gs * (F32(1) / (F32(1) + np.exp(-x)) - y), F32(0)).astype(F32)
    return F32(weight) * F32(s / d), grad


def length_vectors(B, T):
    """length vectors of B entries that between them hold 0, 1, T, T + 5 and -3 (one vector when B >= 5)"""
    vals = [0, 1, T, T + 5, -3, T // 2, T, 2, max(T - 1, 0)]
    out = []
    for i in range(0, 5, B):
        v = vals[i:i + B]
        out.append(np.array(v + [T // 2] * (B - len(v)), dtype=np.int64))
    return out


def bce_inputs(B, P, T, soft=False, seed=0):
    """logits N(0, 3) with the planted values scattered in (where there is room), targets in {0, 1} or, soft, in [0, 1]"""
    rng = np.random.default_rng(1000 + seed + 7 * B + 13 * P + T)
    n = B * P * T
    x = (3.0 * rng.standard_normal(n)).astype(F32)
    if n >= 4 * len(PLANTED):
        x[rng.choice(n, len(PLANTED), replace=False)] = np.array(PLANTED, dtype=F32)
    y = rng.random(n).astype(F32) if soft else (rng.random(n) < 0.3).astype(F32)
    return x.reshape(B, P, T), y.reshape(B, P, T)


def plant_nonfinite(x, y, lengths):
    """copies of x, y with NaN / +Inf / -Inf in masked frames only (both tensors), and zeros there in a second pair -> (xn, yn, xz, yz, count)"""
    B, P, T = x.shape
    dead = ~valid_mask(lengths, B, P, T)
    idx = np.flatnonzero(dead.reshape(-1))
    xn, yn, xz, yz = (a.copy().reshape(-1) for a in (x, y, x, y))
    bad = np.array([np.nan, np.inf, -np.inf], dtype=F32)
    xn[idx] = bad[np.arange(idx.size) % 3]
    yn[idx] = bad[(np.arange(idx.size) + 1) % 3]
    xz[idx] = 0
    yz[idx] = 0
    return xn.reshape(x.shape), yn.reshape(x.shape), xz.reshape(x.shape), yz.reshape(x.shape), int(idx.size)


# ------------------------------------------------------------------ onset / offset targets
def onset_offset_ref(y):
    """y [..., T] -> (onset, offset) in float32: onset[t] = max(y[t] - y[t-1], 0), 0 at t = 0; offset[t] = max(y[t] - y[t+1], 0), 0 at T - 1"""
    y = np.asarray(y, dtype=F32)
    on, off = np.zeros_like(y), np.zeros_like(y)
    on[..., 1:] = np.maximum(y[..., 1:] - y[..., :-1], F32(0))
    off[..., :-1] = np.maximum(y[..., :-1] - y[..., 1:], F32(0))
    return on, off


def roll_inputs(rows, T, binary, seed=0):
    """a roll whose rows alternate between ending in 1 with the next starting in 1, and ending in 1 with the next starting in 0 (and the
    reverse): a difference taken across a row boundary would show"""
    rng = np.random.default_rng(2000 + seed + rows + 3 * T)
    y = (rng.random((rows, T)) < 0.3).astype(F32)
    if not binary:
        y *= rng.integers(1, 128, (rows, T)).astype(F32) / F32(127)
    hi = F32(1) if binary else F32(0.75)
    for r in range(rows):
        y[r, 0] = hi if r % 2 == 1 else 0
        y[r, T - 1] = hi if r % 4 in (0, 1) else 0          # T = 1: the last write wins; the result is all zeros either way
    return y


# ------------------------------------------------------------------ threshold
def predict_ref(x, thr):
    """-> (float64 decision sigmoid(x) > thr as {0, 1}, margin |sigmoid64(x) - thr|); thr is taken as the float32 the kernel receives"""
    s = sigmoid64(x)
    t = f32(thr)
    with np.errstate(invalid="ignore"):
        return (s > t).astype(F64), np.abs(s - t)


def predict_f32(x, thr):
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x)) > F32(thr)).astype(F32)


def predict_inputs(n, seed=0):
    return (3.0 * np.random.default_rng(3000 + seed + n).standard_normal(n)).astype(F32)


# ------------------------------------------------------------------ F1 counts
def f1_counts_ref(pred, target, lengths):
    """pred, target [B][P][T] -> int64 [B][3] = {TP, FP, FN} over the first clamp(lengths[b], 0, T) frames; active means > 0.5 (NaN is not)"""
    pred, target = np.asarray(pred), np.asarray(target)
    B, P, T = pred.shape
    L = np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    out = np.zeros((B, 3), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            yp, yt = pred[b, :, :L[b]] > 0.5, target[b, :, :L[b]] > 0.5
            out[b] = [(yp & yt).sum(), (yp & ~yt).sum(), (~yp & yt).sum()]
    return out


def f1_inputs(B, P, T, seed=0):
    """rolls of density 0.3 with values of exactly 0.5 (inactive) and NaN (inactive) planted in both"""
    rng = np.random.default_rng(4000 + seed + B + 5 * P + 11 * T)
    pred = (rng.random((B, P, T)) < 0.3).astype(F32)
    target = (rng.random((B, P, T)) < 0.3).astype(F32)
    n = B * P * T
    if n >= 12:
        k = max(n // 50, 4)
        for a in (pred, target):
            idx = rng.choice(n, k, replace=False)
            a.reshape(-1)[idx[:k // 2]] = 0.5
            a.reshape(-1)[idx[k // 2:]] = np.nan
    return pred, target


def sweep_thresholds(K):
    """unsorted, one repeated (K >= 2) -> (float32 thresholds, (i, j) with thr[i] == thr[j] or None)"""
    base = np.array([0.5, 0.3, 0.9, 0.05, 0.7, 0.3, 0.95, 0.1, 0.6, 0.2, 0.8, 0.4, 0.15, 0.85, 0.35, 0.65], dtype=F32)
    if K == 1:
        return base[:1].copy(), None
    thr = base[:K].copy()
    thr[K - 1] = thr[1]
    return thr, (1, K - 1)


# ------------------------------------------------------------------ Adam + clip
HYPER = dict(lr=f32(1e-4), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))        # as the project trains; float32 values, as the ABI takes them
ADAM_NS = (1, 7, 4099, 524365)               # 524 365 > the 2048 x 256 update threads and the 1024 x 256 norm threads
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_NORMS = (0.01, 0.999, 1.001, 30.0)      # unclipped, either side of the clip edge, clipped
NORM_REL = 2.0 ** -22                        # norm: accumulated in f64, cast once, multiplied once
# m', v': K U (|b m| + |(1 - b) g'^k|).  p': P_ROUND U |p'| + P_STEP U |p' - p|.  The issue's starting values were 4, 4, 1 and 16; the CPU
# restatement (test_post_optim_ref_cpu.py::test_adam_rules_hold_for_the_float32_restatement) needed 2.9, 6.2 and 1.0 of the first three, so
# those were raised to twice what it needs (DESIGN 6j has the figures and the roundings behind them).
M_K, V_K, P_ROUND, P_STEP = 6, 13, 2, 16


def hyper(wd, max_norm):
    return dict(HYPER, wd=f32(wd), max_norm=f32(max_norm))


def keep_mask(n, keep_ranges):
    k = np.zeros(n, dtype=bool)
    if keep_ranges is None:
        k[:] = True
    else:
        for lo, hi in keep_ranges:
            k[lo:hi] = True
    return k


def adam_ref(p, g, m, v, hyper, step, grad_scale=1.0, keep_ranges=None):
    """clip_grad_norm_ + coupled-L2 Adam in float64 -> (p', m', v', norm, stepped).  Only the kept elements count in the norm and move."""
    p, g, m, v = (np.asarray(a, dtype=F64) for a in (p, g, m, v))
    h = hyper
    keep = keep_mask(p.size, keep_ranges)
    with np.errstate(over="ignore", invalid="ignore"):
        gs = grad_scale * g[keep]
        norm = float(np.sqrt((gs * gs).sum()))
    if not np.isfinite(norm):
        return p.copy(), m.copy(), v.copy(), norm, False
    clip = min(1.0, h["max_norm"] / (norm + 1e-6)) if h["max_norm"] > 0 else 1.0
    g1 = clip * gs + h["wd"] * p[keep]
    m1 = h["beta1"] * m[keep] + (1 - h["beta1"]) * g1
    v1 = h["beta2"] * v[keep] + (1 - h["beta2"]) * g1 * g1
    p1 = p[keep] - h["lr"] / (1 - h["beta1"] ** step) * m1 / (np.sqrt(v1) / np.sqrt(1 - h["beta2"] ** step) + h["eps"])
    po, mo, vo = p.copy(), m.copy(), v.copy()
    po[keep], mo[keep], vo[keep] = p1, m1, v1
    return po, mo, vo, norm, True


def adam_bounds(p, g, m, v, hyper, step, grad_scale=1.0, keep_ranges=None):
    """-> (bound m', bound v', bound p') per element from the float64 reference (zero outside the kept ranges: nothing may move there)"""
    p, g, m, v = (np.asarray(a, dtype=F64) for a in (p, g, m, v))
    h = hyper
    keep = keep_mask(p.size, keep_ranges)
    p1, _, _, norm, ok = adam_ref(p, g, m, v, h, step, grad_scale, keep_ranges)
    assert ok
    clip = min(1.0, h["max_norm"] / (norm + 1e-6)) if h["max_norm"] > 0 else 1.0
    # G = |clip scale g| + |wd p| stands for |g'|: the two are equal unless the weight-decay term cancels the gradient, and then the roundings
    # of the two terms stay while |g'| goes to zero (at n = 524 365 some element always cancels to a few bits)
    G = np.where(keep, np.abs(clip * grad_scale * np.where(keep, g, 0.0)) + np.abs(h["wd"] * p), 0.0)
    bm = np.where(keep, M_K * U * (np.abs(h["beta1"] * m) + (1 - h["beta1"]) * G), 0.0)
    bv = np.where(keep, V_K * U * (np.abs(h["beta2"] * v) + (1 - h["beta2"]) * G * G), 0.0)
    bp = np.where(keep, P_ROUND * U * np.abs(p1) + P_STEP * U * np.abs(p1 - p), 0.0)
    return bm, bv, bp


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; one rounding of the sum (double rounding aside)"""
    return (np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64) + np.asarray(c, dtype=F64)).astype(F32)


def adam_f32(p, g, m, v, hyper, step, grad_scale=1.0, keep_ranges=None):
    """adam_clip_kernel restated in float32 (the norm summed in float64, bc1 and bc2_sqrt cast to float, as the host does)"""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    h = {k: F32(x) for k, x in hyper.items()}
    keep = keep_mask(p.size, keep_ranges)
    with np.errstate(over="ignore", invalid="ignore"):
        gk = g[keep].astype(F64)
        norm = F32(np.sqrt((gk * gk).sum()) * float(F32(grad_scale)))
    if not np.isfinite(norm):
        return p.copy(), m.copy(), v.copy(), norm, False
    bc1 = F32(1.0 - float(h["beta1"]) ** step)
    bc2s = F32(np.sqrt(1.0 - float(h["beta2"]) ** step))
    clip = min(F32(1), h["max_norm"] / (norm + F32(1e-6))) if h["max_norm"] > 0 else F32(1)
    st = h["lr"] / bc1
    pk, mk, vk = p[keep], m[keep], v[keep]
    gi = _fma32(h["wd"], pk, (g[keep] * F32(grad_scale)) * clip)
    mi = _fma32(h["beta1"], mk, (F32(1) - h["beta1"]) * gi)
    vi = _fma32(h["beta2"], vk, (F32(1) - h["beta2"]) * gi * gi)
    pi = pk - st * mi / (np.sqrt(vi) / bc2s + h["eps"])
    po, mo, vo = p.copy(), m.copy(), v.copy()
    po[keep], mo[keep], vo[keep] = pi.astype(F32), mi, vi
    return po, mo, vo, norm, True


def adam_state(n, zero_moments, seed=0):
    """p ~ N(0, 1), m ~ N(0, 0.01), v ~ squares of N(0, 0.01) (or m = v = 0), g ~ N(0, 1) before scaling"""
    rng = np.random.default_rng(5000 + seed + n)
    p = rng.standard_normal(n).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    if n == 1 and g[0] == 0:
        g[0] = 1
    if zero_moments:
        m, v = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    else:
        m = (0.01 * rng.standard_normal(n)).astype(F32)
        v = ((0.01 * rng.standard_normal(n)) ** 2).astype(F32)
    return p, g, m, v


def scale_to_norm(g, target, grad_scale=1.0, keep_ranges=None):
    """g scaled so that the float64 norm of grad_scale g over the kept elements is `target` (to float32 rounding)"""
    keep = keep_mask(g.size, keep_ranges)
    gk = g[keep].astype(F64)
    out = g.copy()
    out[keep] = (gk * (target / (grad_scale * np.sqrt((gk * gk).sum())))).astype(F32)
    return out


def adam_cases(n):
    """(norm target, zero moments, step, wd, max_norm) for one size: every norm target meets both max_norm values and both states; steps and
    weight decays rotate so that each value occurs at every size"""
    out = []
    i = ADAM_NS.index(n)
    for a, norm in enumerate(ADAM_NORMS):
        for z in (False, True):
            for c, mx in enumerate((1.0, 0.0)):
                out.append((norm, z, ADAM_STEPS[(a + i + z + 2 * c) % 4], (0.0, 1e-5)[(a + c) % 2], mx))
    return out


def adam_case(n, norm, zero_moments, seed=0, grad_scale=1.0, keep_ranges=None):
    p, g, m, v = adam_state(n, zero_moments, seed)
    return p, scale_to_norm(g, norm, grad_scale, keep_ranges), m, v


def poison_outside(g, keep_ranges):
    """NaN and 1e30 alternately in every gradient outside the kept ranges: a leak into the norm or the update shows"""
    out = g.copy()
    idx = np.flatnonzero(~keep_mask(g.size, keep_ranges))
    out[idx] = np.where(np.arange(idx.size) % 2 == 0, F32(np.nan), F32(1e30))
    return out


def ragged_ranges(n, seed=0):
    """16 ascending disjoint ranges with ragged borders (none a multiple of 256), one of them empty, two of them adjacent"""
    rng = np.random.default_rng(6000 + seed + n)
    cuts = np.sort(rng.choice(np.arange(1, n - 1), 31, replace=False))
    cuts = [int(c) + (1 if c % 256 == 0 else 0) for c in cuts]
    r = [[cuts[2 * i], cuts[2 * i + 1]] for i in range(15)]
    r.insert(7, [r[6][1], r[6][1]])                      # empty, lo == hi
    r[3][1] = r[4][0]                                    # adjacent: hi of one is lo of the next
    assert len(r) == 16 and all(a[0] <= a[1] for a in r) and all(r[i][1] <= r[i + 1][0] for i in range(15)) and r[-1][1] <= n
    return r


def keep_range_cases(n):
    out = {"inner": [[1, n - 1]], "single": [[n // 2, n // 2 + 1]]}
    if n >= 4099:
        out["ragged16"] = ragged_ranges(n)
    return {k: r for k, r in out.items() if all(lo <= hi for lo, hi in r) and any(hi > lo for lo, hi in r)}


def ratio(err, bound):
    """largest err / bound; where the bound is zero the error must be zero"""
    err, bound = np.asarray(err, dtype=F64), np.asarray(bound, dtype=F64)
    err = np.where(np.isnan(err), 1e300, err)
    assert (err[bound == 0] == 0).all(), "an element whose bound is zero differs from the reference"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
