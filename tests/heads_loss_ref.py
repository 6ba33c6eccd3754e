"""Float64 reference, inputs, tolerance rules and float32 restatement for the weighted / focal three-head loss of csrc/heads_loss.hip
(numpy only).  tests/test_heads_loss_cpu.py checks all of it without a GPU; tests/test_gpu_heads_loss.py feeds the same inputs to
mt_heads_loss_fwd_bwd through the C ABI.  DESIGN 6b "Weighted and focal loss" holds the formula and the derivations.

Per valid cell of head h (logit x, target y, w = pos_weight[h], g = gamma[h]):
    a = softplus(x), b = softplus(-x), l = w y exp(-g a) b + (1 - y) exp(-g b) a
    dl/dx = -w y exp(-g a) (g p b + 1 - p) + (1 - y) exp(-g b) (g (1 - p) a + p),   p = sigmoid(x)
    loss_h = head_weight[h] sum_valid l / denom,  grad = head_weight[h] dl/dx / denom (0 in masked frames),  denom = max(n_valid P, 1)

Rules (the code under test never sets one; U = 2^-24):
    |loss_h - ref| <= K_L U head_weight sum|l| / denom
    |grad - ref|   <= K_G U head_weight max(pos_weight, 1) 1.5 / denom       (1.5 >= max |dl/dx| / max(w, 1) for g <= 8: 1.436 at g = 8,
                                                                               test_heads_loss_cpu.py::test_gradient_factor_stays_below_1_5)
    total: bit for bit float32((frame + onset) + offset) of the three parts the call returned.
K_L and K_G started at post_optim_ref.LOSS_K = 9 and GRAD_K = 5.5.  The float32 restatement below (the kernel's expressions in numpy
float32, run on the CPU over every case of cases() at every shape of BPT) needs 4.41 U of the loss rule (the single cell of (1, 1, 1)) and
5.59 U of the gradient rule (gamma = 8 at (3, 88, 501): the rounding of gamma * softplus is magnified by the exponential it goes into)
(test_heads_loss_cpu.py::test_rules_hold_for_the_float32_restatement prints both).  4.41 is less than half of 9, so K_L stays 9; 5.59 is
more than half of 5.5, so K_G is twice the need, 11.2."""
import numpy as np

import post_optim_ref as P

U, F32, F64 = P.U, P.F32, P.F64
BPT = P.BPT
K_L = 9
K_G = 11.2
GRAD_FACTOR = 1.5
WG = [(1.0, 0.0), (4.0, 0.0), (1.0, 2.0), (8.0, 1.5), (0.5, 8.0)]       # (pos_weight, gamma) drawn per head
HEAD_WEIGHTS = (0.5, 0.25, 0.25)


# ------------------------------------------------------------------ targets
def targets3(roll, onset_roll=None):
    """-> [frame, onset, offset] float32 targets: mt_onset_offset_targets' edges of the roll (within a row, whatever lengths says), the
    onset one replaced by onset_roll where given"""
    on, off = P.onset_offset_ref(roll)
    return [np.asarray(roll, dtype=F32), on if onset_roll is None else np.asarray(onset_roll, dtype=F32), off]


# ------------------------------------------------------------------ float64 reference
def cell64(x, y, w, g):
    """-> (l, dl/dx) in float64"""
    x, y = np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        l1p = np.log1p(np.exp(-np.abs(x)))
        a, b = np.maximum(x, 0.0) + l1p, np.maximum(-x, 0.0) + l1p
        p, q = P.sigmoid64(x), P.sigmoid64(-x)
        fa, fb = np.exp(-g * a), np.exp(-g * b)
        l = w * y * fa * b + (1.0 - y) * fb * a
        d = -w * y * fa * (g * p * b + q) + (1.0 - y) * fb * (g * q * a + p)
    return l, d


def heads_loss_ref(xs, roll, onset_roll, lengths, head_w, pos_w, gamma):
    """xs: [frame] or [frame, onset, offset] logits (B, P, T) -> dict(total, parts[3], grads[len(xs)], scales[3], denom); parts and
    scales of absent heads are 0; scales[h] = head_w[h] sum_valid |l| / denom, what the loss rule is relative to"""
    B, Pn, T = xs[0].shape
    mask = P.valid_mask(lengths, B, Pn, T)
    denom = max(float(P.n_valid_frames(lengths, B, T)) * Pn, 1.0)
    ys = targets3(roll, onset_roll)
    parts, scales, grads = [0.0] * 3, [0.0] * 3, []
    for h, x in enumerate(xs):
        l, d = cell64(x, ys[h], pos_w[h], gamma[h])
        l = np.where(mask, l, 0.0)
        parts[h] = float(head_w[h] * l.sum() / denom)
        scales[h] = float(head_w[h] * np.abs(l).sum() / denom)
        grads.append(np.where(mask, head_w[h] * d / denom, 0.0))
    return dict(total=parts[0] + parts[1] + parts[2], parts=parts, grads=grads, scales=scales, denom=denom)


def loss_bound(scale):
    return K_L * U * scale


def grad_bound(head_w, pos_w, denom):
    return K_G * U * head_w * max(pos_w, 1.0) * GRAD_FACTOR / denom


def total_of(parts):
    """the kernel's total from its own three parts: float32((frame + onset) + offset)"""
    p = np.asarray(parts, dtype=F32)
    return F32(F32(p[0] + p[1]) + p[2])


# ------------------------------------------------------------------ the kernel's expressions in float32
def cell32(x, y, w, g):
    x, y, w, g = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32), F32(w), F32(g)
    one, zero = F32(1), F32(0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = np.exp(-np.abs(x))
        l1p = np.log1p(e)
        a, b = np.maximum(x, zero) + l1p, np.maximum(-x, zero) + l1p
        r = one / (one + e)
        er = e * r
        p, q = np.where(x >= 0, r, er), np.where(x >= 0, er, r)
        fa, fb = np.exp(-g * a), np.exp(-g * b)
        pos, neg = w * y * fa, (one - y) * fb
        d = neg * (g * q * a + p) - pos * (g * p * b + q)
        l = pos * b + neg * a
    assert l.dtype == F32 and d.dtype == F32
    return l, d


def heads_loss_f32(xs, roll, onset_roll, lengths, head_w, pos_w, gamma):
    """-> (parts float32 [3], total float32, grads float32): per-head sums in float64, as the kernel keeps them"""
    B, Pn, T = xs[0].shape
    mask = P.valid_mask(lengths, B, Pn, T)
    denom = max(float(P.n_valid_frames(lengths, B, T)) * Pn, 1.0)
    ys = targets3(roll, onset_roll)
    parts, grads = np.zeros(3, dtype=F32), []
    for h, x in enumerate(xs):
        l, d = cell32(x, ys[h], pos_w[h], gamma[h])
        s = np.where(mask, l.astype(F64), 0.0).sum()
        parts[h] = F32(head_w[h]) * F32(s / denom)
        gs = F32(float(F32(head_w[h])) / denom)
        grads.append(np.where(mask, gs * d, F32(0)).astype(F32))
    return parts, total_of(parts), grads


# ------------------------------------------------------------------ inputs
def inputs(B, Pn, T, soft):
    """-> (xs [3], roll, onset_roll): three heads' logits with post_optim_ref's planted values, a hard or soft roll and a given onset
    roll.  Where there is room, the roll is 1 under the frame head's -100 and 0 under its +100, and the given onset roll likewise under
    the onset head's: the two cells whose loss is 100 w and 100"""
    xs, ys = zip(*(P.bce_inputs(B, Pn, T, soft, seed=h) for h in range(3)))
    roll, onset_roll = ys[0].copy(), ys[1].copy()
    for x, y in ((xs[0], roll), (xs[1], onset_roll)):
        y[x == F32(-100)] = 1
        y[x == F32(100)] = 0
    return list(xs), roll, onset_roll


def cases(B, Pn, T):
    """every call of the float64 comparison at one shape: (xs, roll, onset_roll or None, lengths or None, pos_w [3], gamma [3]).  Hard and
    soft targets x lengths = NULL and every post_optim_ref.length_vectors entry x derived and given onset targets; the (w, g) pairs
    rotate so that the three heads differ within a call and every pair reaches every head at every shape"""
    out, k = [], 0
    for soft in (False, True):
        xs, roll, onset_roll = inputs(B, Pn, T, soft)
        for lengths in [None] + P.length_vectors(B, T):
            for given in (False, True):
                wg = [WG[(k + 2 * h) % len(WG)] for h in range(3)]
                out.append((xs, roll, onset_roll if given else None, lengths, [w for w, _ in wg], [g for _, g in wg]))
                k += 1
    assert k >= len(WG)
    return out


def edge_roll(B, Pn, T, ones):
    """all ones, or zeros with a 1 in the last frame of every even row and in the first frame of the row after it: a target taken across a
    row boundary would show (rows are the B * Pn pitch rows of T frames)"""
    y = np.ones((B * Pn, T), dtype=F32) if ones else np.zeros((B * Pn, T), dtype=F32)
    if not ones:
        y[0::2, T - 1] = 1
        y[1::2, 0] = 1
    return y.reshape(B, Pn, T)
