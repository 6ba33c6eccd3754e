"""Float64 step models of the LSTM recurrences of csrc/lstm.hip (forward) and csrc/lstm_bwd.hip (backward through time), the two
memory images tests/lstm_layout_ref.py does not state, and the inputs of tests/test_gpu_lstm_rec.py.  numpy only; nothing of the package under
test is imported.  tests/test_lstm_rec_ref_cpu.py checks all of it on the CPU (against torch.nn.LSTM and torch autograd in float64).

  gx / activated gates  f32 (f16 with MT_GX_F16)  [b/32][t][dir][k/8][gate][k%8][b%32]                              (mt_lstm_gx_bytes)
  dgx                   bf16  image [b/32][t][dir][w = k/32] of 4096 elements; unit u = k%32, gate p at
                              img[2p + (u>>4)][((u>>3)&1)*32 + b%32][u&7]                                             (mt_lstm_dgx_bytes)

Every model works on plain arrays  x[B][T][2][...]  (direction 0 walks t = 0 .. T-1, direction 1 walks t = T-1 .. 0; gate order i, f, g, o; zero
initial state) and comes in two flavours:
  exact           float64 throughout;
  kernel-rounded  float64 arithmetic with the kernels' ROUNDING POINTS and nothing else of them:
                    forward   W_hh (and W_ihx of the fused projection) rounded to f16; the published h rounded to f16, and that value is the next
                              step's operand;
                    backward  W_hh rounded to bf16; a step's dgates rounded to bf16 (what is stored is what enters W_hh^T dgates); every producer's
                              32-unit partial product rounded to bf16 before the consumer sums them.
                  The f32 summation order and the hardware exp / rcp (about 1e-7 per activation) are deliberately not modelled.

`wrong=` selects a deliberately WRONG variant of a model (tests/test_lstm_rec_ref_cpu.py: each must move the result by ten times the tolerance of the
GPU tests, i.e. those tests would notice a kernel that made the same mistake)."""
import numpy as np

import lstm_layout_ref as L

GATES = 4
WRONG_FWD = ("swap_gates", "omit_kstep", "reverse_forward", "batch_shift")
WRONG_BWD = ("swap_gates", "drop_carry", "cprev_boundary", "omit_partial", "reverse_forward", "batch_shift")


# ================================================================== layouts
def gx_index(b, t, d, p, k, T, H):
    """element offset of gate p of unit k, a[b][t][d][p][k], in the gx / activated-gates image"""
    return ((((((b // 32) * T + t) * 2 + d) * (H // 8) + k // 8) * 4 + p) * 8 + k % 8) * 32 + b % 32


def gx_words(B, T, H):
    return L.groups(B) * T * 2 * (H // 8) * 1024


def dgx_index(b, t, d, p, k, T, H):
    """element offset (bf16 words) of dgates[b][t][d][p][k] in the dgx image"""
    nw, w, u = (H + 31) // 32, k // 32, k % 32
    return (((((b // 32) * T + t) * 2 + d) * nw + w) * 8 + 2 * p + (u >> 4)) * 512 + (((u >> 3) & 1) * 32 + b % 32) * 8 + (u & 7)


def dgx_words(B, T, H):
    return L.groups(B) * T * 2 * ((H + 31) // 32) * 4096


def _grid5(B, T, H):
    return np.meshgrid(np.arange(B), np.arange(T), np.arange(2), np.arange(GATES), np.arange(H), indexing="ij")


def encode_gx(a, pad, dtype=np.float32):
    """a [B][T][2][4][H] -> flat image of `dtype` (float32, or float16 for MT_GX_F16); batch slots >= B hold pad"""
    a = np.asarray(a)
    B, T, _, _, H = a.shape
    assert H % 8 == 0 and a.shape[2] == 2 and a.shape[3] == GATES
    img = np.full(gx_words(B, T, H), pad, dtype=dtype)
    b, t, d, p, k = _grid5(B, T, H)
    img[gx_index(b, t, d, p, k, T, H)] = a.astype(dtype)
    return img


def decode_gx(image, B, T, H):
    b, t, d, p, k = _grid5(B, T, H)
    return np.asarray(image).reshape(-1)[gx_index(b, t, d, p, k, T, H)]


def encode_dgx(bits, pad_bits):
    """bits [B][T][2][4][H] uint16 (bf16 bit patterns) -> flat uint16 image; batch slots >= B and units >= H hold pad_bits"""
    bits = np.asarray(bits, dtype=np.uint16)
    B, T, _, _, H = bits.shape
    assert H % 16 == 0 and bits.shape[2] == 2 and bits.shape[3] == GATES
    img = np.full(dgx_words(B, T, H), pad_bits, dtype=np.uint16)
    b, t, d, p, k = _grid5(B, T, H)
    img[dgx_index(b, t, d, p, k, T, H)] = bits
    return img


def decode_dgx(image, B, T, H):
    """flat uint16 image -> bf16 bits [B][T][2][4][H]"""
    b, t, d, p, k = _grid5(B, T, H)
    return np.asarray(image).reshape(-1)[dgx_index(b, t, d, p, k, T, H)]


def bf16_bits_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ================================================================== rounding points
def r_f16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def r_bf16(x):
    """float64 -> the nearest bf16 (through float32, as the kernel's f32_to_bf16 sees an f32), as float64"""
    return bf16_bits_to_f64(L.bf16_bits_rne_f32(np.asarray(x, dtype=np.float64).astype(np.float32)))


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _same(x):
    return np.asarray(x, dtype=np.float64)


def _order(T, d, wrong):
    fwd = d == 0 or wrong == "reverse_forward"
    return list(range(T)) if fwd else list(range(T - 1, -1, -1))


# ================================================================== forward
def lstm_fwd(gx, w_hh, rounded, wrong=None, xproj=None):
    """gx [B][T][2][4][H] gate pre-activations from the input projection (None with xproj), w_hh [2][4H][H].
    xproj = (x [B][T][2H] = the previous layer's f16 h of both directions, w_ihx [2][4H][2H], bias [2][4H]): the fused input projection, whose
    pre-activations are W_ihx x_t + bias + W_hh h; the kernel holds W_ihx as f16 MFMA operands (rounded like W_hh), bias and the sum stay f32.
    Returns h [B][T][2][H], c [B][T][2][H], gates [B][T][2][4][H] (activated i, f, g, o) as float64; in the rounded flavour h is the PUBLISHED
    (f16-rounded) value."""
    assert wrong in (None,) + WRONG_FWD
    rw = r_f16 if rounded else _same
    w_hh = rw(w_hh)
    if xproj is not None:
        x, w_ihx, bias = xproj
        x, w_ihx, bias = _same(x), rw(w_ihx), _same(bias)
        B, T, H = x.shape[0], x.shape[1], w_hh.shape[2]
        gx = (np.einsum("btk,dgk->btdg", x, w_ihx) + bias[None, None]).reshape(B, T, 2, GATES, H)
    gx = _same(gx)
    B, T, _, _, H = gx.shape
    if wrong == "omit_kstep":
        w_hh = w_hh.copy()
        w_hh[:, :, H - 16:] = 0.0                          # the last 16-wide k-step of W_hh h
    gi, gf, gg, go = (0, 2, 1, 3) if wrong == "swap_gates" else (0, 1, 2, 3)
    h_all, c_all, g_all = np.zeros((B, T, 2, H)), np.zeros((B, T, 2, H)), np.zeros((B, T, 2, GATES, H))
    for d in range(2):
        h, c = np.zeros((B, H)), np.zeros((B, H))
        for t in _order(T, d, wrong):
            hp = np.roll(h, -1, axis=0) if wrong == "batch_shift" else h
            pre = gx[:, t, d] + (hp @ w_hh[d].T).reshape(B, GATES, H)
            i, f, g, o = _sig(pre[:, gi]), _sig(pre[:, gf]), np.tanh(pre[:, gg]), _sig(pre[:, go])
            c = f * c + i * g
            h = o * np.tanh(c)
            if rounded:
                h = r_f16(h)
            h_all[:, t, d], c_all[:, t, d] = h, c
            g_all[:, t, d] = np.stack([i, f, g, o], axis=1)
    return h_all, c_all, g_all


# ================================================================== backward
def lstm_bwd(gates, cx, dh, w_hh, rounded, wrong=None):
    """The formulas at the top of csrc/lstm_bwd.hip.  gates [B][T][2][4][H] activated, cx [B][T][2][H], dh [B][T][2][H] (gradient of the layer output),
    w_hh [2][4H][H].  Returns dgates [B][T][2][4][H] (gradient of the gate pre-activations; bf16 values in the rounded flavour).
    Sequence ends as the kernel has them: c_prev is the cell state of the forward pass's previous step (t - 1 forward, t + 1 reverse) and 0 where
    there is none; the carry dc[t_next] f[t_next] and W_hh^T dgates[t_next] are 0 at the first step processed (t = T - 1 forward, t = 0 reverse)."""
    assert wrong in (None,) + WRONG_BWD
    gates, cx, dh = _same(gates), _same(cx), _same(dh)
    rb = r_bf16 if rounded else _same
    w_hh = rb(w_hh)
    B, T, _, _, H = gates.shape
    nw = (H + 31) // 32
    pi, pf = (1, 0) if wrong == "swap_gates" else (0, 1)
    out = np.zeros((B, T, 2, GATES, H))
    for d in range(2):
        carry, prev = np.zeros((B, H)), None
        for t in _order(T, d, wrong)[::-1]:
            fwd_dir = d == 0 or wrong == "reverse_forward"
            tp = t - 1 if fwd_dir else t + 1
            if 0 <= tp < T:
                c_prev = cx[:, tp, d]
            else:
                c_prev = cx[:, t, d] if wrong == "cprev_boundary" else np.zeros((B, H))
            rec = np.zeros((B, H))
            if prev is not None:
                for w in range(1 if wrong == "omit_partial" else 0, nw):         # reduce-scatter: producer w owns units 32w .. 32w + 31
                    u0, u1 = 32 * w, min(32 * w + 32, H)
                    part = np.zeros((B, H))
                    for p in range(GATES):
                        part += prev[:, p, u0:u1] @ w_hh[d, p * H + u0:p * H + u1, :]
                    rec += rb(part)
                if wrong == "batch_shift":
                    rec = np.roll(rec, -1, axis=0)
            i, f, g, o = gates[:, t, d, pi], gates[:, t, d, pf], gates[:, t, d, 2], gates[:, t, d, 3]
            tc = np.tanh(cx[:, t, d])
            dhv = dh[:, t, d] + rec
            dc = dhv * o * (1.0 - tc * tc) + (0.0 if wrong == "drop_carry" else carry)
            dg = np.stack([dc * g * i * (1.0 - i), dc * c_prev * f * (1.0 - f), dc * i * (1.0 - g * g), dhv * tc * o * (1.0 - o)], axis=1)
            carry = dc * f
            prev = rb(dg)
            out[:, t, d] = prev
    return out


def dg_rel(got, ref):
    """the dgates' error metric, PER GATE: max |got - ref| over gate p divided by max |ref| over gate p of the case, as an array of 4 (i, f, g, o).
    Per gate because the gates' gradients differ in size (the f gate's carries c_prev, which is 0 at the sequence end): relative to the maximum over
    all four, a mistake in one gate of one step would be measured against another gate's largest element.  A gate whose reference is all zero (the f
    gate at T = 1) must be reproduced exactly: 0 if it is, inf if not."""
    out = np.zeros(GATES)
    for p in range(GATES):
        diff, top = np.abs(got[:, :, :, p] - ref[:, :, :, p]).max(), np.abs(ref[:, :, :, p]).max()
        out[p] = diff / top if top > 0 else (0.0 if diff == 0 else np.inf)
    return out


F32_EPS = 2.0 ** -23


def exact_slack(ref):
    """what the comparison with the EXACT model allows on top of twice the kernel-rounded model's distance to it: 8 f32 epsilons of the quantity's
    magnitude.  Where the two models coincide (c and the gates at T = 1: no rounded operand has entered yet) the kernel still computes in f32:
    v_exp_f32 and v_rcp_f32 (1 ulp each), the addition between them, tanh as 2 sigmoid(2x) - 1 (twice that), the product i g and the fma of the
    cell update -- a count of at most 8 roundings of values of magnitude <= max(1, |ref|)."""
    return 8 * F32_EPS * max(1.0, float(np.abs(ref).max()))


# ================================================================== the inputs of tests/test_gpu_lstm_rec.py
W_SCALE = 3.0          # weights U(-1, 1) / sqrt(H) scaled up (as trained weights are) so that the recurrent term matters
W_SCALE_BWD = 8.0      # the backward cases (synthetic saved tensors, so no forward pass saturates): W_hh^T dgates as large as dh_out itself, so that
                       # one missing partial product of sixteen moves the dgates by more than a tenth of their maximum
GX_STD = 2.5           # gate pre-activations: some saturate (|x| > 4), many stay in the linear range


def _seed(kind, H, B, T):
    return [kind, H, B, T]


def _weights(rng, H, K, scale=W_SCALE):
    return ((rng.random((2, 4 * H, K)) * 2 - 1) * (scale / np.sqrt(H))).astype(np.float32)


def fwd_case(H, B, T, g16=False):
    """gx [B][T][2][4][H] float32 (values exactly representable in f16 when g16), w_hh [2][4H][H] float32"""
    rng = np.random.default_rng(_seed(1, H, B, T))
    w_hh = _weights(rng, H, H)
    gx = (rng.standard_normal((B, T, 2, GATES, H)) * GX_STD).astype(np.float32)
    if g16:
        gx = gx.astype(np.float16).astype(np.float32)
    return gx, w_hh


def xproj_case(H, B, T, Hv=None):
    """x bits [B][T][2][H] (uint16 f16 patterns of random values with |x| < 1: the previous layer's h), w_ihx [2][4H][2H], bias [2][4H], w_hh.
    Hv < H: the layer's real width; units >= Hv of x are zero and so are their columns of w_ihx (how the model packs a padded hidden size)"""
    rng = np.random.default_rng(_seed(2, H, B, T))
    w_hh, w_ihx = _weights(rng, H, H), _weights(rng, H, 2 * H)
    bias = (rng.standard_normal((2, 4 * H)) * 1.5).astype(np.float32)
    x = (rng.random((B, T, 2, H)) * 1.98 - 0.99).astype(np.float16)
    if Hv is not None:
        x[..., Hv:] = 0
        w_ihx.reshape(2, 4 * H, 2, H)[..., Hv:] = 0.0
    return x.view(np.uint16), w_ihx, bias, w_hh


def bwd_case(H, B, T):
    """synthetic saved tensors (no forward run): gates [B][T][2][4][H] f32 (i, f, o in (0, 1), g in (-1, 1), from sigmoid / tanh of random
    pre-activations), cx [B][T][2][H] f32 of magnitude up to about 2, dh [B][T][2][H] f32, w_hh [2][4H][H] f32"""
    rng = np.random.default_rng(_seed(3, H, B, T))
    w_hh = _weights(rng, H, H, W_SCALE_BWD)
    pre = rng.standard_normal((B, T, 2, GATES, H)) * GX_STD
    gates = _sig(pre)
    gates[:, :, :, 2] = np.tanh(pre[:, :, :, 2])
    cx = (rng.random((B, T, 2, H)) * 4 - 2).astype(np.float32)
    dh = rng.standard_normal((B, T, 2, H)).astype(np.float32)
    return gates.astype(np.float32), cx, dh, w_hh
