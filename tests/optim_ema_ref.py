"""Float64 references for the weight average of csrc/optim.hip (mt_adam_clip_step_ema), its decay rule and the learning-rate schedule
(numpy only), on top of post_optim_ref.adam_ref.  tests/test_optim_ema_cpu.py checks them without a GPU; tests/test_gpu_optim_ema.py feeds
the same inputs to the kernels through the C ABI.

The bound on the average.  The kernel forms e' = fmaf(w, p' - e, e) in float32 from its own p', with 0 < w <= 1 a float32.  Against the
float64 value of e + w (p' - e) at those same float32 inputs:
  - the subtraction d = p' - e rounds once: at most U |p' - e| <= 2 U max(|e|, |p'|);
  - that error is multiplied by w <= 1, so it stays at most 2 U max;
  - the fused multiply-add rounds once more: at most U |e'|, and e' lies between e and p', so at most U max(|e|, |p'|) (to first order).
Together |e' - ref| <= 3 U max(|e|, |p'|), U = 2^-24.  The bound comes from this arithmetic alone, not from the code under test."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_optim_ref as R  # noqa: E402

U, F32, F64 = R.U, R.F32, R.F64
EMA_K = 3                                    # |e' - ref| <= EMA_K U max(|e|, |p'|)
EMA_NS = (1, 255, 524291)                    # 524 291 = one full grid stride of 2048 x 256 threads, plus 3
SWAP_NS = (1, 3, 1027, 524291)


def ema_decay_ref(ema_decay, t, warmup=True):
    """d_t = min(ema_decay, (1 + t) / (10 + t)) with the warm-up, ema_decay without; t is the 1-based step count"""
    return min(float(ema_decay), (1.0 + t) / (10.0 + t)) if warmup else float(ema_decay)


def ema_weight_f32(ema_decay, t, warmup=True):
    """1 - d_t formed in float64 and cast once: the float the kernel receives"""
    return R.f32(1.0 - ema_decay_ref(ema_decay, t, warmup))


def ema_ref(e, p_new, w, keep_ranges=None, stepped=True):
    """e + w (p' - e) in float64 on the kept elements of a step that was taken; everything else keeps e"""
    e, p_new = np.asarray(e, dtype=F64), np.asarray(p_new, dtype=F64)
    out = e.copy()
    if stepped:
        keep = R.keep_mask(e.size, keep_ranges)
        out[keep] = e[keep] + float(w) * (p_new[keep] - e[keep])
    return out


def ema_bound(e, p_new, keep_ranges=None):
    """EMA_K U max(|e|, |p'|) on the kept elements, zero elsewhere (nothing may move there)"""
    e, p_new = np.asarray(e, dtype=F64), np.asarray(p_new, dtype=F64)
    return np.where(R.keep_mask(e.size, keep_ranges), EMA_K * U * np.maximum(np.abs(e), np.abs(p_new)), 0.0)


def adam_ema_ref(p, g, m, v, e, hyper, step, w, grad_scale=1.0, keep_ranges=None):
    """post_optim_ref.adam_ref, then the average moved towards ITS p' -> (p', m', v', e', norm, stepped), all float64"""
    p1, m1, v1, norm, ok = R.adam_ref(p, g, m, v, hyper, step, grad_scale, keep_ranges)
    return p1, m1, v1, ema_ref(e, p1, w, keep_ranges, ok), norm, ok


def ema_state(p, seed=0):
    """an average that is neither the parameters nor far from them: p + N(0, 0.05), float32"""
    rng = np.random.default_rng(7000 + seed + p.size)
    return (p.astype(F64) + 0.05 * rng.standard_normal(p.size)).astype(F32)


def lr_ref(base_lr, warmup_steps, total_steps, min_lr, t):
    """the schedule in float64: linear warm-up, then (with total_steps) a half cosine down to min_lr, held there; else base_lr"""
    if warmup_steps and t <= warmup_steps:
        return base_lr * t / warmup_steps
    if total_steps is None:
        return base_lr
    if t >= total_steps:
        return min_lr
    return min_lr + (base_lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (t - warmup_steps) / (total_steps - warmup_steps)))
