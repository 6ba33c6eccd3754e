"""CPU-side tests (no GPU) of the weight average and the learning-rate schedule of optim.FusedAdamClip: the float64 references of
tests/optim_ema_ref.py, the decay rule, LRSchedule, and the two new exports in the header and the ctypes bindings."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ema_ref as E  # noqa: E402
import post_optim_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def test_ema_reference_rule_on_top_of_adam_ref():
    n, ranges = 255, [[3, 100], [100, 100], [200, 255]]
    p, g, m, v = R.adam_case(n, 30.0, False, keep_ranges=ranges)
    e = E.ema_state(p)
    h = R.hyper(1e-5, 1.0)
    w = E.ema_weight_f32(0.99, 1000)
    p1, m1, v1, e1, norm, ok = E.adam_ema_ref(p, g, m, v, e, h, 7, w, 1.0, ranges)
    a = R.adam_ref(p, g, m, v, h, 7, 1.0, ranges)
    assert ok and all(np.array_equal(x, y) for x, y in zip((p1, m1, v1), a[:3])) and norm == a[3]
    keep = R.keep_mask(n, ranges)
    assert np.array_equal(e1[~keep], e.astype(np.float64)[~keep])
    assert np.allclose(e1[keep], (1 - w) * e.astype(np.float64)[keep] + w * p1[keep], rtol=0, atol=1e-15)
    # w = 1 lands on p', p' == e stays, and a skipped step moves nothing
    assert np.allclose(E.ema_ref(e, p1, 1.0)[keep], p1[keep], rtol=0, atol=1e-15)
    assert np.array_equal(E.ema_ref(p1, p1, 0.37), p1)
    g2 = g.copy()
    g2[5] = np.nan
    assert np.array_equal(E.adam_ema_ref(p, g2, m, v, e, h, 7, w, 1.0, ranges)[3], e.astype(np.float64))
    # the float32 restatement of the kernel's expression stays inside the bound
    e32 = R._fma32(np.float32(w), p1.astype(np.float32) - e, e)
    ref = E.ema_ref(e, p1.astype(np.float32), w, ranges)
    assert R.ratio(np.abs(e32.astype(np.float64) - ref)[keep], E.ema_bound(e, p1.astype(np.float32))[keep]) <= 1


def test_ema_decay_rule(mta):
    from music_transcription_amd.optim import ema_decay_at
    for fn in (E.ema_decay_ref, ema_decay_at):
        assert fn(0.999, 1) == 2.0 / 11.0
        assert fn(0.999, 9) == 10.0 / 19.0
        assert fn(0.999, 10 ** 6) == 0.999
        assert fn(0.999, 1, False) == 0.999
        assert fn(0.0, 5) == 0.0
    assert E.ema_weight_f32(0.999, 1) == R.f32(9.0 / 11.0) and 0.0 < E.ema_weight_f32(0.999, 10 ** 6) <= 1.0


def test_lr_schedule(mta):
    S = mta.LRSchedule
    base, mn, wu, tot = 3e-4, 1e-5, 100, 1100
    s = S(base, warmup_steps=wu, total_steps=tot, min_lr=mn)
    assert s.at(1) == base * 1 / wu and s.at(wu) == base                      # the end points of the warm-up
    assert s.at((wu + tot) // 2) == pytest.approx((base + mn) / 2, rel=1e-12)  # the cosine's midpoint
    lrs = [s.at(t) for t in range(1, tot + 50)]
    assert all(a < b for a, b in zip(lrs[:wu - 1], lrs[1:wu]))                # rises through the warm-up ...
    assert all(a >= b for a, b in zip(lrs[wu - 1:], lrs[wu:]))                # ... and never after it
    assert s.at(tot) == mn and s.at(tot + 1) == mn and s.at(10 * tot) == mn
    assert all(s.at(t) == E.lr_ref(base, wu, tot, mn, t) for t in (1, 2, wu, wu + 1, 600, tot - 1, tot, tot + 7))
    flat = S(base, warmup_steps=4)
    assert [flat.at(t) for t in (1, 4, 5, 10 ** 6)] == [base / 4, base, base, base]
    assert S(base).at(1) == base and S(base, total_steps=10).at(1) < base and S(base, total_steps=10).at(10) == 0.0
    assert s.params() == dict(base_lr=base, warmup_steps=wu, total_steps=tot, min_lr=mn)
    for bad in (dict(warmup_steps=10, total_steps=10), dict(warmup_steps=11, total_steps=10), dict(warmup_steps=-1), dict(total_steps=0),
                dict(warmup_steps=1.5), dict(min_lr=-1e-6), dict(min_lr=1.0)):
        with pytest.raises(ValueError):
            S(base, **bad)
    for bad_lr in (0.0, -1e-4, math.nan, math.inf):
        with pytest.raises(ValueError):
            S(bad_lr)


def test_new_exports_in_header_and_bindings(mta):
    hdr = open(os.path.join(ROOT, "include", "mt_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mt_[a-z0-9_]+)\s*\(", hdr))
    from music_transcription_amd import _lib
    for name in ("mt_adam_clip_step_ema", "mt_swap_f32"):
        assert name in declared, f"{name} is not declared in include/mt_hip.h"
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), f"{name} is not bound in _lib.py"
    # the entry point takes mt_adam_clip_step_ex's arguments plus the average and its weight
    ex, ema = (getattr(_lib.lib, n).argtypes for n in ("mt_adam_clip_step_ex", "mt_adam_clip_step_ema"))
    assert len(ema) == len(ex) + 2 and len(_lib.lib.mt_swap_f32.argtypes) == 4
