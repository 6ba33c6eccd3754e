"""The loss, target, threshold, count and optimizer kernels of csrc/post.hip and csrc/optim.hip, one by one through the C ABI.

  mt_onset_offset_targets, mt_f1_counts, mt_f1_sweep_counts, masking, accumulate, keep ranges, skipped steps:   EXACT (== / bit for bit)
  mt_bce_masked_fwd_bwd, mt_adam_clip_step(_ex):   float64 references within the rules of tests/post_optim_ref.py
  mt_predict_threshold:   the float64 decision wherever sigmoid is further than 4 x 2^-24 from the threshold

Inputs, references and rules come from tests/post_optim_ref.py (numpy only; tests/test_post_optim_ref_cpu.py checks them without a GPU, and
that the float32 restatement of every kernel uses at most half of its rule); DESIGN 6j holds the derivations.  Every output lies in a
sentinel-filled buffer between two guard bands (an f32 NaN pattern; garbage for the uint64 counts, so the kernels' own memset is what is
observed), and whatever the contract does not write must still hold the sentinel afterwards.

Every test prints the figure it is about to assert (`-s` shows them).  Run only this file:  python -m pytest tests/test_gpu_post_optim.py -q -m gpu
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import post_optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                                # elements of guard band on either side of every output
SENT32 = 0x7FC0BEEF                        # an f32 NaN pattern
GARBAGE64 = 0x5A5AC3C3DEADBEEF             # what the count buffers hold before a call
MT_EINVAL, MT_EWORKSPACE = -1, -2
U = R.U


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


def _ptr(t):
    from music_transcription_amd._lib import ptr
    return ptr(t)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _say(what, **figs):
    print(f"MEASURED {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


class _Out:
    """n words of 4 or 8 bytes between two guard bands, all of it (the body too) pre-filled with a sentinel"""

    def __init__(self, n, np_dtype=np.float32):
        self.n, self.np_dtype = n, np.dtype(np_dtype)
        self.size = self.np_dtype.itemsize
        self.sent = SENT32 if self.size == 4 else GARBAGE64
        self.buf = torch.full((2 * GUARD + n,), self.sent, dtype=torch.int32 if self.size == 4 else torch.int64, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.size

    def preset(self, values):
        v = np.ascontiguousarray(values, dtype=self.np_dtype).reshape(-1)
        self.buf[GUARD:GUARD + self.n] = torch.from_numpy(v.view(np.int32 if self.size == 4 else np.int64)).cuda()
        return self

    def bits(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(np.uint32 if self.size == 4 else np.uint64)

    def body(self):
        return self.bits().view(self.np_dtype)

    def guards_ok(self):
        return bool((self.buf[:GUARD] == self.sent).all().item()) and bool((self.buf[GUARD + self.n:] == self.sent).all().item())

    def untouched(self):
        return bool((self.buf == self.sent).all().item())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ================================================================== 1. masked BCE
def _bce(x, y, lengths, weight, accumulate=0, preset=None, want_grad=True, ws_short=0, dims=None):
    """-> (rc, loss _Out, grad _Out or None)"""
    lib, st = _lib()
    B, P, T = dims or x.shape
    xd, yd, ld = _dev(x), _dev(y), _dev(None if lengths is None else np.asarray(lengths, dtype=np.int64))
    loss = _Out(1)
    if preset is not None:
        loss.preset([preset])
    grad = _Out(x.size) if want_grad else None
    nws = lib.mt_bce_workspace_bytes() - ws_short
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    rc = lib.mt_bce_masked_fwd_bwd(_ptr(xd), _ptr(yd), _ptr(ld), R.n_valid_frames(lengths, x.shape[0], x.shape[2]), float(weight), accumulate,
                                   loss.ptr, grad.ptr if grad else None, _ptr(ws), nws, B, P, T, st)
    torch.cuda.synchronize()
    return rc, loss, grad


@pytest.mark.parametrize("B,P,T", R.BPT)
@pytest.mark.parametrize("soft", [False, True])
def test_bce_loss_and_gradient_against_float64(mta, B, P, T, soft):
    """|loss - loss64| <= LOSS_K U (weight sum|bce| / denom); |grad - grad64| <= GRAD_K U weight / denom, and exactly 0 in every masked frame"""
    x, y = R.bce_inputs(B, P, T, soft)
    worst_l = worst_g = 0.0
    for lengths in [None] + R.length_vectors(B, T):
        for weight in (1.0, 0.25):
            nv = R.n_valid_frames(lengths, B, T)
            want_l, want_g, scale = R.bce_ref(x, y, lengths, nv, weight)
            rc, loss, grad = _bce(x, y, lengths, weight)
            _ok(rc)
            assert loss.guards_ok() and grad.guards_ok()
            got_l, got_g = float(loss.body()[0]), grad.body().reshape(B, P, T)
            mask = R.valid_mask(lengths, B, P, T)
            assert (_bits(got_g)[~mask] == 0).all(), "a masked frame's gradient is not +0"
            assert not np.isnan(got_g).any(), "a gradient was not written"
            el, eg = abs(got_l - want_l), float(np.abs(got_g - want_g).max())
            rl = el / (R.LOSS_K * U * scale) if scale > 0 else (0.0 if got_l == 0.0 else np.inf)
            rg = eg / (R.GRAD_K * U * weight / max(nv * P, 1))
            worst_l, worst_g = max(worst_l, rl), max(worst_g, rg)
            _say(f"bce ({B},{P},{T}) soft={soft} lengths={None if lengths is None else lengths.tolist()} w={weight}", loss_ratio=rl, grad_ratio=rg)
            assert rl <= 1 and rg <= 1
    _say(f"bce ({B},{P},{T}) soft={soft} worst", loss_ratio=worst_l, grad_ratio=worst_g)


@pytest.mark.parametrize("B,P,T", R.BPT[1:])
def test_bce_ignores_nonfinite_values_in_masked_frames(mta, B, P, T):
    """NaN and +-Inf in logits and targets of masked frames: loss and the valid frames' gradient keep their bits, masked gradients are 0"""
    x, y = R.bce_inputs(B, P, T)
    for lengths in R.length_vectors(B, T):
        xn, yn, xz, yz, count = R.plant_nonfinite(x, y, lengths)
        if count == 0:
            continue
        _, l1, g1 = _bce(xn, yn, lengths, 0.25)
        _, l0, g0 = _bce(xz, yz, lengths, 0.25)
        mask = R.valid_mask(lengths, B, P, T).reshape(-1)
        assert l1.bits()[0] == l0.bits()[0] and np.array_equal(g1.bits()[mask], g0.bits()[mask]) and (g1.bits()[~mask] == 0).all()
        assert np.isfinite(l1.body()[0])


def test_bce_accumulate_null_gradient_empty_batch_and_repeatability(mta):
    B, P, T = 3, 88, 501
    x, y = R.bce_inputs(B, P, T)
    lengths = R.length_vectors(B, T)[0]
    heads = []
    for w, seed in ((1.0, 0), (0.5, 1), (0.25, 2)):
        xs, ys = R.bce_inputs(B, P, T, seed=seed)
        _, l, g = _bce(xs, ys, lengths, w)
        _, l2, g2 = _bce(xs, ys, lengths, w)
        assert l.bits()[0] == l2.bits()[0] and np.array_equal(g.bits(), g2.bits()), "two calls differ"
        _, l3, _ = _bce(xs, ys, lengths, w, want_grad=False)
        assert l3.bits()[0] == l.bits()[0], "grad = NULL changes the loss"
        heads.append((xs, ys, w, np.float32(l.body()[0])))
    # accumulate = 1 onto a preset c: float32(c) + v, bit for bit
    for c in (0.0, 1.5, -0.3333333432674408, 1e-9):
        xs, ys, w, v = heads[0]
        _, l, _ = _bce(xs, ys, lengths, w, accumulate=1, preset=c)
        assert l.bits()[0] == _bits(np.float32(c) + v)[0]
    # three heads into one word: the chained float32 sum
    lib, st = _lib()
    loss = _Out(1)
    ws = torch.empty(lib.mt_bce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    chain = np.float32(0)
    ld = _dev(lengths)
    for i, (xs, ys, w, v) in enumerate(heads):
        xd, yd = _dev(xs), _dev(ys)
        _ok(lib.mt_bce_masked_fwd_bwd(_ptr(xd), _ptr(yd), _ptr(ld), R.n_valid_frames(lengths, B, T), w, 1 if i else 0, loss.ptr, None,
                                      _ptr(ws), ws.numel(), B, P, T, st))
        chain = v if i == 0 else np.float32(chain + v)
    torch.cuda.synchronize()
    assert loss.bits()[0] == _bits(chain)[0] and loss.guards_ok()
    # every length 0 (or negative): loss exactly 0, gradient all zero
    for empty in (np.zeros(B, dtype=np.int64), np.array([0, -3, 0], dtype=np.int64)):
        _, l, g = _bce(x, y, empty, 1.0)
        assert l.bits()[0] == 0 and (g.bits() == 0).all()
    # argument checks: nothing is written
    rc, l, g = _bce(x, y, lengths, 1.0, ws_short=1)
    assert rc == MT_EWORKSPACE and l.untouched() and g.untouched()
    rc, l, g = _bce(x, y, None, 1.0, dims=(0, P, T))
    assert rc == MT_EINVAL and l.untouched() and g.untouched()


# ================================================================== 2. onset / offset targets
@pytest.mark.parametrize("rows,T", R.ROWS_T)
@pytest.mark.parametrize("binary", [True, False])
def test_onset_offset_targets_exact(mta, rows, T, binary):
    """equal to the float32 reference everywhere; T = 1 gives zeros; no difference crosses a row boundary (rows end and start in every
    combination of 0 and 1)"""
    lib, st = _lib()
    y = R.roll_inputs(rows, T, binary)
    want_on, want_off = R.onset_offset_ref(y)
    yd = _dev(y)
    on, off = _Out(rows * T), _Out(rows * T)
    _ok(lib.mt_onset_offset_targets(_ptr(yd), on.ptr, off.ptr, rows, T, st))
    torch.cuda.synchronize()
    assert on.guards_ok() and off.guards_ok()
    assert np.array_equal(on.bits(), _bits(want_on).reshape(-1)) and np.array_equal(off.bits(), _bits(want_off).reshape(-1))
    if T == 1:
        assert (on.bits() == 0).all() and (off.bits() == 0).all()


# ================================================================== 3. threshold
@pytest.mark.parametrize("n", [1, 70, 300 * 901])
@pytest.mark.parametrize("thr", R.THRESHOLDS)
def test_predict_threshold_against_float64(mta, n, thr):
    lib, st = _lib()
    x = R.predict_inputs(n)
    want, margin = R.predict_ref(x, thr)
    xd = _dev(x)
    out = _Out(n)
    _ok(lib.mt_predict_threshold(_ptr(xd), out.ptr, n, thr, st))
    torch.cuda.synchronize()
    got = out.body()
    assert out.guards_ok() and set(np.unique(got).tolist()) <= {0.0, 1.0}
    live = margin > R.PREDICT_K * U
    share = 1.0 - float(live.mean())
    _say(f"threshold n={n} thr={thr}", left_out=share, wrong=int((got[live] != want[live]).sum()))
    assert share <= 1e-3 and np.array_equal(got[live], want[live])


def test_predict_threshold_planted_cases_and_empty_call(mta):
    lib, st = _lib()
    xd = _dev(np.array([0.0, np.inf, -np.inf, np.nan], dtype=np.float32))
    out = _Out(4)
    _ok(lib.mt_predict_threshold(_ptr(xd), out.ptr, 4, 0.5, st))
    torch.cuda.synchronize()
    assert out.body().tolist() == [0.0, 1.0, 0.0, 0.0] and out.guards_ok()          # sigmoid(0) = 0.5 is not > 0.5; NaN compares false
    out = _Out(4)
    _ok(lib.mt_predict_threshold(_ptr(xd), out.ptr, 0, 0.5, st))
    torch.cuda.synchronize()
    assert out.untouched()


# ================================================================== 4. F1 counts
def _f1_counts(pred, target, lengths):
    lib, st = _lib()
    B, P, T = pred.shape
    pd, td, ld = _dev(pred), _dev(target), _dev(None if lengths is None else np.asarray(lengths, dtype=np.int64))
    counts = _Out(3 * B, np.uint64)
    _ok(lib.mt_f1_counts(_ptr(pd), _ptr(td), _ptr(ld), counts.ptr, B, P, T, st))
    torch.cuda.synchronize()
    assert counts.guards_ok()
    return counts.body().astype(np.int64).reshape(B, 3)


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("P,T", [(3, 5), (88, 501)])
def test_f1_counts_exact(mta, B, P, T):
    """P T = 15: a partial wave; 88 x 501 > the 8 x 256 threads per sample.  Values of exactly 0.5 and NaN are inactive; lengths beyond T, zero
    and negative are clamped; the counts start from garbage"""
    pred, target = R.f1_inputs(B, P, T)
    for lengths in [None] + R.length_vectors(B, T):
        want = R.f1_counts_ref(pred, target, lengths)
        got = _f1_counts(pred, target, lengths)
        assert np.array_equal(got, want), (None if lengths is None else lengths.tolist(), got.tolist(), want.tolist())
    assert R.f1_counts_ref(pred, target, None).sum() > 0


# ================================================================== 5. F1 sweep
@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("B,P,T", [(1, 3, 5), (9, 88, 33), (3, 88, 501)])
def test_f1_sweep_equals_threshold_then_counts(mta, K, B, P, T):
    """counts[b][k] == mt_f1_counts(mt_predict_threshold(logits, thr[k]), target, lengths), bit for bit: the same expression, so no tolerance"""
    lib, st = _lib()
    x, _ = R.bce_inputs(B, P, T)
    _, target = R.f1_inputs(B, P, T)
    thr, rep = R.sweep_thresholds(K)
    xd, td, thd = _dev(x), _dev(target), _dev(thr)
    for lengths in [None] + R.length_vectors(B, T):
        ld = _dev(None if lengths is None else lengths)
        counts = _Out(3 * B * K, np.uint64)
        _ok(lib.mt_f1_sweep_counts(_ptr(xd), _ptr(td), _ptr(ld), _ptr(thd), K, counts.ptr, B, P, T, st))
        torch.cuda.synchronize()
        assert counts.guards_ok()
        got = counts.body().astype(np.int64).reshape(B, K, 3)
        for k in range(K):
            roll = _Out(B * P * T)
            _ok(lib.mt_predict_threshold(_ptr(xd), roll.ptr, B * P * T, float(thr[k]), st))
            torch.cuda.synchronize()
            want = _f1_counts(roll.body().reshape(B, P, T), target, lengths)
            assert np.array_equal(got[:, k], want), (k, float(thr[k]))
            assert np.array_equal(want, R.f1_counts_ref(roll.body().reshape(B, P, T), target, lengths))
        if rep:
            assert np.array_equal(got[:, rep[0]], got[:, rep[1]])
    assert got.sum() > 0 or B * P * T < 100


def test_f1_sweep_rejects_zero_and_seventeen_thresholds(mta):
    lib, st = _lib()
    x, _ = R.bce_inputs(2, 5, 7)
    _, target = R.f1_inputs(2, 5, 7)
    xd, td, thd = _dev(x), _dev(target), _dev(np.linspace(0.1, 0.9, 17).astype(np.float32))
    for K in (0, 17):
        counts = _Out(3 * 2 * 17, np.uint64)
        assert lib.mt_f1_sweep_counts(_ptr(xd), _ptr(td), None, _ptr(thd), K, counts.ptr, 2, 5, 7, st) == MT_EINVAL
        torch.cuda.synchronize()
        assert counts.untouched()


# ================================================================== 6. Adam + clip
def _adam(p, g, m, v, h, step, gs=1.0, ranges=None, stats=True, plain=False, ws_short=0, n=None):
    """one call -> (rc, p', m', v', stats or None, the gradient buffer afterwards), everything as float32 arrays"""
    lib, st = _lib()
    n = p.size if n is None else n
    outs = [_Out(p.size).preset(a) for a in (p, m, v)]
    gd = _dev(g)
    so = _Out(2) if stats else None
    nws = lib.mt_adam_workspace_bytes() - ws_short
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    hy = (h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["max_norm"])
    if plain:
        rc = lib.mt_adam_clip_step(outs[0].ptr, _ptr(gd), outs[1].ptr, outs[2].ptr, n, *hy, step, so.ptr if so else None, _ptr(ws), nws, st)
    else:
        kr = None if ranges is None else torch.tensor(ranges, dtype=torch.int64).reshape(-1)            # a HOST array
        rc = lib.mt_adam_clip_step_ex(outs[0].ptr, _ptr(gd), outs[1].ptr, outs[2].ptr, n, *hy, step, float(gs),
                                      None if kr is None else kr.data_ptr(), 0 if ranges is None else len(ranges),
                                      so.ptr if so else None, _ptr(ws), nws, st)
    torch.cuda.synchronize()
    assert all(o.guards_ok() for o in outs) and (so is None or so.guards_ok())
    return rc, outs[0].body(), outs[1].body(), outs[2].body(), (so.body() if so else None), gd.cpu().numpy()


def _adam_check(what, got, p, g, m, v, h, step, gs, ranges, worst):
    """the rules of post_optim_ref against adam_ref; outside the kept ranges the bounds are zero, so nothing may have moved there"""
    rc, p1, m1, v1, stats, g_after = got
    _ok(rc)
    ref = R.adam_ref(p, g, m, v, h, step, gs, ranges)
    bm, bv, bp = R.adam_bounds(p, g, m, v, h, step, gs, ranges)
    assert np.array_equal(_bits(g_after), _bits(g)), "grads was written"
    keep = R.keep_mask(p.size, ranges)
    for a, b in ((p1, p), (m1, m), (v1, v)):
        assert np.array_equal(_bits(a)[~keep], _bits(b)[~keep]), "an element outside the kept ranges moved"
    assert stats[1] == 1.0, f"{what}: the step was skipped (norm {stats[0]})"
    figs = dict(norm=abs(float(stats[0]) - ref[3]) / (R.NORM_REL * ref[3]) if ref[3] > 0 else float(stats[0] != 0),
                m=R.ratio(np.abs(m1 - ref[1]), bm), v=R.ratio(np.abs(v1 - ref[2]), bv), p=R.ratio(np.abs(p1 - ref[0]), bp))
    for k, x in figs.items():
        worst[k] = max(worst.get(k, 0.0), x)
    assert max(figs.values()) <= 1, (what, figs)


@pytest.mark.parametrize("n", R.ADAM_NS)
def test_adam_one_step_against_float64(mta, n):
    """one step from a given state (nothing compounds): norms 0.01, 0.999, 1.001 and 30 against max_norm 1 and 0, both states, every step count
    and weight decay, grad_scale 1, 0.5 and 0.125.  Rules: norm 2^-22 relative; m', v', p' per element (post_optim_ref.adam_bounds)"""
    worst = {}
    scaled = [c for c in R.adam_cases(n) if not c[1]][::2]                  # the non-zero state at every norm target
    for (norm, zero, step, wd, mx) in R.adam_cases(n):
        for gs in (1.0, 0.5, 0.125):
            if gs != 1.0 and (norm, zero, step, wd, mx) not in scaled:
                continue
            p, g, m, v = R.adam_case(n, norm, zero, grad_scale=gs)
            h = R.hyper(wd, mx)
            got = _adam(p, g, m, v, h, step, gs)
            _adam_check(f"n={n} norm={norm} zero={zero} step={step} wd={wd} max_norm={mx} scale={gs}", got, p, g, m, v, h, step, gs, None, worst)
            if gs != 1.0:
                # the same step from pre-scaled gradients (the scale is a power of two: exact) with scale 1
                g2 = (g * np.float32(gs)).astype(np.float32)
                _, p2, m2, v2, s2, _ = _adam(p, g2, m, v, h, step, 1.0)
                bm, bv, bp = R.adam_bounds(p, g, m, v, h, step, gs)
                assert R.ratio(np.abs(p2.astype(np.float64) - got[1]), bp) <= 1 and R.ratio(np.abs(m2.astype(np.float64) - got[2]), bm) <= 1
                assert R.ratio(np.abs(v2.astype(np.float64) - got[3]), bv) <= 1 and abs(float(s2[0]) - float(got[4][0])) <= R.NORM_REL * float(s2[0])
    _say(f"adam n={n} worst ratio", **worst)


@pytest.mark.parametrize("n", [7, 4099, 524365])
def test_adam_keep_ranges(mta, n):
    """outside the ranges p, m, v keep their bits although the gradients there are NaN and 1e30 (a leak into the norm would skip the step, a
    leak into the update would move an element); inside, the rules hold"""
    worst = {}
    for name, ranges in R.keep_range_cases(n).items():
        for (norm, zero, step, wd, mx) in R.adam_cases(n)[::5]:
            p, g, m, v = R.adam_case(n, norm, zero, keep_ranges=ranges)
            g = R.poison_outside(g, ranges)
            h = R.hyper(wd, mx)
            _adam_check(f"n={n} ranges={name} norm={norm}", _adam(p, g, m, v, h, step, 1.0, ranges), p, g, m, v, h, step, 1.0, ranges, worst)
    _say(f"adam keep ranges n={n} worst ratio", **worst)


def test_adam_rejects_bad_arguments_without_writing(mta):
    n = 4099
    p, g, m, v = R.adam_case(n, 1.0, False)
    h = R.hyper(1e-5, 1.0)
    bad = {"17 ranges": [[10 * i, 10 * i + 5] for i in range(17)], "overlap": [[0, 100], [99, 200]], "descending": [[200, 300], [0, 100]],
           "hi > n": [[0, n + 1]], "hi < lo": [[100, 50]]}
    for name, ranges in bad.items():
        rc, p1, m1, v1, stats, _ = _adam(p, g, m, v, h, 1, 1.0, ranges)
        assert rc == MT_EINVAL, name
        assert np.array_equal(_bits(p1), _bits(p)) and np.array_equal(_bits(m1), _bits(m)) and np.array_equal(_bits(v1), _bits(v)) and np.isnan(stats).all()
    rc, p1, *_ = _adam(p, g, m, v, h, 0)
    assert rc == MT_EINVAL and np.array_equal(_bits(p1), _bits(p))
    rc, p1, *_ = _adam(p, g, m, v, h, 1, gs=0.0)
    assert rc == MT_EINVAL and np.array_equal(_bits(p1), _bits(p))
    rc, p1, *_ = _adam(p, g, m, v, h, 1, ws_short=1)
    assert rc == MT_EWORKSPACE and np.array_equal(_bits(p1), _bits(p))


@pytest.mark.parametrize("n", [7, 524365])
def test_adam_nonfinite_zero_null_stats_and_the_plain_entry_point(mta, n):
    h = R.hyper(1e-5, 1.0)
    p, g, m, v = R.adam_case(n, 1.0, False)
    # a NaN or an Inf in one kept gradient: the step is skipped, nothing moves
    for bad in (np.nan, np.inf):
        for ranges in (None, [[1, n - 1]]):
            g2 = g.copy()
            g2[n // 2] = bad
            rc, p1, m1, v1, stats, _ = _adam(p, g2, m, v, h, 3, 1.0, ranges)
            _ok(rc)
            assert stats[1] == 0.0 and not np.isfinite(stats[0])
            assert np.array_equal(_bits(p1), _bits(p)) and np.array_equal(_bits(m1), _bits(m)) and np.array_equal(_bits(v1), _bits(v))
    # g = 0, wd = 0, m = v = 0: p keeps its bits, stats = {0, 1}
    z = np.zeros(n, dtype=np.float32)
    rc, p1, m1, v1, stats, _ = _adam(p, z, z, z, R.hyper(0.0, 1.0), 1)
    _ok(rc)
    assert np.array_equal(_bits(p1), _bits(p)) and not m1.any() and not v1.any() and stats.tolist() == [0.0, 1.0]
    # stats = NULL; mt_adam_clip_step == _ex(..., 1.0, NULL, 0), bit for bit; two calls agree
    a = _adam(p, g, m, v, h, 2)
    b = _adam(p, g, m, v, h, 2, stats=False)
    c = _adam(p, g, m, v, h, 2, plain=True)
    _ok(a[0]), _ok(b[0]), _ok(c[0])
    for i in (1, 2, 3):
        assert np.array_equal(_bits(a[i]), _bits(b[i])) and np.array_equal(_bits(a[i]), _bits(c[i]))
    assert np.array_equal(_bits(a[4]), _bits(c[4])) and not np.array_equal(_bits(a[1]), _bits(p))
