"""The weighted / focal three-head loss of csrc/heads_loss.hip: mt_heads_loss_fwd_bwd through the C ABI, then ops.heads_loss /
compute_loss(loss=LossConfig) under autograd and one training step.

  parts and gradients: the float64 reference within the rules of tests/heads_loss_ref.py (K_L, K_G; the code under test sets neither)
  total, masked gradients, non-finite values in masked frames, repeatability, NULL gradients, refusals:   EXACT (bit for bit)
  default settings: today's composition (mt_onset_offset_targets + 3 x mt_bce_masked_fwd_bwd) within the sum of both kernels' rules

Inputs, reference and rules come from tests/heads_loss_ref.py and tests/post_optim_ref.py (numpy only; tests/test_heads_loss_cpu.py checks
them without a GPU); DESIGN 6b "Weighted and focal loss" holds the derivations.  Every output lies in a sentinel-filled buffer between
two guard bands, and whatever the contract does not write must still hold the sentinel afterwards.

Every test prints the figure it is about to assert (`-s` shows them).  Run only this file:  python -m pytest tests/test_gpu_heads_loss.py -q -m gpu
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_loss_ref as H  # noqa: E402
import post_optim_ref as R  # noqa: E402

from oracle import model_ref as OR  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 256                                # elements of guard band on either side of every output
SENT32 = 0x7FC0BEEF                        # an f32 NaN pattern
MT_EINVAL, MT_EWORKSPACE = -1, -2
U = R.U
HW = H.HEAD_WEIGHTS
F3 = C.c_float * 3


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


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _say(what, **figs):
    print(f"MEASURED {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


class _Out:
    """n float32 words between two guard bands, all of it (the body too) pre-filled with a NaN sentinel"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), SENT32, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * 4

    def bits(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(np.uint32)

    def body(self):
        return self.bits().view(np.float32)

    def guards_ok(self):
        return bool((self.buf[:GUARD] == SENT32).all().item()) and bool((self.buf[GUARD + self.n:] == SENT32).all().item())

    def untouched(self):
        return bool((self.buf == SENT32).all().item())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _call(xs, roll, onr, lengths, hw=HW, pw=(1, 1, 1), gm=(0, 0, 0), grads=(True, True, True), ws_short=0, dims=None, null=(), no_ws=False):
    """xs: 1 or 3 logit arrays.  null: names among {"frame", "onset", "offset", "roll", "loss"} passed as NULL.  Gradient buffers are
    handed over for every head with grads[h], also for absent heads (the call must not write those)  -> (rc, loss _Out(4), [grad _Out or None] * 3)"""
    lib, st = _lib()
    B, P, T = xs[0].shape
    d = [_dev(x) for x in xs] + [None] * (3 - len(xs))
    rd, od, ld = _dev(roll), _dev(onr), _dev(None if lengths is None else np.asarray(lengths, dtype=np.int64))
    loss = _Out(4)
    g = [_Out(xs[0].size) if want else None for want in grads]
    nws = lib.mt_heads_loss_workspace_bytes() - ws_short
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device="cuda")
    ptrs = dict(frame=_p(d[0]), onset=_p(d[1]), offset=_p(d[2]), roll=_p(rd), loss=loss.ptr)
    for k in null:
        ptrs[k] = None
    rc = lib.mt_heads_loss_fwd_bwd(ptrs["frame"], ptrs["onset"], ptrs["offset"], ptrs["roll"], _p(od), _p(ld), R.n_valid_frames(lengths, B, T),
                                   F3(*hw), F3(*pw), F3(*gm), ptrs["loss"], *(x.ptr if x else None for x in g), None if no_ws else _p(ws), nws,
                                   *(dims or (B, P, T)), st)
    torch.cuda.synchronize()
    return rc, loss, g


def _check_against_ref(tag, xs, roll, onr, lengths, hw, pw, gm):
    """one call against the float64 reference -> (worst loss ratio, worst gradient ratio)"""
    B, P, T = xs[0].shape
    ref = H.heads_loss_ref(xs, roll, onr, lengths, hw, pw, gm)
    rc, loss, grads = _call(xs, roll, onr, lengths, hw, pw, gm)
    _ok(rc)
    assert loss.guards_ok() and all(g.guards_ok() for g in grads)
    got = loss.body()
    assert np.isfinite(got).all(), got
    assert loss.bits()[0] == _bits(H.total_of(got[1:]))[0], "total is not float32((frame + onset) + offset) of the parts"
    mask = R.valid_mask(lengths, B, P, T)
    rl = rg = 0.0
    for h in range(len(xs)):
        if ref["scales"][h] > 0:
            rl = max(rl, abs(float(got[1 + h]) - ref["parts"][h]) / H.loss_bound(ref["scales"][h]))
        else:
            assert loss.bits()[1 + h] == 0
        gh = grads[h].body().reshape(B, P, T)
        assert (_bits(gh)[~mask] == 0).all(), "a masked frame's gradient is not +0"
        assert np.isfinite(gh).all(), "a gradient was not written, or is not finite"
        rg = max(rg, float(np.abs(gh - ref["grads"][h]).max()) / H.grad_bound(hw[h], pw[h], ref["denom"]))
    for h in range(len(xs), 3):
        assert loss.bits()[1 + h] == 0 and grads[h].untouched()
    _say(tag, loss_ratio=rl, grad_ratio=rg)
    return rl, rg


# ================================================================== 1. against float64
@pytest.mark.parametrize("B,P,T", H.BPT)
def test_loss_parts_and_gradients_against_float64(mta, B, P, T):
    """|part_h - ref| <= K_L U head_weight sum|l| / denom; |grad - ref| <= K_G U head_weight max(w, 1) 1.5 / denom, exactly 0 in every masked
    frame; total = float32((frame + onset) + offset) bit for bit.  The planted logits (0, +-1e-7, +-20, +-100; -100 under a target of 1 and
    +100 under 0 among them) give finite values inside the rules."""
    worst_l = worst_g = 0.0
    for xs, roll, onr, lengths, pw, gm in H.cases(B, P, T):
        tag = f"heads loss ({B},{P},{T}) soft={bool(((roll != 0) & (roll != 1)).any())} given_onset={onr is not None} " \
              f"lengths={None if lengths is None else lengths.tolist()} w={pw} g={gm}"
        rl, rg = _check_against_ref(tag, xs, roll, onr, lengths, HW, pw, gm)
        worst_l, worst_g = max(worst_l, rl), max(worst_g, rg)
        assert rl <= 1 and rg <= 1
    _say(f"heads loss ({B},{P},{T}) worst", loss_ratio=worst_l, grad_ratio=worst_g)


# ================================================================== 2. default settings against today's composition
def _composition(xs, roll, onr, lengths):
    """mt_onset_offset_targets + three mt_bce_masked_fwd_bwd calls, as ops.compute_loss(loss=None) makes them -> (parts f32 [3], total f32 as
    the chained accumulate gives it, grads [3])"""
    lib, st = _lib()
    B, P, T = xs[0].shape
    rd = _dev(roll)
    on, off = torch.empty_like(rd), torch.empty_like(rd)
    _ok(lib.mt_onset_offset_targets(_p(rd), _p(on), _p(off), B * P, T, st))
    ys = [rd, on if onr is None else _dev(onr), off]
    ld = _dev(None if lengths is None else np.asarray(lengths, dtype=np.int64))
    ws = torch.empty(lib.mt_bce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    parts, grads = np.zeros(3, np.float32), []
    for h in range(3):
        xd, l, g = _dev(xs[h]), torch.zeros(1, device="cuda"), torch.empty(B * P * T, device="cuda")
        _ok(lib.mt_bce_masked_fwd_bwd(_p(xd), _p(ys[h]), _p(ld), R.n_valid_frames(lengths, B, T), HW[h], 0, _p(l), _p(g), _p(ws), ws.numel(),
                                      B, P, T, st))
        torch.cuda.synchronize()
        parts[h] = l.item()
        grads.append(g.cpu().numpy().reshape(B, P, T))
    return parts, np.float32(np.float32(parts[0] + parts[1]) + parts[2]), grads


@pytest.mark.parametrize("B,P,T", H.BPT)
def test_default_settings_against_todays_composition(mta, B, P, T):
    """head weights (0.5, 0.25, 0.25), w = 1, gamma = 0: each part within the sum of the two kernels' loss rules of the composed launches'
    part, each gradient within the sum of the two gradient rules; the totals within the sum over the heads plus 4 U |total| (each side
    adds its three float32 parts in two rounded additions).  The reduction orders differ, so the bits may."""
    worst_l = worst_g = 0.0
    for xs, roll, onr, lengths, _, _ in H.cases(B, P, T):
        ref = H.heads_loss_ref(xs, roll, onr, lengths, HW, [1.0] * 3, [0.0] * 3)
        rc, loss, grads = _call(xs, roll, onr, lengths)
        _ok(rc)
        want_parts, want_total, want_grads = _composition(xs, roll, onr, lengths)
        got = loss.body()
        bounds = [H.loss_bound(ref["scales"][h]) + R.LOSS_K * U * ref["scales"][h] for h in range(3)]
        for h in range(3):
            err = abs(float(got[1 + h]) - float(want_parts[h]))
            assert err <= bounds[h], (h, err, bounds[h])
            worst_l = max(worst_l, err / bounds[h] if bounds[h] > 0 else 0.0)
            gb = H.grad_bound(HW[h], 1.0, ref["denom"]) + R.GRAD_K * U * HW[h] / ref["denom"]
            eg = float(np.abs(grads[h].body().reshape(B, P, T) - want_grads[h]).max())
            worst_g = max(worst_g, eg / gb)
            assert eg <= gb, (h, eg, gb)
        assert abs(float(got[0]) - float(want_total)) <= sum(bounds) + 4 * U * abs(ref["total"])
    _say(f"defaults against the composition ({B},{P},{T})", loss_ratio=worst_l, grad_ratio=worst_g)


# ================================================================== 3. row edges
@pytest.mark.parametrize("B,P,T", [(2, 5, 7), (9, 88, 33)])
@pytest.mark.parametrize("ones", [True, False])
def test_edge_targets_do_not_leak_across_row_boundaries(mta, B, P, T, ones):
    """a roll of ones, and a roll with a 1 in the last frame of a row and in the first frame of the next: with a hard target the gradient
    of a cell is negative exactly where its target is 1, so the sign pattern of the onset and offset gradients is the target pattern of
    mt_onset_offset_targets' definition, and their size is the reference's"""
    xs = [np.clip(x, -20, 20) for x in H.inputs(B, P, T, False)[0]]       # at +-100 a gradient underflows to 0 and has no sign
    roll = H.edge_roll(B, P, T, ones)
    pw, gm = (1.0, 4.0, 8.0), (0.0, 2.0, 1.5)
    rc, _, grads = _call(xs, roll, None, None, HW, pw, gm)
    _ok(rc)
    ys = H.targets3(roll)
    for h in (1, 2):
        g = grads[h].body().reshape(B, P, T)
        assert np.array_equal(g < 0, ys[h] == 1) and (g != 0).all(), f"head {h}: a target of 1 where the definition has none, or the reverse"
    if ones:
        assert not ys[1].any() and not ys[2].any()
    else:
        assert ys[1][..., T - 1].any() and not ys[1][..., :T - 1].any() and ys[2][..., 0].any() and not ys[2][..., 1:].any()
    rl, rg = _check_against_ref(f"row edges ({B},{P},{T}) ones={ones}", xs, roll, None, None, HW, pw, gm)
    assert rl <= 1 and rg <= 1


# ================================================================== 4. non-finite values in masked frames
@pytest.mark.parametrize("B,P,T", H.BPT[1:])
def test_nonfinite_values_in_masked_frames_change_nothing(mta, B, P, T):
    """NaN and +-Inf in every masked frame of the three logits, the roll and the onset roll: the four loss words and the three gradients keep
    the bits they have with zeros there (the last valid frame's offset target reads the first masked frame of the roll)"""
    xs, roll, onr = H.inputs(B, P, T, False)
    pw, gm = (4.0, 8.0, 0.5), (0.0, 1.5, 8.0)
    for lengths in R.length_vectors(B, T):
        x0n, rn, x0z, rz, count = R.plant_nonfinite(xs[0], roll, lengths)
        if count == 0:
            continue
        x1n, on_n, x1z, on_z, _ = R.plant_nonfinite(xs[1], onr, lengths)
        x2n, _, x2z, _, _ = R.plant_nonfinite(xs[2], roll, lengths)
        for given in (False, True):
            _, l1, g1 = _call([x0n, x1n, x2n], rn, on_n if given else None, lengths, HW, pw, gm)
            _, l0, g0 = _call([x0z, x1z, x2z], rz, on_z if given else None, lengths, HW, pw, gm)
            assert np.array_equal(l1.bits(), l0.bits()) and np.isfinite(l1.body()).all()
            mask = R.valid_mask(lengths, B, P, T).reshape(-1)
            for a, b in zip(g1, g0):
                assert np.array_equal(a.bits(), b.bits()) and (a.bits()[~mask] == 0).all()


# ================================================================== 5. argument handling
def test_single_head_null_gradients_repeatability_and_empty_batch(mta):
    B, P, T = 3, 88, 501
    xs, roll, onr = H.inputs(B, P, T, True)
    lengths = R.length_vectors(B, T)[0]
    pw, gm = (8.0, 1.0, 4.0), (1.5, 2.0, 0.0)
    # one head: onset and offset logits NULL; parts 2 and 3 are 0 and the other heads' gradient buffers stay untouched
    rl, rg = _check_against_ref("single head", xs[:1], roll, None, lengths, (1.0, 0.25, 0.25), pw, gm)
    assert rl <= 1 and rg <= 1
    # two calls give the same bits
    _, l, g = _call(xs, roll, onr, lengths, HW, pw, gm)
    _, l2, g2 = _call(xs, roll, onr, lengths, HW, pw, gm)
    assert np.array_equal(l.bits(), l2.bits()) and all(np.array_equal(a.bits(), b.bits()) for a, b in zip(g, g2)), "two calls differ"
    # any gradient pointer NULL: the loss and the other gradients keep their bits
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        rc, l3, g3 = _call(xs, roll, onr, lengths, HW, pw, gm, grads=want)
        _ok(rc)
        assert np.array_equal(l3.bits(), l.bits()) and l3.guards_ok()
        assert all(b is None or (np.array_equal(a.bits(), b.bits()) and b.guards_ok()) for a, b in zip(g, g3))
    # every length 0 (or negative): the four loss words exactly 0, every gradient all zero
    for empty in (np.zeros(B, dtype=np.int64), np.array([0, -3, 0], dtype=np.int64)):
        _, l4, g4 = _call(xs, roll, onr, empty, HW, pw, gm)
        assert (l4.bits() == 0).all() and all((a.bits() == 0).all() for a in g4)


def test_refusals_write_nothing(mta):
    B, P, T = 2, 5, 7
    xs, roll, onr = H.inputs(B, P, T, False)
    nan, inf = float("nan"), float("inf")
    cases = [dict(null=("frame",)), dict(null=("roll",)), dict(null=("loss",)), dict(no_ws=True), dict(null=("onset",)), dict(null=("offset",)),
             dict(null=("onset", "offset"), onr=onr), dict(dims=(0, P, T)), dict(dims=(B, 0, T)), dict(dims=(B, P, -1)),
             dict(pw=(1, 0, 1)), dict(pw=(1, 1, -4)), dict(pw=(inf, 1, 1)), dict(pw=(1, nan, 1)), dict(hw=(-0.5, 0.25, 0.25)),
             dict(hw=(0.5, nan, 0.25)), dict(hw=(0.5, 0.25, inf)), dict(gm=(-1, 0, 0)), dict(gm=(0, 8.001, 0)), dict(gm=(0, 0, nan)),
             dict(gm=(inf, 0, 0))]
    for kw in cases:
        kw = dict(kw)
        rc, l, g = _call(xs, roll, kw.pop("onr", None), None, **kw)
        assert rc == MT_EINVAL, kw
        assert l.untouched() and all(a.untouched() for a in g), kw
    rc, l, g = _call(xs, roll, None, None, ws_short=1)
    assert rc == MT_EWORKSPACE and l.untouched() and all(a.untouched() for a in g)
    # the limits themselves are accepted: gamma 8, head weight 0
    rc, l, g = _call(xs, roll, None, None, hw=(0.5, 0.0, 0.25), gm=(8.0, 0.0, 8.0))
    _ok(rc)
    assert l.bits()[2] == 0 and (g[1].bits() & 0x7FFFFFFF == 0).all() and np.isfinite(l.body()).all()


# ================================================================== 6. autograd
def test_compute_loss_with_a_config_under_autograd(mta):
    B, P, T = 2, 5, 7
    xs, roll, onr = H.inputs(B, P, T, False)
    lengths = np.array([T, 4], dtype=np.int64)
    cfg = mta.LossConfig(head_weights=(0.5, 0.3, 0.2), pos_weight=(1, 8, 4), focal_gamma=(0, 2, 1.5))
    rc, loss, grads = _call(xs, roll, None, lengths, cfg.head_weights, cfg.pos_weight, cfg.focal_gamma)
    _ok(rc)
    lt = torch.from_numpy(lengths)
    for scale in (1.0, 3.0):
        leaf = {k: _dev(x).requires_grad_(True) for k, x in zip(("frame", "onset", "offset"), xs)}
        total = mta.compute_loss(leaf, _dev(roll), lt, loss=cfg)
        assert total.shape == () and _bits(total.item())[0] == loss.bits()[0]
        assert np.array_equal(_bits(mta.ops.heads_loss.last_parts.cpu().numpy()), loss.bits()) and not mta.ops.heads_loss.last_parts.requires_grad
        (total * scale).backward()
        for k, g in zip(("frame", "onset", "offset"), grads):
            assert np.array_equal(_bits(leaf[k].grad.cpu().numpy().reshape(-1)), _bits(np.float32(scale) * g.body())), (k, scale)
    # the {"frame", "onset"} dict of targets trains the onset head against the given roll; TranscriptionModel.compute_loss passes the config on
    _, loss_g, grads_g = _call(xs, roll, onr, lengths, cfg.head_weights, cfg.pos_weight, cfg.focal_gamma)
    leaf = {k: _dev(x).requires_grad_(True) for k, x in zip(("frame", "onset", "offset"), xs)}
    total = mta.compute_loss(leaf, {"frame": _dev(roll), "onset": _dev(onr)}, lt, loss=cfg)
    total.backward()
    assert _bits(total.item())[0] == loss_g.bits()[0] and loss_g.bits()[2] != loss.bits()[2]
    assert np.array_equal(_bits(leaf["onset"].grad.cpu().numpy().reshape(-1)), grads_g[1].bits())
    # a single tensor: element 0 of the settings, head weight 1; only the heads that need a gradient get one
    _, loss_1, grads_1 = _call(xs[:1], roll, None, lengths, (1.0, 0.0, 0.0), cfg.pos_weight, cfg.focal_gamma)
    x0 = _dev(xs[0]).requires_grad_(True)
    one = mta.heads_loss(x0, _dev(roll), lt, pos_weight=cfg.pos_weight, focal_gamma=cfg.focal_gamma)
    one.backward()
    assert _bits(one.item())[0] == loss_1.bits()[0] and np.array_equal(_bits(x0.grad.cpu().numpy().reshape(-1)), grads_1[0].bits())
    with torch.no_grad():
        again = mta.heads_loss(_dev(xs[0]), _dev(roll), lt, pos_weight=cfg.pos_weight, focal_gamma=cfg.focal_gamma)
    assert _bits(again.item())[0] == loss_1.bits()[0]
    # loss=None is today's path: what masked_bce gives, bit for bit
    d = {k: _dev(x) for k, x in zip(("frame", "onset", "offset"), xs)}
    on, off = mta.ops.onset_offset_targets(_dev(roll))
    want = (mta.ops.masked_bce(d["frame"], _dev(roll), lt, 0.5) + mta.ops.masked_bce(d["onset"], on, lt, 0.25)
            + mta.ops.masked_bce(d["offset"], off, lt, 0.25))
    assert torch.equal(mta.compute_loss(d, _dev(roll), lt, loss=None), want) and torch.equal(mta.compute_loss(d, _dev(roll), lt), want)
    assert torch.equal(mta.compute_loss(d["frame"], _dev(roll), lt, loss=None), mta.ops.masked_bce(d["frame"], _dev(roll), lt, 1.0))
    with pytest.raises(ValueError):
        mta.heads_loss(d["frame"], {"frame": _dev(roll), "onset": _dev(onr)}, lt)


# ================================================================== 7. one training step
def _tiny_large(mta, nm=16, hidden=16, layers=2, seed=5):
    m = mta.TranscriptionModel(model_type="cnn_rnn_large", n_mels=nm, hidden_size=hidden, num_layers=layers, dropout=0.0, device="cuda")
    m.load_state_dict(OR.make_state_dict("cnn_rnn_large", nm, hidden, layers, seed), strict=True)
    m.model.dropout2d_p = (0.0, 0.0, 0.0)
    return m


def test_one_training_step_logs_the_per_head_losses(mta):
    """train_one_epoch(all_heads=True) over the one batch of the fixture cache, from the same initial weights: with LossConfig() the logged
    step loss is the loss=None run's within the two kernels' loss rules (BCE terms are non-negative, so sum|l| is the part itself) plus
    4 U |total| for the float32 additions; the parts sum to the total; pos_weight (1, 8, 8) raises the onset part of that first batch."""
    ds = mta.CachedMaestroDataset(os.path.join(GOLDEN, "cache_fixture"), "train")
    batch = mta.collate_fn([ds[i] for i in range(len(ds))])
    dev = torch.device("cuda")

    def run(loss):
        m = _tiny_large(mta)
        opt = mta.make_optimizer(m, lr=1e-3)
        seen = []
        _, losses = mta.train_one_epoch(m, [batch], opt, dev, all_heads=True, loss=loss, log=lambda *a, **kw: seen.append((a, kw)))
        assert len(losses) == 1 and len(seen) == 1 and seen[0][0][:2] == (1, losses[0]) and np.isfinite(seen[0][0][2])
        return losses[0], seen[0][1]
    plain, kw = run(None)
    assert kw == {}                                                   # without a config the callback is called as it always was
    fused, kw = run(mta.LossConfig())
    parts = kw["parts"]
    assert list(parts) == ["frame", "onset", "offset"] and all(v > 0 for v in parts.values())
    bound = (H.K_L + R.LOSS_K) * U * sum(parts.values()) + 4 * U * abs(plain)
    _say("training step, LossConfig() against loss=None", plain=plain, fused=fused, err=abs(fused - plain), bound=bound)
    assert abs(fused - plain) <= bound
    assert _bits(fused)[0] == _bits(H.total_of([parts["frame"], parts["onset"], parts["offset"]]))[0]
    heavy, kw = run(mta.LossConfig(pos_weight=(1, 8, 8)))
    _say("training step, onset part", default=parts["onset"], pos_weight_8=kw["parts"]["onset"])
    assert kw["parts"]["onset"] > parts["onset"] and kw["parts"]["offset"] > parts["offset"]
    assert _bits(kw["parts"]["frame"])[0] == _bits(parts["frame"])[0] and heavy > fused
