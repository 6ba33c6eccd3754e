"""CPU tests of tests/heads_loss_ref.py, the reference, inputs, rules and float32 restatement behind tests/test_gpu_heads_loss.py, and of the
host side of the weighted / focal loss: LossConfig, the refusals of mt_heads_loss_fwd_bwd (made before any device call) and the flags of
scripts/train_cnn.py.  DESIGN 6b "Weighted and focal loss" has the derivations and the measured figures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_loss_ref as H  # noqa: E402
import post_optim_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARE = 0.5                                   # the restatement may use half of a rule
MT_EINVAL = -1


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


# ------------------------------------------------------------------ the reference
def test_reference_gradient_matches_central_differences():
    """d total / d logit of every cell of every head, against (total(x + h) - total(x - h)) / 2h in float64: within 1e-7 at h = 1e-5"""
    B, P, T = 2, 5, 7
    h, worst = 1e-5, 0.0
    for xs, roll, onr, lengths, pw, gm in H.cases(B, P, T)[::3]:
        xs64 = [x.astype(np.float64) for x in xs]
        ref = H.heads_loss_ref(xs64, roll, onr, lengths, H.HEAD_WEIGHTS, pw, gm)
        for k in range(3):
            for i in range(B * P * T):
                tot = []
                for s in (h, -h):
                    moved = [x.copy() for x in xs64]
                    moved[k].reshape(-1)[i] += s
                    tot.append(H.heads_loss_ref(moved, roll, onr, lengths, H.HEAD_WEIGHTS, pw, gm)["total"])
                worst = max(worst, abs((tot[0] - tot[1]) / (2 * h) - ref["grads"][k].reshape(-1)[i]))
    print(f"MEASURED central differences: worst |fd - grad| = {worst:.3g}")
    assert worst <= 1e-7


@pytest.mark.parametrize("B,P,T", H.BPT)
def test_reference_at_unit_weight_and_zero_gamma_is_the_bce_reference(B, P, T):
    for xs, roll, onr, lengths, _, _ in H.cases(B, P, T):
        ref = H.heads_loss_ref(xs, roll, onr, lengths, H.HEAD_WEIGHTS, [1.0] * 3, [0.0] * 3)
        nv = R.n_valid_frames(lengths, B, T)
        for h, y in enumerate(H.targets3(roll, onr)):
            loss, grad, scale = R.bce_ref(xs[h], y, lengths, nv, H.HEAD_WEIGHTS[h])
            assert abs(ref["parts"][h] - loss) <= 1e-13 * scale + 1e-300
            assert abs(ref["scales"][h] - scale) <= 1e-13 * scale + 1e-300
            assert np.abs(ref["grads"][h] - grad).max() <= 1e-15 * H.HEAD_WEIGHTS[h] / ref["denom"]
            assert (ref["grads"][h][~R.valid_mask(lengths, B, P, T)] == 0).all()
        one = H.heads_loss_ref(xs[:1], roll, None, lengths, (1.0, 0.0, 0.0), [1.0] * 3, [0.0] * 3)
        assert abs(one["total"] - R.bce_ref(xs[0], roll, lengths, nv, 1.0)[0]) <= 1e-13 * one["scales"][0] + 1e-300 and one["parts"][1:] == [0.0, 0.0]


def test_gradient_factor_stays_below_1_5():
    """max |dl/dx| / max(w, 1) over x, for y in {0, 1} (a soft target mixes the two) and gamma up to 8: 1.436 at gamma = 8"""
    x = np.linspace(-60.0, 60.0, 1200001)
    worst = 0.0
    for g in (0.0, 0.5, 1.0, 1.5, 2.0, 4.0, 6.0, 8.0):
        for w in (0.5, 1.0, 8.0):
            for y in (0.0, 1.0):
                worst = max(worst, float(np.abs(H.cell64(x, y, w, g)[1]).max()) / max(w, 1.0))
    print(f"MEASURED max |dl/dx| / max(w, 1) = {worst:.4f}")
    assert 1.43 < worst < 1.44 < H.GRAD_FACTOR


def test_edge_targets_stay_inside_the_row():
    """mt_onset_offset_targets' definition: onset 0 at t = 0, offset 0 at t = T - 1, nothing taken across a row boundary"""
    for B, P, T in H.BPT[1:]:
        _, on, off = H.targets3(H.edge_roll(B, P, T, ones=True))
        assert not on.any() and not off.any()
        y = H.edge_roll(B, P, T, ones=False)
        _, on, off = H.targets3(y)
        assert not on[..., 0].any() and not off[..., T - 1].any()
        # the 1 in a row's last frame is an onset there (a rise from 0) and never an offset; the 1 in a row's first frame is an offset
        # there (a fall to 0) and never an onset
        assert np.array_equal(on, np.where(np.arange(T) == T - 1, y, 0).astype(np.float32))
        assert np.array_equal(off, np.where(np.arange(T) == 0, y, 0).astype(np.float32))
        for binary in (True, False):
            r = R.roll_inputs(B * P, T, binary).reshape(B, P, T)
            _, on, off = H.targets3(r)
            for t in range(T):
                assert np.array_equal(on[..., t], np.maximum(r[..., t] - r[..., t - 1], 0) if t else np.zeros((B, P), np.float32))
                assert np.array_equal(off[..., t], np.maximum(r[..., t] - r[..., t + 1], 0) if t + 1 < T else np.zeros((B, P), np.float32))
    given = np.full((1, 1, 3), 0.25, np.float32)
    assert H.targets3(np.ones((1, 1, 3), np.float32), given)[1] is not None and np.array_equal(H.targets3(np.ones((1, 1, 3), np.float32), given)[1], given)


def test_inputs_hold_the_planted_extremes():
    for B, P, T in H.BPT[1:]:
        for soft in (False, True):
            xs, roll, onr = H.inputs(B, P, T, soft)
            for x in xs:
                assert set(np.float32(R.PLANTED)) <= set(x.reshape(-1).tolist())
            assert (roll[xs[0] == -100] == 1).all() and (roll[xs[0] == 100] == 0).all() and (xs[0] == -100).any() and (xs[0] == 100).any()
            assert (onr[xs[1] == -100] == 1).all() and (onr[xs[1] == 100] == 0).all()
        seen = [set(), set(), set()]
        for _, _, _, _, pw, gm in H.cases(B, P, T):
            assert len({(w, g) for w, g in zip(pw, gm)}) == 3
            for h in range(3):
                seen[h].add((pw[h], gm[h]))
        assert all(s == set(H.WG) for s in seen)


@pytest.mark.parametrize("B,P,T", H.BPT)
def test_rules_hold_for_the_float32_restatement(B, P, T):
    worst_l = worst_g = 0.0
    for xs, roll, onr, lengths, pw, gm in H.cases(B, P, T):
        ref = H.heads_loss_ref(xs, roll, onr, lengths, H.HEAD_WEIGHTS, pw, gm)
        parts, total, grads = H.heads_loss_f32(xs, roll, onr, lengths, H.HEAD_WEIGHTS, pw, gm)
        assert np.isfinite(parts).all() and np.isfinite(total)
        for h in range(3):
            if ref["scales"][h] == 0:
                assert parts[h] == 0
            else:
                worst_l = max(worst_l, abs(float(parts[h]) - ref["parts"][h]) / H.loss_bound(ref["scales"][h]))
            worst_g = max(worst_g, float(np.abs(grads[h] - ref["grads"][h]).max()) / H.grad_bound(H.HEAD_WEIGHTS[h], pw[h], ref["denom"]))
    print(f"MEASURED heads-loss restatement ({B},{P},{T}): loss {worst_l:.3f} of the rule ({worst_l * H.K_L:.2f} U), "
          f"grad {worst_g:.3f} ({worst_g * H.K_G:.2f} U)")
    assert worst_l <= SPARE and worst_g <= SPARE


# ------------------------------------------------------------------ the host side
def test_loss_config_validation(mta):
    cfg = mta.LossConfig()
    assert cfg.head_weights == (0.5, 0.25, 0.25) and cfg.pos_weight == (1.0, 1.0, 1.0) and cfg.focal_gamma == (0.0, 0.0, 0.0)
    cfg = mta.LossConfig(pos_weight=4, focal_gamma=[0, 2, 8], head_weights=(1, 0, 0.5))
    assert cfg.pos_weight == (4.0, 4.0, 4.0) and cfg.focal_gamma == (0.0, 2.0, 8.0) and cfg.head_weights == (1.0, 0.0, 0.5)
    assert mta.LossConfig is mta.ops.LossConfig
    for bad in (dict(pos_weight=0), dict(pos_weight=(1, -1, 1)), dict(pos_weight=float("inf")), dict(pos_weight=(1, 1)),
                dict(head_weights=(0.5, -0.1, 0.25)), dict(head_weights=float("nan")), dict(focal_gamma=-0.5), dict(focal_gamma=(0, 0, 8.5)),
                dict(focal_gamma=float("nan")), dict(focal_gamma=(0, 0, 0, 0))):
        with pytest.raises(ValueError):
            mta.LossConfig(**bad)
    with pytest.raises(TypeError):
        mta.compute_loss(None, None, loss=(0.5, 0.25, 0.25))


def test_entry_point_refuses_bad_arguments_before_any_device_call(mta):
    """every MT_EINVAL case is decided on the host: the pointers below are never read (tests/test_gpu_heads_loss.py repeats the cases with
    sentinel-filled device buffers)"""
    from music_transcription_amd import _lib
    lib = _lib.lib
    assert lib.mt_heads_loss_workspace_bytes() == 512 * 3 * 8
    f3 = C.c_float * 3
    X = 0x1000                                                       # stands for a device pointer

    def call(xf=X, xo=X, xk=X, roll=X, onr=None, loss=X, ws=X, hw=(0.5, 0.25, 0.25), pw=(1, 1, 1), gm=(0, 0, 0), dims=(2, 88, 7)):
        return lib.mt_heads_loss_fwd_bwd(xf, xo, xk, roll, onr, None, 14, f3(*hw), f3(*pw), f3(*gm), loss, None, None, None, ws,
                                         lib.mt_heads_loss_workspace_bytes(), *dims, None)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(xf=None), dict(roll=None), dict(loss=None), dict(ws=None), dict(xo=None), dict(xk=None), dict(xo=None, xk=None, onr=X),
               dict(dims=(0, 88, 7)), dict(dims=(2, -1, 7)), dict(dims=(2, 88, 0)), dict(pw=(1, 0, 1)), dict(pw=(-2, 1, 1)), dict(pw=(1, 1, inf)),
               dict(pw=(nan, 1, 1)), dict(hw=(0.5, -0.25, 0.25)), dict(hw=(nan, 0, 0)), dict(hw=(0, inf, 0)), dict(gm=(-0.1, 0, 0)),
               dict(gm=(0, 8.5, 0)), dict(gm=(0, 0, nan))):
        assert call(**kw) == MT_EINVAL, kw
        assert "mt_heads_loss_fwd_bwd" in _lib.last_error()


def _script(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), *argv], capture_output=True, text=True, timeout=120)


def test_train_script_loss_flags():
    r = _script("--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--pos_weight", "--focal_gamma", "--head_weights"))
    large = ["--model", "cnn_rnn_large"]
    for argv, word in ((large + ["--pos_weight", "1", "8", "8"], "--train_all_heads"),                     # three values, frame-only loss
                       (["--focal_gamma", "0", "2", "2"], "--train_all_heads"),
                       (large + ["--head_weights", "0.5"], "--train_all_heads"),
                       (large + ["--train_all_heads", "--pos_weight", "1", "8"], "one value or three"),
                       (large + ["--train_all_heads", "--pos_weight", "1", "0", "8"], "--pos_weight"),
                       (large + ["--train_all_heads", "--focal_gamma", "9"], "--focal_gamma"),
                       (large + ["--train_all_heads", "--head_weights", "0.5", "-1", "0.25"], "--head_weights"),
                       (["--pos_weight", "x"], "invalid float")):
        r = _script(*argv)
        assert r.returncode == 2 and "usage:" in r.stderr and word in r.stderr, (argv, r.stderr[-500:])
