"""CPU tests of tests/train_cnn_ref.py, the generators and float64 references behind tests/test_gpu_train_cnn.py: every generator runs,
every exactness and separation condition is asserted, and the closed forms (the dz formula of BatchNorm + ReLU + MaxPool2d((2,1)), the
routing with tie words) are checked against plain torch autograd in float64 on hand-built cases."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_cnn_ref as R  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("shape", R.CONV1_STATS_SHAPES)
def test_conv1_stats_case_is_exact_and_every_tap_matters(shape):
    P = R.conv1_stats_case(*shape)
    R.assert_exact(P.units, "conv1_stats")
    B, F, T = shape
    assert bool((P.x != 0).all()) and bool((P.w != 0).all())
    # dropping any one tap changes the sums (where that tap is ever inside the image)
    for k in range(9):
        kh, kw = divmod(k, 3)
        inside = (F > 1 or kh == 1) and (T > 1 or kw == 1)
        w2 = P.w.clone()
        w2[:, k] = 0
        z2 = torch.nn.functional.conv2d(P.x[:, None], w2.reshape(32, 1, 3, 3), P.bias, padding=1)
        s2 = torch.cat([z2.sum((0, 2, 3)), (z2 * z2).sum((0, 2, 3))])
        assert bool((s2 != P.sums).any()) == inside
    # by hand: one corner position
    z00 = P.bias.clone()
    for kh in range(3):
        for kw in range(3):
            if kh - 1 >= 0 and kw - 1 >= 0 and kh - 1 < F and kw - 1 < T:
                z00 += P.w[:, kh * 3 + kw] * P.x[0, kh - 1, kw - 1]
    assert torch.equal(z00, P.z[0, :, 0, 0])


def test_conv1_stats_shapes_cover_the_launch_geometry():
    n = [b * f * t for b, f, t in R.CONV1_STATS_SHAPES]
    assert (1, 1, 1) in R.CONV1_STATS_SHAPES and any(v < 256 for v in n) and any(256 < v <= 512 for v in n)
    assert any(R.conv1_stats_grid(*s) > 1 for s in R.CONV1_STATS_SHAPES) and any(s[0] == 3 for s in R.CONV1_STATS_SHAPES)
    assert any(s[1] % 2 and s[1] > 1 for s in R.CONV1_STATS_SHAPES) and any(s[1] % 2 == 0 for s in R.CONV1_STATS_SHAPES)


@pytest.mark.parametrize("case", R.BN_FINALIZE_CASES)
def test_bn_finalize_case(case):
    C, count, momentum = case[:3]
    P = R.bn_finalize_case(C, count, momentum)
    R.assert_bn_finalize_conditions(P)
    # against torch's BatchNorm on data with these sums: two values per channel reproduce any (sum, sum of squares) with count = 2
    if count == 2:
        s, q = torch.from_numpy(P.sums[:C]), torch.from_numpy(P.sums[C:])
        d = torch.sqrt(torch.clamp(q / 2 - (s / 2) ** 2, min=0))
        x = torch.stack([s / 2 - d, s / 2 + d])[:, :, None, None]                  # [2][C][1][1]
        bn = torch.nn.BatchNorm2d(C, eps=P.eps, momentum=P.momentum).double()
        bn.running_mean.copy_(torch.from_numpy(P.rmean).double())
        bn.running_var.copy_(torch.from_numpy(P.rvar).double())
        bn.train()
        bn(x)
        om = 1.0 - P.momentum
        np.testing.assert_allclose(bn.running_mean.numpy(), om * P.rmean.astype(np.float64) + P.momentum * P.mean, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(bn.running_var.numpy(), om * P.rvar.astype(np.float64) + P.momentum * P.unb, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(P.rmean_ref, bn.running_mean.numpy(), rtol=1e-7)       # (1 - momentum) in f32 or f64: 2^-25 apart
        np.testing.assert_allclose(P.rvar_ref, bn.running_var.numpy(), rtol=1e-6)
        assert np.all(np.abs(P.unb - 2 * np.maximum(P.raw_var, 0)) <= 1e-12 * P.unb)            # count / (count - 1) = 2


def test_ulps32():
    one = np.float32(1.0)
    nxt = np.nextafter(one, np.float32(2.0))
    assert R.ulps32(np.array([nxt]), np.array([1.0]))[0] == 1.0
    assert R.ulps32(np.array([one]), np.array([1.0 + 2.0 ** -24]))[0] == 0.5


@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_bn_stats_cases(C):
    Rr = R.bn_stats_rows(C)
    ns = R.bn_stats_ns(C)
    assert 1 in ns and Rr - 1 in ns and Rr + 1 in ns
    assert any(3 * Rr < n < 4 * Rr for n in ns)            # one workgroup, rows r + 3R of the four in flight partly out of range
    for N in ns:
        P = R.bn_stats_case(N, C)
        R.assert_exact(P.units, "bn_stats_cl")
        assert R.is_bf16(P.z)


@pytest.mark.parametrize("shape", R.BN_APPLY_SHAPES)
@pytest.mark.parametrize("ties", [False, True])
def test_bn_apply_cases(shape, ties):
    B, F, T, _ = shape
    P = R.bn_apply_case(B, F, T, ties=ties)
    R.assert_bn_apply_exact(P)
    if F % 2:
        assert bool(torch.isnan(P.z[:, F - 1]).all()) and not bool(torch.isnan(P.ref).any())
    # by hand, one element of a channel with negative gamma: the SMALLER z wins
    c = 1
    assert float(P.gamma[c] * P.rstd[c]) < 0 or ties
    z0, z1 = float(P.z[0, 0, 0, c]), float(P.z[0, 1, 0, c])
    f = lambda v: max(float(P.gamma[c]) * (v - float(P.mean[c])) * float(P.rstd[c]) + float(P.beta[c]), 0.0)  # noqa: E731
    assert float(P.ref[0, 0, 0, c]) == max(f(z0), f(z1))


def test_bn_apply_shapes_cover():
    s = R.BN_APPLY_SHAPES
    assert any(b == 1 for b, *_ in s) and any(b == 3 for b, *_ in s) and any(f % 2 for _, f, _, _ in s) and any(e > 0 for *_, e in s)
    assert any((b * (f // 2) * t) % 64 and b * (f // 2) * t > 64 for b, f, t, _ in s)


# ------------------------------------------------------------------ the closed form of the backward pass against autograd
def _hand_case():
    """B = 1, F = 5 (odd), T = 2, four channels: positive, negative and zero gamma, and one whose outputs are all negative.  Row pairs with
    equal z, and values chosen by hand so that both rows win somewhere."""
    za = torch.tensor([[1.0, -2.0], [1.0, 3.0],            # [F][T]; pair 0: a tie at t = 0 (first row), the second row is larger at t = 1
                       [-1.0, 2.0], [-3.0, 2.0],           # pair 1: first row larger at t = 0, a tie at t = 1
                       [0.25, 0.75]], dtype=F64)           # the single last row
    zb = torch.tensor([[0.5, 0.5], [0.5, -1.5], [2.5, 2.5], [-0.5, 2.5], [4.0, -4.0]], dtype=F64)
    z = torch.stack([za, zb, za, zb], -1)[None]                          # [1][5][2][4]
    gamma = torch.tensor([1.5, -0.75, 0.0, 0.5], dtype=F64)
    beta = torch.tensor([0.1, 0.2, 0.3, -5.0], dtype=F64)
    g = torch.tensor([[[1.0, -2.0, 3.0, 4.0], [0.5, 0.25, -1.0, 2.0]], [[-1.5, 2.0, 1.0, 1.0], [3.0, -0.5, 0.5, 1.0]]], dtype=F64)[None]
    return z, g, gamma, beta


def test_closed_form_matches_autograd_on_a_hand_built_case():
    z, g, gamma, beta = _hand_case()
    Rr = R.pool_bwd_closed(z, g, gamma, beta)
    dz, dgamma, dbeta = R.pool_bwd_autograd(z, g, gamma, beta)
    assert float((Rr.dz - dz).abs().max()) < 1e-13 and float((Rr.dgamma - dgamma).abs().max()) < 1e-13
    assert float((Rr.dbeta - dbeta).abs().max()) < 1e-13
    # routing, by hand: channel 0 (gamma > 0), pair 0, t = 0 is a tie -> first row; t = 1: the second row (3 > -2) wins
    assert float(Rr.dy[0, 0, 0, 0]) == 1.0 and float(Rr.dy[0, 1, 0, 0]) == 0.0
    assert float(Rr.dy[0, 0, 1, 0]) == 0.0 and float(Rr.dy[0, 1, 1, 0]) == 0.5
    # channel 1 (gamma < 0): the smaller z wins
    assert float(Rr.dy[0, 0, 1, 1]) == 0.0 and float(Rr.dy[0, 1, 1, 1]) == 0.25
    # channel 2 (gamma = 0): always the first row; channel 3: every output negative, no gradient at all
    assert bool((Rr.dy[0, 1::2, :, 2] == 0).all()) and bool((Rr.dy[0, 0:4:2, :, 2] == g[0, :, :, 2]).all())
    assert bool((Rr.dy[..., 3] == 0).all()) and bool((Rr.dz[..., 3] == 0).all())
    # the single last row of the odd F gets only the mean terms, and N counts it
    assert Rr.N == 10 and bool((Rr.dy[0, 4] == 0).all()) and bool((Rr.dz[0, 4, :, :2] != 0).all())
    # BatchNorm's two identities: sum dz = 0, and sum dz*xhat = k dgamma (1 - sum xhat^2 / N) = k dgamma eps rstd^2 (zero but for eps)
    assert float(Rr.dz.sum((0, 1, 2)).abs().max()) < 1e-13
    assert float(((Rr.dz * Rr.xhat).sum((0, 1, 2)) - R.dz_xhat_residual(Rr)).abs().max()) < 1e-13
    assert float(R.dz_xhat_residual(Rr).abs().max()) < 1e-4


@pytest.mark.parametrize("shape", R.POOL_BWD_SHAPES)
def test_pool_bwd_generator(shape):
    P = R.pool_bwd_case(*shape)
    R.assert_pool_bwd_case(P)
    dz, dgamma, dbeta = R.pool_bwd_autograd(P.z, P.dX, P.gamma, P.beta)
    scale = float(P.R.dz.abs().max())
    assert float((P.R.dz - dz).abs().max()) < 1e-12 * max(scale, 1.0)
    assert float((P.R.dgamma - dgamma).abs().max()) < 1e-11 and float((P.R.dbeta - dbeta).abs().max()) < 1e-11
    t_dz, t_dg, t_db = R.dz_tolerance(P.R, P.gamma, R.pool_bwd_geometry(*shape)[1] + 17)
    nz = P.R.dz.abs() > 1e-3 * scale
    # the bound is a rounding-error bound: parts in a million of the values, far below the 2^-9 of a lost second bf16 piece
    assert float((t_dz[nz] / P.R.dz.abs()[nz]).median()) < 2.0 ** -14


@pytest.mark.parametrize("shape", R.POOL_BWD_SHAPES)
def test_tie_word_routing_matches_autograd_on_the_unrounded_values(shape):
    """The tie words are the order of the conv's f32 results before their bf16 rounding.  Rebuild such values -- the bf16 z moved by a tiny
    amount in the direction the bits give -- and let autograd route on them: the closed form with tie words must give the same gradient."""
    P = R.pool_bwd_case(*shape, with_tie=True)
    R.assert_pool_bwd_case(P)
    gt, lt = P.tie
    Fo = P.F // 2
    delta = 1e-9
    zt = P.z.clone()
    zt[:, 0:2 * Fo:2] += delta * (gt.double() - lt.double()) * (P.z[:, 0:2 * Fo:2] == P.z[:, 1:2 * Fo:2])
    dz, dgamma, dbeta = R.pool_bwd_autograd(zt, P.dX, P.gamma, P.beta)
    scale = max(float(P.R.dz.abs().max()), 1.0)
    assert float((P.R.dz - dz).abs().max()) < 1e-6 * scale
    assert float((P.R.dbeta - dbeta).abs().max()) < 1e-6 * scale and float((P.R.dgamma - dgamma).abs().max()) < 1e-5 * scale
    # and it differs from the routing on the bf16 values alone (first row on every equal pair)
    plain = R.pool_bwd_closed(P.z, P.dX, P.gamma, P.beta)
    if P.B * Fo * P.T >= 20:
        assert bool((plain.dy != P.R.dy).any())
    words = R.pack_tie_words(P.tie)
    assert tuple(words.shape) == (P.B, Fo, P.T, 2, 2)
    b, fo, t, c = 0, Fo - 1, P.T - 1, 37
    assert bool((int(words[b, fo, t, 1, 0]) >> (c - 32)) & 1) == bool(gt[b, fo, t, c])
    assert bool((int(words[b, fo, t, 1, 1]) >> (c - 32)) & 1) == bool(lt[b, fo, t, c])


@pytest.mark.parametrize("shape", R.CONV1_BWD_SHAPES)
def test_conv1_bwd_generator(shape):
    P = R.conv1_bwd_case(*shape)
    R.assert_conv1_bwd_case(P)
    dW, db, dgamma, dbeta = R.conv1_bwd_autograd(P)
    dWc = torch.einsum("bftc,bftk->ck", P.R.dz, P.taps)
    s = max(float(dW.abs().max()), 1.0)
    assert float((dW - dWc).abs().max()) < 1e-12 * s and float(db.abs().max()) < 1e-12 * s       # db is analytically zero
    assert float((dgamma - P.R.dgamma).abs().max()) < 1e-12 * s and float((dbeta - P.R.dbeta).abs().max()) < 1e-12 * s
    t_dW, t_db, t_dg, t_dbeta, sabs = R.conv1_bwd_tolerances(P, R.conv1_bwd_geometry(*shape)[1])
    for t in (t_dW, t_db, t_dg, t_dbeta):
        assert bool(torch.isfinite(t).all()) and bool((t >= 0).all())
    if shape == (2, 9, 150):                                     # the bounds stay rounding-error bounds: parts in 10^4 of the sums of |addends|
        assert bool((t_db <= 1e-4 * sabs).all())
        assert bool((t_dW <= 1e-4 * torch.einsum("bftc,bftk->ck", P.R.dz.abs(), P.taps.abs())).all())


def test_conv1_bwd_shapes_cover():
    s = R.CONV1_BWD_SHAPES
    assert any(f == 2 for _, f, _ in s) and any(f % 2 and f > 2 for _, f, _ in s) and any(t == 1 for *_, t in s) and any(t == 2 for *_, t in s)
    assert any(b == 1 for b, *_ in s) and any(b == 3 for b, *_ in s)
    pos = [R.conv1_bwd_geometry(*c)[1] for c in s]
    assert any(b * ((f + 1) // 2) * t < 256 for b, f, t in s) and max(pos) >= 4


def test_rowsum_cases_are_exact():
    for rows in R.ROWSUM_ROWS:
        for n in R.ROWSUM_NS:
            P = R.rowsum_case(rows, n)
            R.assert_exact(P.units, "rowsum_bf16")
            assert R.is_bf16(P.a) and float(P.a[:, -1].abs().min()) > 0      # the last element always counts


def test_rounding_values_sit_on_and_beside_ties():
    v = R.rounding_values((3, 88, 67))
    tie = R.on_bf16_tie(v)
    assert 0.25 < float(tie.float().mean()) < 0.45
    r = v.to(torch.bfloat16).float()
    lo = (v.view(torch.int32) & ~0xFFFF).view(torch.float32)                  # truncation toward zero
    up = ((v.view(torch.int32) & ~0xFFFF) + 0x10000).view(torch.float32)
    even_lo = ((v.view(torch.int32) >> 16) & 1) == 0
    assert bool(torch.equal(r[tie], torch.where(even_lo, lo, up)[tie]))       # ties go to the even neighbour
    assert bool((v < 0).any()) and bool((v > 0).any())
