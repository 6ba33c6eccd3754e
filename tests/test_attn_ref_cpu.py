"""CPU tests of tests/attn_ref.py, the generators, float64 references, bounds and float32 emulations behind tests/test_gpu_attn.py: every
generator runs, every precondition is asserted, the references are checked against torch float64 autograd, the plain emulations must fit the
bounds with half of each bound's f32 term (the 16-bit rounding terms are attained by a single rounding, so they are taken whole: DESIGN 6i),
and each planted mutation must break a bound or an equality of at least one case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

F64 = torch.float64


def _ratio(err, bound):
    err = err.nan_to_num(nan=1e300)
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


# ------------------------------------------------------------------ dropout_keep
def test_dropout_keep_replica_matches_the_scalar_form():
    idx = np.concatenate([np.arange(0, 300), np.array([2 ** 31 - 1, 2 ** 31, 2 ** 40 + 7, 4202499])])
    for seed, layer, p in ((0, 0, 0.5), (7, 3, 0.25), (2 ** 31 + 5, 255, 0.3), (123456, 9, 0.75)):
        v = R.dropout_keep(seed, layer, idx, p)
        assert [bool(x) for x in v] == [bool(R.dropout_keep_scalar(seed, layer, int(i), p)) for i in idx]
    big = R.dropout_keep(7, 3, np.arange(200000), 0.25)
    assert 0.74 < big.mean() < 0.76
    assert not np.array_equal(R.dropout_keep(7, 3, np.arange(64), 0.5), R.dropout_keep(8, 3, np.arange(64), 0.5))
    assert not np.array_equal(R.dropout_keep(7, 3, np.arange(64), 0.5), R.dropout_keep(7, 4, np.arange(64), 0.5))


# ------------------------------------------------------------------ fused attention
def test_fused_cases_cover_what_they_must():
    cases = R.fused_cases()
    for dt in ("f16", "bf16"):
        assert {c[2] for c in cases if c[0] == dt and c[1] == 192} == set(R.FUSED_TS)
        for dp in (64, 128, 192):
            assert {1, 40, 65, 257} <= {c[2] for c in cases if c[0] == dt and c[1] == dp}
    assert {c[3] for c in cases} == {1, 3} and {c[4] for c in cases} == {1, 2}
    assert {1, 5, 8, 12, 31, 32, 33, 40, 56, 63, 64, 65, 97, 129, 255, 256, 257, 513} <= set(R.FUSED_TS)
    assert [T for T in R.FUSED_TS if R.pi_mask_differs(T)] == [5, 8, 40, 56]           # where af_pi(rho) < kleft is not rho < kleft
    assert sorted(R.af_pi(r) for r in range(32)) == list(range(32)) and R.af_pi(4) == 8 and R.af_pi(12) == 12


@pytest.mark.parametrize("dt,dp,T,B,heads", R.fused_cases())
def test_fused_case_preconditions_and_emulation(dt, dp, T, B, heads):
    P = R.fused_case(dt, dp, T, B, heads)
    assert P.ld3 > 2 * P.Ca + heads * dp and P.ldo > heads * dp and P.Ca > heads * dp and P.ld3 % 8 == 0 and P.Ca % 8 == 0 and P.ldo % 8 == 0
    for x in (P.q, P.k, P.v):
        assert torch.equal(R.r16(x, dt), x)
    if T >= 5:
        hi, lo = R.clamp_fractions(P)
        assert hi >= 0.05 and lo >= 0.05
    assert 0.4 < float(P.v.abs()[P.v != 0].mean()) < 1.6 and bool((P.v > 0).any()) and bool((P.v < 0).any())
    if T > 1:
        vis = R.fused_key_visibility(P, R.fused_sample_rows(T))
        assert vis > 1, f"a key's absence would move no output by more than the bound ({vis:.3g})"
    # the reference against torch's own softmax
    q, k, v = (x.permute(1, 2, 0, 3) for x in (P.q, P.k, P.v))
    want = torch.softmax(torch.clamp(q @ k.transpose(-1, -2) * P.scale, -10, 10), -1) @ v
    assert float((want - P.ref).abs().max()) < 1e-13
    r = _ratio((R.emulate_fused(P) - P.ref).abs(), R.fused_bound(P, w32=0.5))
    assert r <= 1, f"the plain emulation is {r:.3g} times the bound away"


FUSED_MUTATIONS = {            # mutation -> a case it must break
    "mask_rho": ("f16", 192, 40, 1, 1), "skip_partial": ("bf16", 192, 33, 3, 1), "count_past_T": ("bf16", 192, 255, 3, 1),
    "clamp_after_exp": ("bf16", 64, 40, 3, 1), "no_clamp": ("bf16", 192, 513, 1, 2),
}


@pytest.mark.parametrize("mutation", sorted(FUSED_MUTATIONS))
def test_fused_mutation_breaks_the_bound(mutation):
    P = R.fused_case(*FUSED_MUTATIONS[mutation])
    assert _ratio((R.emulate_fused(P, mutation) - P.ref).abs(), R.fused_bound(P)) > 1


def test_fused_mask_mutation_breaks_every_T_where_the_masks_differ():
    for T in R.FUSED_TS:
        P = R.fused_case("bf16", 192, T, 1, 1)
        broken = _ratio((R.emulate_fused(P, "mask_rho") - P.ref).abs(), R.fused_bound(P)) > 1
        assert broken == R.pi_mask_differs(T), T


def test_fused_row_sum_from_the_rounded_p_is_not_separable():
    """with the row sum taken from the rounded P the result is the exact quotient of the rounded terms -- its error is bounded by
    the same two 16-bit terms, and at T = 1 it is even exact.  No bound that admits the kernel can refuse it; recorded here as a fact."""
    for c in (("f16", 192, 1, 3, 2), ("bf16", 192, 129, 1, 2)):
        P = R.fused_case(*c)
        assert _ratio((R.emulate_fused(P, "sum_rounded_p") - P.ref).abs(), R.fused_bound(P)) <= 1


@pytest.mark.parametrize("case", R.TRANSPOSE_V_CASES)
def test_transpose_v_cases(case):
    P = R.transpose_v_case(*case)
    assert len(np.unique(P.words)) == min(P.words.size, 30011) and (P.words != 0x7BCD).all() and (P.words != 0).all()
    assert np.array_equal(R.emulate_transpose_v(P, 0x7BCD)[:, :, :P.dp, :], P.want)
    assert not np.array_equal(R.emulate_transpose_v(P, 0x7BCD, "no_zero_fill")[:, :, :P.dp, :], P.want)       # T < Tp in every case
    assert any(c[4] % 64 for c in R.TRANSPOSE_V_CASES) and any(c[2] > R.ru(c[1], 64) for c in R.TRANSPOSE_V_CASES)
    assert {c[5] for c in R.TRANSPOSE_V_CASES} == {"qkv", "v0", "vca", "plain"}


# ------------------------------------------------------------------ unfused softmax
@pytest.mark.parametrize("rows,T,extra", R.SOFTMAX_SHAPES)
def test_softmax_case_and_emulations(rows, T, extra):
    P = R.softmax_case(rows, T, extra)
    assert rows % 4 and P.lds > T and P.ldp > T and P.Tp % 64 == 0 and P.Tp != T
    R.assert_clip_separated(P)
    a = P.S * float(np.float32(P.scale))
    if T > 1:
        assert bool((a > P.clip).any()) and bool((a < -P.clip).any())
    ref = R.softmax_reference(P)
    for dt in ("f16", "bf16"):
        out = R.emulate_softmax(P, dt)
        assert bool((out[:, T:] == 0).all())
        assert _ratio((out[:, :T] - ref).abs(), R.softmax_fwd_bound(P, ref, dt, w32=0.5)) <= 1
    for p in R.SOFTMAX_PS:
        keep = R.softmax_keep(P, p, 7, 3) if p > 0 else torch.ones((rows, T), dtype=torch.bool)
        want = ref * keep / (1 - p)
        out = R.emulate_softmax(P, "bf16", p, 7, 3)[:, :T]
        assert torch.equal(out != 0, keep)
        assert _ratio((out - want).abs(), R.softmax_fwd_bound(P, want, "bf16", p, w32=0.5)) <= 1
        g = R.softmax_bwd_reference(P, p, keep)
        got = R.emulate_softmax_bwd(P, p, 7, 3)[:, :T]
        assert _ratio((got - g).abs(), R.softmax_bwd_bound(P, g, p, keep, w32=0.5)) <= 1
        if p > 0 and rows > 1:
            # the dropout index row*Tp + j: another mask, and a backward that no longer fits
            assert not torch.equal(R.emulate_softmax(P, "bf16", p, 7, 3, mutate="index_Tp")[:, :T] != 0, keep)
            if T > 1:
                assert _ratio((R.emulate_softmax_bwd(P, p, 7, 3, mutate="index_Tp")[:, :T] - g).abs(), R.softmax_bwd_bound(P, g, p, keep)) > 1


def test_softmax_backward_reference_is_the_closed_form():
    P = R.softmax_case(5, 63, 0)
    keep = R.softmax_keep(P, 0.25, 1, 2)
    g = R.softmax_bwd_reference(P, 0.25, keep)
    pr = R.softmax_reference(P)
    dP = P.dP * keep / 0.75
    a = P.S * float(np.float32(P.scale))
    want = torch.where(a.abs() <= P.clip, pr * (dP - (dP * pr).sum(-1, keepdim=True)) * float(np.float32(P.scale)), torch.zeros_like(pr))
    assert float((g - want).abs().max()) < 1e-15


def test_softmax_clamp_edge():
    P = R.softmax_case(5, 65, 0, scale=0.25, clip=10.0, edge=True)
    R.assert_clip_separated(P)
    assert P.S[0, :2].tolist() == [40.0, -40.0] and float(P.S[0, 2]) > 40.0 and float(P.S[0, 3]) < -40.0
    keep = torch.ones((5, 65), dtype=torch.bool)
    g = R.softmax_bwd_reference(P, 0.0, keep)
    b = R.softmax_bwd_bound(P, g, 0.0, keep)
    assert bool((g[0, :2].abs() > 2 * b[0, :2]).all()) and bool((g[0, 2:4] == 0).all())          # torch.clamp passes the gradient AT the edge
    got = R.emulate_softmax_bwd(P)[:, :65]
    assert _ratio((got - g).abs(), R.softmax_bwd_bound(P, g, 0.0, keep, w32=0.5)) <= 1 and bool((got[0, 2:4] == 0).all())
    assert _ratio((R.emulate_softmax_bwd(P, mutate="clamp_exclusive")[:, :65] - g).abs(), b) > 1


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("n", R.LN_NS)
def test_ln_case_and_emulation(n, rows):
    P = R.ln_case(rows, n)
    assert len({P.ldr, P.ldp, P.ldy}) == 3 and min(P.ldr, P.ldp, P.ldy) > n
    assert abs(float(P.mean[0]) - 1000) < 5 and (n < 48 or 0.5 < float(P.var[0].sqrt()) < 2)
    want = torch.nn.functional.layer_norm(P.v, (n,), P.gamma, P.beta, float(np.float32(P.eps)))
    assert float((want - P.y).abs().max()) < 1e-9
    um, ur = R.ln_stats_ulps(P)
    for dt in ("f16", "bf16"):
        y, m, r = R.emulate_ln(P, dt)
        assert _ratio((y - P.y).abs(), R.ln_fwd_bound(P, dt, w32=0.5)) <= 1
        if n == 1:
            assert torch.equal(y[:, 0], R.r16(P.beta, dt).expand(rows))
        elif n >= 48:
            y1, _, _ = R.emulate_ln(P, dt, "one_pass")
            assert _ratio((y1 - P.y).abs(), R.ln_fwd_bound(P, dt)) > 1, "a one-pass variance must not fit"
    assert bool((torch.from_numpy(R.ulps32(m, P.mean.reshape(-1).numpy())) <= 0.5 * um).all())
    assert bool((torch.from_numpy(R.ulps32(r, P.rstd.reshape(-1).numpy())) <= 0.5 * ur).all())


@pytest.mark.parametrize("rows,n", R.LN_BWD_SHAPES)
def test_ln_bwd_case_and_emulation(rows, n):
    P = R.ln_case(rows, n, big_mean=False)
    dx, dg, db = R.ln_bwd_reference(P)
    gg = P.dy * P.gamma                                   # the closed form the kernel implements, against autograd
    closed = P.rstd * (gg - gg.mean(1, keepdim=True) - P.xhat * (gg * P.xhat).mean(1, keepdim=True))
    assert float((closed - dx).abs().max()) < 1e-12 and float(((P.dy * P.xhat).sum(0) - dg).abs().max()) < 1e-10
    bx, bg, bb = R.ln_bwd_bounds(P)
    hx, hg, hb = R.ln_bwd_bounds(P, w32=0.5)              # (the roundings of the stored f32 results themselves are taken whole)
    ex, part = R.emulate_ln_bwd(P)
    assert _ratio((ex - dx).abs(), hx) <= 1
    if rows == 1:                                         # one row: dgamma_j is five roundings of one product, each of which can be attained
        hg = bg
    assert _ratio((part[:, 0].sum(0) - dg).abs(), hg) <= 1 and _ratio((part[:, 1].sum(0) - db).abs(), hb) <= 1
    mx, _ = R.emulate_ln_bwd(P, "no_xhat_m2")
    assert _ratio((mx - dx).abs(), bx) > 1
    assert {r for r, _ in R.LN_BWD_SHAPES} >= {1, 1024, 1025, 2500} and (6, 2048) in R.LN_BWD_SHAPES and (6, 65) in R.LN_BWD_SHAPES


# ------------------------------------------------------------------ element-wise helpers
def test_elementwise_shapes_and_mutations():
    assert any(M * N > R.GRID_CAP for M, N, _ in R.ELEMENTWISE_SHAPES) and (1, 1, 1) in R.ELEMENTWISE_SHAPES
    assert any(N % 2 and ld > N for _, N, ld in R.ELEMENTWISE_SHAPES) and max(R.DROPOUT_F32_NS) > R.GRID_CAP
    M, N, ld = R.ELEMENTWISE_SHAPES[-1]
    f = lambda m, n, i: ((m * 7 + n) % 1000 + 1).astype(np.int64)                      # noqa: E731
    full = R.emulate_rowwise(f, M, N, -1)
    assert (full > 0).all()
    cut = R.emulate_rowwise(f, M, N, -1, mutate="one_pass")
    assert not np.array_equal(full, cut) and int((cut == -1).sum()) == M * N - R.GRID_CAP
    # the dropout index m*ld + n gives another mask as soon as ld != N and M > 1
    for (M, N, ld) in R.ELEMENTWISE_SHAPES[1:3]:
        assert not np.array_equal(R.dropout_rows_keep(M, N, 0.5, 11, 5), R.dropout_rows_keep(M, N, 0.5, 11, 5, ld=ld + 3, mutate="index_ld"))
    assert np.array_equal(R.dropout_rows_keep(3, 7, 0.5, 11, 5).reshape(-1), R.dropout_keep(11, 5, np.arange(21), 0.5))


def test_dropout_scaling_at_p_03_is_within_one_ulp():
    """1 - 0.3f is exact in f32; ks = fl(1 / 0.7f) carries a relative error below 2^-25, so x ks rounded once is within 1 ulp of x / 0.7f
    (1/2 ulp of the product + |delta ks| 2^24 ulps < 1/2)"""
    f = np.float32
    one_minus = f(1.0) - f(0.3)
    assert float(one_minus) == 1.0 - float(f(0.3))
    ks = f(1.0) / one_minus
    assert abs(float(ks) * float(one_minus) - 1.0) < 2.0 ** -25
    x = (np.random.default_rng(0).random(1 << 20, dtype=np.float32) + f(0.5))
    assert R.ulps32(x * ks, x.astype(np.float64) / float(one_minus)).max() <= 1


def test_tie_words_and_specials():
    v = R.tie_words_f32(30000)
    assert int(((v.view(torch.int32) & 0xFFFF) == 0x8000).sum()) > 9000
    assert np.isnan(R.SPECIALS_F32[2]) and np.float32(R.SPECIALS_F32[2]).view(np.uint32) == 0x7FC00000
    w = R.position_words(4100, 1025)
    assert (w != 0).all() and (w != 0x7BCD).all() and (w[0, :7] != w[1, :7]).all()
