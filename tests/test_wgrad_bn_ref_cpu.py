"""tests/wgrad_bn_ref.py without a GPU: the closed forms against float64 torch autograd, every exactness and separation condition, the restated
launch geometry, and -- as tests/test_lstm_rec_ref_cpu.py does for the recurrences -- that each subtle fault of W.FAULTS, applied to a reference,
moves at least one case beyond that case's acceptance rule (`==` for the exact cases, the derived bound for the bounded ones)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_bn_ref as W  # noqa: E402

F64 = torch.float64


# ------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("KH,KW", [(1, 1), (3, 3), (7, 3), (3, 1)])
def test_conv_wgrad_reference_equals_float64_autograd(KH, KW):
    for B, F, T in ((2, 3, 5), (1, 1, 4), (2, 2, 1)):
        P = W.conv_wgrad_case(B, F, T, 64, 32, KH, KW, edge=True)
        assert torch.equal(P.ref, W.conv_wgrad_autograd(P.hi, P.lo, P.x, KH, KW))
        P = W.conv_wgrad_case(B, F, T, 64, 32, KH, KW, lo=False)
        assert torch.equal(P.ref, W.conv_wgrad_autograd(P.hi, None, P.x, KH, KW))


def test_conv2_wgrad_reference_equals_float64_autograd():
    P = W.conv2_wgrad_case(2, 5, 17)
    assert torch.equal(P.dW, W.conv_wgrad_autograd(P.hi, P.lo, P.a1, 3, 3))
    assert bool((P.lo.sum((0, 1, 2)) != 0).all()) and torch.equal(P.db, P.hi.sum((0, 1, 2)))


def test_conv_wgrad_cases_are_exact_and_reach_what_they_claim():
    for B, F, T, KH, edge in W.CW_SHAPES:
        for Cout, Cin in W.CW_TILINGS:
            P = W.conv_wgrad_case(B, F, T, Cout, Cin, KH, 3, edge=edge) if (Cout, Cin) in ((64, 32), (256, 128)) else None
            if P is not None:
                W.assert_conv_wgrad_case(P)
            assert W.cw_ws_bytes(B, F, T, Cout, Cin, KH, 3) > 0
    assert {T for _, _, T, _, _ in W.CW_SHAPES} == {1, 63, 64, 65, 129}
    assert any(KH == 7 and F < 4 for _, F, _, KH, _ in W.CW_SHAPES) and any(KH == 3 and F == 1 for _, F, _, KH, _ in W.CW_SHAPES)
    assert W.cw_row_tiles(2, 3, 65, 7, 0)[1] == 0                       # KH = 7, F = 3: the outermost kernel rows have no dz row at all
    for name, (B, F, T, Cout, Cin, KH, KW) in W.CW_SPLIT_CASES.items():
        P = W.conv_wgrad_case(B, F, T, Cout, Cin, KH, KW)
        W.assert_conv_wgrad_case(P)
        W.assert_cw_split_case(name, P)
    assert W.cw_plan(64, 32, 1, 10 ** 6)[4] == W.CW_S_MAX
    assert all(W.cw_plan(co, ci, kh, 10 ** 6)[4] <= W.CW_S_MAX for co in (64, 128, 256, 512) for ci in (32, 64, 128, 256) for kh in (1, 3, 7))
    assert W.cw_ws_bytes(2, 3, 5, 96, 32, 3, 3) == 0 and W.cw_ws_bytes(2, 3, 5, 64, 48, 3, 3) == 0 and W.cw_ws_bytes(2, 3, 5, 64, 32, 3, 2) == 0


def test_conv2_cases_are_exact_and_cover_the_tile_counts():
    counts = []
    for B, F, T in W.CONV2_SHAPES:
        P = W.conv2_wgrad_case(B, F, T)
        W.assert_exact(P.units, "mt_conv2_wgrad")
        counts.append(W.conv2_tiles(B, F, T))
    assert min(counts) <= 2 and 36 <= max(counts) <= 48
    B, F, T = W.CONV2_SHAPES[-1]
    assert W.conv2_tiles_of(0, 1, B, F, T) == max(counts)                                  # one workgroup walks every tile
    assert len({W.conv2_tiles_of(w, 3, *W.CONV2_SHAPES[3]) for w in range(3)}) > 1         # unequal counts
    assert W.conv2_tiles_of(255, 256, B, F, T) == 0                                         # idle workgroups
    assert {v for s in W.CONV2_SHAPES for v in s[1:]} >= {1, 5, 16, 17, 33}


def test_rounding_case_bound_is_meaningful():
    P = W.conv_wgrad_rounding_case()
    assert float((P.tol / (P.ref.abs() + 1e-30)).median()) < 1e-2
    assert torch.allclose(P.ref, W.conv_wgrad_autograd(P.hi, P.lo, P.x, P.KH, P.KW), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ BatchNorm activation
@pytest.mark.parametrize("case", W.BN_BWD_CASES)
def test_bn_bwd_closed_form_equals_float64_autograd(case):
    B, F, T, C, two, relu, pool, mask, _ = case
    P = W.bn_bwd_real_case(B, F, T, C, two, relu, pool, mask)
    W.assert_bn_bwd_real_case(P)
    ref = W.bn_act_bwd_autograd(P.za, P.pa[2], P.pa[3], P.zb, P.pb[2] if two else None, P.pb[3] if two else None, P.mask, P.g, relu, pool)
    tight = dict(rtol=1e-9, atol=1e-11)
    assert torch.allclose(P.cf.a.dz, ref[0], **tight) and torch.allclose(P.cf.a.dgamma, ref[1], **tight) and torch.allclose(P.cf.dbeta, ref[2], **tight)
    if two:
        assert torch.allclose(P.cf.b.dz, ref[3], **tight) and torch.allclose(P.cf.b.dgamma, ref[4], **tight) and torch.allclose(P.cf.dbeta, ref[5], **tight)
    for t in W.bn_bwd_tolerances(P):
        if t is not None:
            assert bool(torch.isfinite(t[0]).all())


def test_bn_forward_reference_equals_torch_ops():
    P = W.bn_fwd_case(2, 5, 7, 64, True, 1, 1, True)
    y = (P.pa[2] * (torch.nan_to_num(P.za) - P.pa[0]) * P.pa[1] + P.pa[3]) + (P.pb[2] * (torch.nan_to_num(P.zb) - P.pb[0]) * P.pb[1] + P.pb[3])
    y = torch.nn.functional.max_pool2d(torch.relu(y).permute(0, 3, 1, 2), (2, 1)).permute(0, 2, 3, 1) * P.mask[:, None, None, :]
    assert torch.equal(y, P.ref)


def test_bn_cases_meet_their_conditions_and_cover_the_combinations():
    for B, F, T, C, two, relu, pool, mask, mode in W.BN_FWD_CASES:
        W.assert_bn_fwd_exact(W.bn_fwd_case(B, F, T, C, two, relu, pool, mask))
    for C in (32, 256):
        for pool in (0, 1):
            W.assert_bn_fwd_exact(W.bn_fwd_case(2, 5, 9, C, False, 1, pool, True, ties=True))
    f = W.BN_FWD_CASES
    assert {c[3] for c in f} == {32, 64, 128, 256} and {c[2] for c in f} == {1, 7, 64, 65, 937} and {c[8] for c in f} == {0, 1}
    assert any(c[6] and c[1] % 2 for c in f) and any(c[6] and not c[5] for c in f) and any(c[4] and c[6] and c[7] for c in f)
    for case in W.BN_BWD_CASES:
        W.assert_bn_bwd_int_case(W.bn_bwd_int_case(*case[:8]))
    b = W.BN_BWD_CASES
    assert {(c[4], bool(c[6]), c[5]) for c in b} == {(t, p, r) for t in (False, True) for p in (False, True) for r in (0, 1)}
    assert any(c[6] and c[1] % 2 for c in b) and any(c[4] and c[6] and c[7] for c in b) and {c[8] for c in b} == {"cl", "x"}
    n, ppb, g, _ = W.bn_bwd_grid(*W.BN_BWD_CAP[:4], W.BN_BWD_CAP[6])
    assert g == 2048 and n > 2 * g * ppb
    W.bn_fwd_cap_case.__doc__ and W.bn_fwd_grid(3, 47, 937, 256, 0)[2] == 8192


def test_lo_gain_is_what_two_pieces_buy():
    P = W.bn_bwd_real_case(2, 7, 13, 64, True, 1, 1, True)
    t = W.bn_bwd_tolerances(P)[0][0]
    assert W.lo_gain(P.cf.a.dz, t) > 4
    # the f32 restatement of the closed form on the CPU stays inside the bound
    f = lambda v: v.float()
    xa = (f(P.za) - f(P.pa[0])) * f(P.pa[1])
    m1, m2 = (P.cf.dbeta / P.cf.a.N).float(), (P.cf.a.dgamma / P.cf.a.N).float()
    dz32 = f(P.pa[2]) * f(P.pa[1]) * (f(P.cf.dy) - m1 - xa * m2)
    used = float(((dz32.double() - P.cf.a.dz).abs() / (t + 1e-300)).max())
    print(f"f32 restatement uses {used:.3g} of tol_dz")
    assert used <= 1


# ------------------------------------------------------------------ every listed fault is caught
def _wgrad_hit(fault):
    hits = []
    for (B, F, T, KH, edge), (Cout, Cin), KW in ((W.CW_SHAPES[0], (64, 32), 3), (W.CW_SHAPES[4], (64, 64), 3), (W.CW_SHAPES[1], (64, 32), 3)):
        a, b = W.conv_wgrad_case(B, F, T, Cout, Cin, KH, KW, edge=edge), W.conv_wgrad_case(B, F, T, Cout, Cin, KH, KW, edge=edge, wrong=fault)
        hits.append(not torch.equal(a.ref, b.ref))
    a, b = W.conv2_wgrad_case(2, 5, 17), W.conv2_wgrad_case(2, 5, 17, wrong=fault)
    hits.append(not torch.equal(a.dW, b.dW))
    return hits


def _bn_hit(fault):
    hits = []
    for case in W.BN_BWD_CASES:
        for build in (W.bn_bwd_int_case, W.bn_bwd_real_case):
            hits.append(W.bn_bwd_detected(build(*case[:8]), build(*case[:8], wrong=fault)))
    if fault == "mask_before_pool":
        for B, F, T, C, two, relu, pool, mask, mode in W.BN_FWD_CASES:
            hits.append(not torch.equal(W.bn_fwd_case(B, F, T, C, two, relu, pool, mask).ref, W.bn_fwd_case(B, F, T, C, two, relu, pool, mask, wrong=fault).ref))
    return hits


@pytest.mark.parametrize("fault", W.FAULTS)
def test_every_fault_moves_a_case_beyond_its_acceptance_rule(fault):
    wg = fault in ("lo_dropped", "lo_from_hi", "kw_shift", "kh_flip", "halo_wrap", "split_lost")
    hits = _wgrad_hit(fault) if wg else _bn_hit(fault)
    print(f"{fault}: caught by {sum(hits)} of {len(hits)} cases")
    assert any(hits), f"no case notices the fault '{fault}'"


def test_dropped_or_copied_lo_piece_of_bn_bwd_breaks_the_sum_rule():
    """lo = 0 or lo = hi: |hi + lo - dz| must exceed sum_bound somewhere (the rule the GPU test applies to the returned pieces)"""
    P = W.bn_bwd_real_case(2, 7, 13, 64, True, 1, 1, True)
    t = W.bn_bwd_tolerances(P)[0][0]
    dz = P.cf.a.dz
    hi = W.bf16_round(dz)
    for lo in (torch.zeros_like(hi), hi):
        assert bool(((hi + lo - dz).abs() > W.sum_bound(dz, t)).any())
    assert bool(((hi + W.bf16_round(dz - hi) - dz).abs() <= W.sum_bound(dz, t)).all())


# ------------------------------------------------------------------ helpers
def test_helper_references():
    src = torch.arange(12.0).reshape(3, 4)
    assert torch.equal(W.transpose_ref(src, 3, 4, 5, 6)[:4, :3], src.t()) and float(W.transpose_ref(src, 3, 4, 5, 6)[4:].abs().sum()) == 0
    s = torch.arange(400.0)
    n, st = (2, 3, 4, 5), (200, 30, 1, 4)
    assert torch.equal(W.gather4_ref(s, n, st, 0.5), 0.5 * torch.as_strided(s, n, st)) and W.gather4_takes_lds_kernel(n, st)
    assert not W.gather4_takes_lds_kernel((3, 4, 1, 16), (100, 20, 0, 1))
    w = torch.arange(4 * 2 * 3 * 5, dtype=torch.float32).reshape(8, 15)
    out = W.pack_wih_ref(w, 2, 4, 3, 5)
    assert out.shape == (16, 15) and float(out[1, 1 * 3 + 2]) == float(w[1, 2 * 5 + 1]) and float(out[2].abs().sum()) == 0
