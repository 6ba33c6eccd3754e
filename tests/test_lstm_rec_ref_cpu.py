"""tests/lstm_rec_ref.py checked on the CPU: the exact forward model against torch.nn.LSTM(bidirectional=True) in float64, the exact backward model
against torch autograd through an explicit float64 loop, the gx and dgx layout encoders index by index, and the DISCRIMINATING POWER of
tests/test_gpu_lstm_rec.py: on that module's own inputs, a recurrence that made one of seven plausible mistakes differs from the right one by at
least ten times the tolerance that module allows (the dgates per gate).  No GPU, nothing of the package under test."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_layout_ref as L  # noqa: E402
import lstm_rec_ref as R  # noqa: E402
import test_gpu_lstm_rec as G  # noqa: E402    (its header block: tolerances and cases; importing it touches no GPU)


# ================================================================== forward model == torch.nn.LSTM
@pytest.mark.parametrize("H,B,T,K", [(16, 3, 5, 7), (48, 3, 5, 20), (16, 2, 1, 5)])
def test_exact_forward_model_equals_torch_lstm(H, B, T, K):
    torch.manual_seed(H + T)
    lstm = torch.nn.LSTM(K, H, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, T, K, dtype=torch.float64)
    sfx = ("", "_reverse")
    with torch.no_grad():
        gx = torch.stack([x @ getattr(lstm, "weight_ih_l0" + s).t() + getattr(lstm, "bias_ih_l0" + s) + getattr(lstm, "bias_hh_l0" + s) for s in sfx], 2)
        w_hh = torch.stack([getattr(lstm, "weight_hh_l0" + s) for s in sfx]).numpy()
        h, c, gates = R.lstm_fwd(gx.reshape(B, T, 2, 4, H).numpy(), w_hh, False)
        y, _ = lstm(x)
        assert np.abs(y.reshape(B, T, 2, H).numpy() - h).max() < 1e-12
        for t in range(T):                                       # c of every step: the final cell state of the sequence cut there
            _, (_, cn) = lstm(x[:, :t + 1])
            assert np.abs(cn[0].numpy() - c[:, t, 0]).max() < 1e-12
            _, (_, cn) = lstm(x[:, t:])
            assert np.abs(cn[1].numpy() - c[:, t, 1]).max() < 1e-12
    assert gates[:, :, :, [0, 1, 3]].min() > 0 and gates[:, :, :, [0, 1, 3]].max() < 1 and np.abs(gates[:, :, :, 2]).max() < 1


# ================================================================== backward model == autograd
@pytest.mark.parametrize("H", [16, 48])
@pytest.mark.parametrize("T", [5, 1])
def test_exact_backward_model_equals_autograd(H, T):
    B = 3
    g = torch.Generator().manual_seed(H * 10 + T)
    gx = torch.randn(B, T, 2, 4 * H, generator=g, dtype=torch.float64) * 1.5
    w_hh = ((torch.rand(2, 4 * H, H, generator=g, dtype=torch.float64) * 2 - 1) * 3 / np.sqrt(H)).requires_grad_(True)
    dh = torch.randn(B, T, 2, H, generator=g, dtype=torch.float64)
    pres, hs, cs, gs = {}, {}, {}, {}
    for d in range(2):
        h = c = torch.zeros(B, H, dtype=torch.float64)
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            pre = gx[:, t, d] + h @ w_hh[d].t()
            pre.retain_grad()
            i, f, gg, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            pres[t, d], hs[t, d], cs[t, d], gs[t, d] = pre, h, c, torch.stack([i, f, gg, o], 1)
    sum((hs[t, d] * dh[:, t, d]).sum() for t in range(T) for d in range(2)).backward()
    pack = lambda m: torch.stack([torch.stack([m[t, d].detach() for d in range(2)], 1) for t in range(T)], 1).numpy()
    want = torch.stack([torch.stack([pres[t, d].grad for d in range(2)], 1) for t in range(T)], 1).reshape(B, T, 2, 4, H).numpy()
    got = R.lstm_bwd(pack(gs), pack(cs), dh.numpy(), w_hh.detach().numpy(), False)
    assert np.abs(want).max() > 0.05 and np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    # and the forward model gives the same saved tensors
    h, c, gates = R.lstm_fwd(gx.reshape(B, T, 2, 4, H).numpy(), w_hh.detach().numpy(), False)
    assert np.abs(h - pack(hs)).max() < 1e-12 and np.abs(c - pack(cs)).max() < 1e-12 and np.abs(gates - pack(gs)).max() < 1e-12


def test_rounding_points():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3, 1e-3, 0.0])
    assert np.array_equal(R.r_bf16(x), torch.from_numpy(x).float().bfloat16().double().numpy())       # ties to even: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    assert R.r_bf16(x)[1] == 1.0 and R.r_bf16(x)[2] == 1.0 + 2.0 ** -6
    assert np.array_equal(R.r_f16(x), torch.from_numpy(x).half().double().numpy())
    # the rounded flavours differ from the exact ones, by about the operand formats' precision
    gx, w = R.fwd_case(48, 3, 5)
    d = np.abs(R.lstm_fwd(gx, w, True)[0] - R.lstm_fwd(gx, w, False)[0]).max()
    assert 1e-5 < d < 5e-3
    gates, cx, dh, w = R.bwd_case(48, 3, 5)
    e, r = R.lstm_bwd(gates, cx, dh, w, False), R.lstm_bwd(gates, cx, dh, w, True)
    assert 1e-4 < np.abs(e - r).max() / np.abs(e).max() < 3e-2
    assert np.array_equal(r, R.r_bf16(r))                                                              # stored dgates are bf16 values


# ================================================================== the gx and dgx images
@pytest.mark.parametrize("B", [1, 17, 33])
@pytest.mark.parametrize("H", [16, 48])
def test_gx_and_dgx_encoders(B, H):
    T = 2
    n = B * T * 2 * 4 * H
    # ---- gx: [b/32][t][dir][k/8][gate][k%8][b%32]
    vals = (np.arange(n, dtype=np.float32) + 1).reshape(B, T, 2, 4, H)
    img = R.encode_gx(vals, -7.0)
    assert img.size == R.gx_words(B, T, H) == L.groups(B) * T * 2 * (H // 8) * 4 * 8 * 32 and img.dtype == np.float32
    assert np.array_equal(R.decode_gx(img, B, T, H), vals)
    assert np.count_nonzero(img == -7.0) == img.size - n and np.unique(img[img != -7.0]).size == n       # every index hit exactly once
    v7 = img.reshape(L.groups(B), T, 2, H // 8, 4, 8, 32)
    for b, t, d, p, k in ((0, 0, 0, 0, 0), (B - 1, 1, 1, 3, H - 1), (B // 2, 1, 0, 2, 9), (B - 1, 0, 1, 1, H - 8)):
        assert v7[b // 32, t, d, k // 8, p, k % 8, b % 32] == vals[b, t, d, p, k]
    assert np.array_equal(v7[-1, :, :, :, :, :, (B - 1) % 32 + 1:], np.full_like(v7[-1, :, :, :, :, :, (B - 1) % 32 + 1:], -7.0))
    half = R.encode_gx(vals / 64, 0.0, np.float16)                                                     # MT_GX_F16: the same index, f16 words
    assert half.dtype == np.float16 and np.array_equal(R.decode_gx(half, B, T, H), (vals / 64).astype(np.float16))
    # ---- dgx: image [b/32][t][dir][k/32] of 4096; img[2p + (u>>4)][((u>>3)&1)*32 + b%32][u&7]
    bits = (np.arange(n, dtype=np.uint32) + 1).astype(np.uint16).reshape(B, T, 2, 4, H)
    assert n < 0xFFFF
    dimg = R.encode_dgx(bits, 0xFFFF)
    nw = (H + 31) // 32
    assert dimg.size == R.dgx_words(B, T, H) == L.groups(B) * T * 2 * nw * 4096 and dimg.dtype == np.uint16
    assert np.array_equal(R.decode_dgx(dimg, B, T, H), bits)
    assert np.count_nonzero(dimg == 0xFFFF) == dimg.size - n and np.unique(dimg[dimg != 0xFFFF]).size == n
    v7 = dimg.reshape(L.groups(B), T, 2, nw, 8, 64, 8)
    for b, t, d, p, k in ((0, 0, 0, 0, 0), (B - 1, 1, 1, 3, H - 1), (B // 2, 1, 0, 2, 9), (B - 1, 0, 1, 1, 24 % H), (0, 1, 1, 2, 40 % H)):
        u = k % 32
        assert v7[b // 32, t, d, k // 32, 2 * p + (u >> 4), ((u >> 3) & 1) * 32 + b % 32, u & 7] == bits[b, t, d, p, k]
    if H == 48:                                                                                        # units 48 .. 63 of the second workgroup: padding
        assert (v7[:, :, :, 1, 1::2] == 0xFFFF).all()
    assert np.array_equal(R.bf16_bits_to_f64(np.array([0x3F80, 0xBF00, 0x0000], dtype=np.uint16)), np.array([1.0, -0.5, 0.0]))


# ================================================================== discriminating power
def _applies(wrong, B, T):
    if wrong in ("omit_kstep", "reverse_forward", "drop_carry", "omit_partial"):
        return T > 1                       # (T = 1 has no recurrent term, no carry and one walking order)
    if wrong == "batch_shift":
        return T > 1 and B > 1
    return True


def _fwd_cases():
    seen = []
    for cases, g16 in ((G.FWD_CASES, False), (G.G16_CASES, True), (G.TRAIN_CASES, False)):
        seen += [(c, g16) for c in cases if (c, g16) not in seen]
    return seen


@pytest.mark.parametrize("wrong", R.WRONG_FWD)
def test_gpu_forward_cases_discriminate(wrong):
    """every forward case of the GPU module (to which the mistake can apply at all): the wrong model's h is >= 10 x TOL_H_MAX away, and in train mode
    c and the gates by 10 x their tolerances too"""
    n = 0
    for (H, B, T), g16 in _fwd_cases():
        if not _applies(wrong, B, T):
            continue
        gx, w_hh = R.fwd_case(H, B, T, g16)
        good, bad = R.lstm_fwd(gx, w_hh, True), R.lstm_fwd(gx, w_hh, True, wrong=wrong)
        assert np.abs(good[0] - bad[0]).max() >= 10 * G.TOL_H_MAX, (wrong, H, B, T)
        assert np.abs(good[1] - bad[1]).max() >= 10 * G.TOL_C_MAX and np.abs(good[2] - bad[2]).max() >= 10 * G.TOL_G_MAX, (wrong, H, B, T)
        n += 1
    assert n >= 10


@pytest.mark.parametrize("wrong", R.WRONG_FWD)
def test_gpu_fused_projection_cases_discriminate(wrong):
    n = 0
    for H, B, T, Hv in G.XP_CASES:
        if not _applies(wrong, B, T):
            continue
        x_bits, w_ihx, bias, w_hh = R.xproj_case(H, B, T, Hv)
        xp = (x_bits.view(np.float16).astype(np.float64).reshape(B, T, 2 * H), w_ihx, bias)
        good, bad = R.lstm_fwd(None, w_hh, True, xproj=xp), R.lstm_fwd(None, w_hh, True, wrong=wrong, xproj=xp)
        assert np.abs(good[0] - bad[0]).max() >= 10 * G.TOL_H_MAX, (wrong, H, B, T)
        n += 1
    assert n >= 4


@pytest.mark.parametrize("wrong", R.WRONG_BWD)
def test_gpu_backward_cases_discriminate(wrong):
    """every backward case of the GPU module to which the mistake can apply: under the per-gate metric (R.dg_rel) at least one gate moves by 10 x its
    tolerance.  (Per gate because a wrong c_prev at the sequence end changes the f gate of one step only.  T = 2 is run at NW <= 3 only: after a
    single recurrent step one missing partial of NW is 1 / sqrt(NW) of W_hh^T dgates, itself a part of dh -- at NW = 16 a seventh of a gate's maximum,
    where nine steps compound it to a third.)"""
    n = 0
    for H, B, T in G.BWD_CASES:
        if not _applies(wrong, B, T):
            continue
        gates, cx, dh, w_hh = R.bwd_case(H, B, T)
        good, bad = R.lstm_bwd(gates, cx, dh, w_hh, True), R.lstm_bwd(gates, cx, dh, w_hh, True, wrong=wrong)
        moved = R.dg_rel(bad, good)
        assert (moved >= 10 * np.array(G.TOL_DG_REL)).any(), (wrong, H, B, T, moved)
        n += 1
    assert n >= 8


def test_dg_rel_metric():
    ref = np.zeros((2, 3, 2, 4, 16))
    ref[0, 0, 0, 0, 0], ref[1, 2, 1, 2, 5], ref[0, 1, 1, 3, 7] = 4.0, -0.5, 1.0             # the f gate stays all zero
    got = ref.copy()
    assert np.array_equal(R.dg_rel(got, ref), np.zeros(4))
    got[1, 1, 0, 0, 3] += 0.4
    got[0, 0, 0, 2, 0] -= 0.1
    assert np.allclose(R.dg_rel(got, ref), [0.1, 0.0, 0.2, 0.0])
    got[0, 0, 0, 1, 0] = 1e-30
    assert R.dg_rel(got, ref)[1] == np.inf
    assert R.exact_slack(np.array([0.5, -0.2])) == 8 * 2.0 ** -23 and R.exact_slack(np.array([3.0])) == 24 * 2.0 ** -23


def test_gpu_cases_cover_what_the_dispatch_can_launch():
    """the parametrisation of tests/test_gpu_lstm_rec.py read against launch_rec / lstm_fwd_impl / mt_lstm_bidir_bwd_ex"""
    nksw = lambda H: {1: 1, 2: 2, 3: 4, 4: 4}.get(-(-(H // 16) // 4), 8 if H <= 512 else 16)
    ng = lambda B: (B + 31) // 32
    for cases in (G.FWD_CASES, G.G16_CASES):
        assert {nksw(H) for H, B, T in cases if B <= 16} >= {1, 2, 4, 8, 16}                      # rec16 NK = 1, 1, 2, 4; H = 528: the 32-column kernel
        assert {nksw(H) for H, B, T in cases if B > 16} >= {1, 2, 4, 8, 16}
        assert {min(ng(B), 4) for H, B, T in cases if H <= 512} == {1, 2, 3, 4} and any(ng(B) == 5 for H, B, T in cases)
        assert {T for H, B, T in cases} == {1, 2, 11}
    assert {nksw(H) for H, B, T in G.TRAIN_CASES if B <= 16} >= {1, 2, 4, 8, 16} and {nksw(H) for H, B, T in G.TRAIN_CASES if B > 16} >= {1, 2, 4, 8, 16}
    assert {B for H, B, T in G.TRAIN_CASES} >= {1, 16, 17, 40, 70}
    assert {nksw(H) for H, B, T, Hv in G.XP_CASES} == {1, 2, 4, 8} and {B for H, B, T, Hv in G.XP_CASES} == {3, 32, 40} and any(Hv for H, B, T, Hv in G.XP_CASES)
    nw = lambda H: (H + 31) // 32
    assert {(nw(H) <= 8, B <= 16) for H, B, T in G.BWD_CASES} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {nw(H) for H, B, T in G.BWD_CASES} == {1, 2, 3, 8, 9, 13, 16}
    assert {B for H, B, T in G.BWD_CASES} == {1, 16, 17, 32, 40} and {T for H, B, T in G.BWD_CASES} == {1, 2, 9}
    # one workgroup per CU in the fused-projection kernel, all co-resident in the backward (the other forward grids: lstm_fwd_impl splits them)
    assert all(2 * (H // 8) * ng(B) <= 128 for H, B, T, Hv in G.XP_CASES) and all(2 * nw(H) * ng(B) <= 256 for H, B, T in G.BWD_CASES)
