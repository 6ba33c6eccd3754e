"""CPU tests of tests/post_optim_ref.py and tests/lstm_layout_ref.py, the references, generators, rules and layouts behind
tests/test_gpu_post_optim.py and tests/test_gpu_lstm_layouts.py: the references are checked against torch in float64 (autograd, clip_grad_norm_
and torch.optim.Adam), the count reference against the oracle's F1 on the committed golden, the layouts index by index against the formulas
of include/mt_hip.h, and every tolerance rule must hold for the float32 restatement of its kernel, on the GPU tests' own inputs, with a
factor 2 to spare (DESIGN 6j has the figures)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_layout_ref as L  # noqa: E402
import post_optim_ref as R  # noqa: E402

from oracle import model_ref as OR  # noqa: E402

F64 = torch.float64
SPARE = 0.5                                   # the restatement may use half of a rule


# ------------------------------------------------------------------ masked BCE
@pytest.mark.parametrize("B,P,T", R.BPT)
@pytest.mark.parametrize("soft", [False, True])
def test_bce_ref_matches_torch_float64_and_autograd(B, P, T, soft):
    x, y = R.bce_inputs(B, P, T, soft)
    for lengths in [None] + R.length_vectors(B, T):
        for weight in (1.0, 0.25):
            nv = R.n_valid_frames(lengths, B, T)
            loss, grad, scale = R.bce_ref(x, y, lengths, nv, weight)
            xt = torch.from_numpy(x).to(F64).requires_grad_(True)
            mask = torch.from_numpy(R.valid_mask(lengths, B, P, T).copy())
            per = torch.nn.functional.binary_cross_entropy_with_logits(xt, torch.from_numpy(y).to(F64), reduction="none")
            want = weight * (per * mask).sum() / max(nv * P, 1)
            want.backward()
            assert abs(loss - float(want.detach())) <= 1e-13 * max(scale, 1e-300) + 1e-300
            assert np.abs(grad - xt.grad.numpy()).max() <= 1e-15 * weight / max(nv * P, 1)
            assert scale >= abs(loss) and (grad[~R.valid_mask(lengths, B, P, T)] == 0).all()
            if lengths is not None:
                assert nv == sum(min(max(int(v), 0), T) for v in lengths)


def test_length_vectors_hold_every_edge():
    for B, _, T in R.BPT:
        seen = {int(v) for vec in R.length_vectors(B, T) for v in vec}
        assert {0, 1, T, T + 5, -3} <= seen and all(len(vec) == B for vec in R.length_vectors(B, T))
    assert len(R.length_vectors(9, 33)) == 1


@pytest.mark.parametrize("B,P,T", R.BPT)
def test_bce_rules_hold_for_the_float32_restatement(B, P, T):
    worst_l = worst_g = 0.0
    for soft in (False, True):
        x, y = R.bce_inputs(B, P, T, soft)
        if B * P * T >= 28:
            assert set(np.float32(R.PLANTED)) <= set(x.reshape(-1).tolist())
        for lengths in [None] + R.length_vectors(B, T):
            for weight in (1.0, 0.25):
                nv = R.n_valid_frames(lengths, B, T)
                loss, grad, scale = R.bce_ref(x, y, lengths, nv, weight)
                l32, g32 = R.bce_f32(x, y, lengths, nv, weight)
                if scale == 0:
                    assert float(l32) == 0.0
                else:
                    worst_l = max(worst_l, abs(float(l32) - loss) / (R.LOSS_K * R.U * scale))
                worst_g = max(worst_g, float(np.abs(g32 - grad).max()) / (R.GRAD_K * R.U * weight / max(nv * P, 1)))
    print(f"MEASURED bce restatement ({B},{P},{T}): loss {worst_l:.3f} of the rule, grad {worst_g:.3f}")
    assert worst_l <= SPARE and worst_g <= SPARE


def test_nonfinite_planting_touches_masked_frames_only():
    B, P, T = 9, 88, 33
    x, y = R.bce_inputs(B, P, T)
    lengths = R.length_vectors(B, T)[0]
    xn, yn, xz, yz, count = R.plant_nonfinite(x, y, lengths)
    mask = R.valid_mask(lengths, B, P, T)
    assert count == int((~mask).sum()) > 0
    assert np.array_equal(xn[mask], x[mask]) and np.array_equal(yz[mask], y[mask]) and not np.isfinite(xn[~mask]).any() and not np.isfinite(yn[~mask]).any()
    assert {"nan", "inf", "-inf"} == {str(v) for v in xn[~mask][:3]}
    nv = R.n_valid_frames(lengths, B, T)
    a, b = R.bce_ref(xn, yn, lengths, nv, 1.0), R.bce_ref(xz, yz, lengths, nv, 1.0)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ targets, threshold, counts
def test_onset_offset_ref_matches_the_oracle_and_plants_row_borders():
    for rows, T in R.ROWS_T[:4]:
        for binary in (True, False):
            y = R.roll_inputs(rows, T, binary)
            on, off = R.onset_offset_ref(y)
            ron, roff = OR.onset_offset_targets(torch.from_numpy(y)[None])
            assert np.array_equal(on, ron[0].numpy()) and np.array_equal(off, roff[0].numpy())
            if T == 1:
                assert not on.any() and not off.any()
    y = R.roll_inputs(10, 7, True)
    ends, starts = y[:-1, -1], y[1:, 0]
    assert {(1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)} == set(zip(ends.tolist(), starts.tolist()))
    on, off = R.onset_offset_ref(y)
    flat_on = np.maximum(np.diff(y.reshape(-1), prepend=0), 0).reshape(y.shape)          # what a kernel that ignores the rows would give
    assert not np.array_equal(flat_on, on)


@pytest.mark.parametrize("thr", R.THRESHOLDS)
def test_threshold_rule_leaves_out_little_and_fits_the_restatement(thr):
    x = R.predict_inputs(300 * 901)
    want, margin = R.predict_ref(x, thr)
    live = margin > R.PREDICT_K * R.U
    share = 1.0 - live.mean()
    print(f"MEASURED threshold {thr}: {share:.2e} of the cells left out")
    assert share <= 1e-3
    assert np.array_equal(R.predict_f32(x, thr)[live], want[live])
    half = margin > 0.5 * R.PREDICT_K * R.U                                                # the restatement agrees at half the margin too
    assert np.array_equal(R.predict_f32(x, thr)[half], want[half])
    planted = np.array([0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert R.predict_ref(planted, 0.5)[0].tolist() == [0, 1, 0, 0]


def test_f1_counts_ref_matches_the_oracle_on_the_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "f1.npz"))
    yt, yp = g["y_true"].reshape(-1, 88, 20), g["y_pred"].reshape(-1, 88, 20)
    lens = np.array([20, 7, 0, 13, 25, 1, -3, 19])[:yt.shape[0]]
    for lengths in (None, lens):
        c = R.f1_counts_ref(yp, yt, lengths)
        for b in range(yt.shape[0]):
            n = 20 if lengths is None else min(max(int(lengths[b]), 0), 20)
            tp, fp, fn = (int(v) for v in c[b])
            f1 = 0.0 if 2 * tp + fp + fn == 0 else 2.0 * tp / (2 * tp + fp + fn)
            assert abs(f1 - OR.f1_binary(yt[b, :, :n], yp[b, :, :n])) < 1e-12
            if lengths is None:
                assert abs(f1 - g["f1"][b]) < 1e-12
    pred, target = R.f1_inputs(9, 88, 33)
    assert (pred == 0.5).any() and np.isnan(pred).any() and (target == 0.5).any() and np.isnan(target).any()
    half = np.full((1, 1, 4), 0.5, dtype=np.float32)
    assert R.f1_counts_ref(half, np.ones((1, 1, 4), dtype=np.float32), None).tolist() == [[0, 0, 4]]


def test_sweep_thresholds_are_unsorted_with_one_repeat():
    for K in (5, 16):
        thr, (i, j) = R.sweep_thresholds(K)
        assert thr.size == K and thr[i] == thr[j] and i != j and list(thr) != sorted(thr)
    assert R.sweep_thresholds(1)[0].size == 1


# ------------------------------------------------------------------ Adam + clip
@pytest.mark.parametrize("wd,max_norm,scale", [(1e-5, 1.0, 1.0), (0.0, 0.0, 0.5), (1e-5, 1.0, 0.125)])
def test_adam_ref_matches_torch_clip_and_adam_with_skipped_parameters(wd, max_norm, scale):
    """three parameters in one flat buffer, the middle one left with grad None: clip_grad_norm_ and Adam skip it, as the keep ranges do"""
    n = 57
    ranges = [[0, 20], [31, 57]]
    p, g, m, v = R.adam_state(n, False)
    g = R.poison_outside(R.scale_to_norm(g, 3.0, scale, ranges), ranges)
    h = dict(R.hyper(wd, max_norm))
    parts = [torch.from_numpy(p[a:b]).to(F64).requires_grad_(True) for a, b in ([0, 20], [20, 31], [31, 57])]
    opt = torch.optim.Adam(parts, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"])
    state = (p.astype(np.float64), np.zeros(n), np.zeros(n))
    for step in range(1, 5):
        gs = g.astype(np.float64) * (1 + 0.1 * step)
        for q, (a, b) in zip(parts, ([0, 20], [20, 31], [31, 57])):
            q.grad = None if a == 20 else torch.from_numpy(scale * gs[a:b]).clone()
        live = [q for q in parts if q.grad is not None]
        tnorm = float(torch.nn.utils.clip_grad_norm_(live, max_norm if max_norm > 0 else float("inf")))
        opt.step()
        p1, m1, v1, norm, ok = R.adam_ref(state[0], gs, state[1], state[2], h, step, scale, ranges)
        assert ok and abs(norm - tnorm) <= 1e-14 * tnorm
        got = torch.cat([q.detach() for q in parts]).numpy()
        assert np.abs(p1 - got).max() <= 1e-13 and np.array_equal(p1[20:31], p[20:31].astype(np.float64))
        for q, (a, b) in zip(parts, ([0, 20], [20, 31], [31, 57])):
            if a != 20:
                assert np.abs(opt.state[q]["exp_avg"].numpy() - m1[a:b]).max() <= 1e-15
                assert np.abs(opt.state[q]["exp_avg_sq"].numpy() - v1[a:b]).max() <= 1e-16
        assert not m1[20:31].any() and not v1[20:31].any()
        state = (p1, m1, v1)


def test_adam_ref_skips_on_a_nonfinite_norm():
    p, g, m, v = R.adam_case(7, 1.0, False)
    for bad in (np.nan, np.inf):
        g2 = g.copy()
        g2[3] = bad
        p1, m1, v1, norm, ok = R.adam_ref(p, g2, m, v, R.hyper(1e-5, 1.0), 3)
        assert not ok and not np.isfinite(norm) and np.array_equal(p1, p) and np.array_equal(m1, m) and np.array_equal(v1, v)
        assert R.adam_f32(p, g2, m, v, R.hyper(1e-5, 1.0), 3)[4] is False


def test_adam_cases_cover_what_they_must():
    for n in R.ADAM_NS:
        cases = R.adam_cases(n)
        assert {c[0] for c in cases} == set(R.ADAM_NORMS) and {c[2] for c in cases} == set(R.ADAM_STEPS)
        assert {(c[0], c[4]) for c in cases} == {(a, b) for a in R.ADAM_NORMS for b in (1.0, 0.0)}
        assert {c[3] for c in cases} == {0.0, 1e-5} and {c[1] for c in cases} == {False, True}
    for n in (4099, 524365):
        r = R.keep_range_cases(n)["ragged16"]
        assert len(r) == 16 and any(lo == hi for lo, hi in r) and all(lo % 256 for lo, hi in r if hi > lo)
    assert set(R.keep_range_cases(7)) == {"inner", "single"} and R.keep_range_cases(7)["inner"] == [[1, 6]]
    p, g, m, v = R.adam_case(4099, 0.999, False, grad_scale=0.5)
    assert abs(R.adam_ref(p, g, m, v, R.hyper(0, 1), 1, 0.5)[3] - 0.999) < 1e-6


@pytest.mark.parametrize("n", R.ADAM_NS)
def test_adam_rules_hold_for_the_float32_restatement(n):
    w = dict(norm=0.0, m=0.0, v=0.0, p=0.0)
    runs = [(c, gs, None) for c in R.adam_cases(n) for gs in (1.0, 0.5, 0.125)]
    runs += [(c, 1.0, r) for c in R.adam_cases(n)[::5] for r in R.keep_range_cases(n).values()]
    for (norm, zero, step, wd, mx), gs, ranges in runs:
        p, g, m, v = R.adam_case(n, norm, zero, grad_scale=gs, keep_ranges=ranges)
        if ranges is not None:
            g = R.poison_outside(g, ranges)
        h = R.hyper(wd, mx)
        ref = R.adam_ref(p, g, m, v, h, step, gs, ranges)
        got = R.adam_f32(p, g, m, v, h, step, gs, ranges)
        bm, bv, bp = R.adam_bounds(p, g, m, v, h, step, gs, ranges)
        assert ref[4] and got[4] and abs(ref[3] - norm) <= 1e-6 * norm
        w["norm"] = max(w["norm"], abs(float(got[3]) - ref[3]) / (R.NORM_REL * ref[3]))
        w["m"] = max(w["m"], R.ratio(np.abs(got[1] - ref[1]), bm))
        w["v"] = max(w["v"], R.ratio(np.abs(got[2] - ref[2]), bv))
        w["p"] = max(w["p"], R.ratio(np.abs(got[0] - ref[0]), bp))
    print(f"MEASURED adam restatement n={n}: " + ", ".join(f"{k} {x:.3f}" for k, x in w.items()) + " of the rule")
    assert max(w.values()) <= SPARE


def test_adam_rules_catch_the_planted_mistakes():
    """the mistakes the issue names, made in the restatement: each must break a rule"""
    n, gs = 4099, 0.5
    p, g, m, v = R.adam_case(n, 0.999, False, grad_scale=gs)
    h = R.hyper(1e-5, 1.0)
    ref = R.adam_ref(p, g, m, v, h, 2, gs)
    bm, bv, bp = R.adam_bounds(p, g, m, v, h, 2, gs)
    p1, m1, v1, norm, _ = R.adam_f32(p, g, m, v, h, 2, 1.0)                   # grad_scale applied in the norm only
    assert np.abs(m1 - ref[1]).max() > bm.max() and R.ratio(np.abs(p1 - ref[0]), bp) > 1
    ranges = [[1, n - 1]]
    ref = R.adam_ref(p, g, m, v, h, 2, gs, ranges)
    bm, bv, bp = R.adam_bounds(p, g, m, v, h, 2, gs, ranges)
    late = R.adam_f32(p, g, m, v, h, 2, gs, [[2, n - 1]])                      # a segment that starts at lo + 1
    assert np.abs(late[0] - ref[0])[1] > bp[1] > 0 and np.abs(late[1] - ref[1])[1] > bm[1]
    assert R.adam_f32(p, R.poison_outside(g, ranges), m, v, h, 2, gs, None)[4] is False      # the norm counts a skipped element


# ------------------------------------------------------------------ LSTM layouts
def test_hx_and_cell_layouts_index_by_index_on_a_tiny_case():
    """B = 2, T = 2, H = 16: every index written out from hx[b/32][t][dir][k/16][((k/8)%2)*32 + b%32][k%8] and [b/32][t][dir][k/8][k%8][b%32]"""
    B, T, H = 2, 2, 16
    bits = (np.arange(B * T * 2 * H, dtype=np.uint16) + 0x3C00).reshape(B, T, 2, H)
    img = L.encode_hx(bits, 0x7E00)
    a = np.arange(B * T * 2 * H, dtype=np.float32).reshape(B, T, 2, H) + 1
    cimg = L.encode_cell(a, -7.0)
    assert img.size == 1 * T * 2 * 1 * 64 * 8 == L.hx_words(B, T, H) and cimg.size == 1 * T * 2 * 2 * 8 * 32 == L.cell_words(B, T, H)
    img6 = img.reshape(1, T, 2, 1, 64, 8)
    cimg6 = cimg.reshape(1, T, 2, 2, 8, 32)
    for b in range(B):
        for t in range(T):
            for d in range(2):
                for k in range(H):
                    assert img6[0, t, d, 0, (k // 8) * 32 + b, k % 8] == bits[b, t, d, k]
                    assert cimg6[0, t, d, k // 8, k % 8, b] == a[b, t, d, k]
    assert L.hx_index(1, 1, 1, 9, T, H) == ((1 * 2 + 1) * 64 + 32 + 1) * 8 + 1                      # one address by hand
    assert L.cell_index(1, 0, 1, 9, T, H) == ((0 * 2 + 1) * 2 + 1) * 256 + 1 * 32 + 1
    assert int((img == 0x7E00).sum()) == img.size - bits.size and int((cimg == -7.0).sum()) == cimg.size - a.size
    assert img6[0, 0, 0, 0, 2, 0] == 0x7E00 and img6[0, 0, 0, 0, 32 + 2, 0] == 0x7E00                 # slot b = 2 of either half is pad


@pytest.mark.parametrize("B,T,H", [(1, 1, 16), (5, 3, 16), (16, 4, 48), (33, 5, 32), (70, 3, 64), (40, 2, 512)])
def test_encoders_are_bijections_onto_the_live_slots(B, T, H):
    bits = L.distinct_f16_bits((B, T, 2, H), 1)
    if bits.size <= 63488:
        assert np.unique(bits).size == bits.size
    assert (((bits >> 10) & 31) != 31).all()
    b, t, d, k = L._grid(B, T, H)
    for index, words in ((L.hx_index, L.hx_words), (L.cell_index, L.cell_words)):
        idx = index(b, t, d, k, T, H).reshape(-1)
        assert np.unique(idx).size == idx.size and idx.min() >= 0 and idx.max() < words(B, T, H)
        assert words(B, T, H) - idx.size == (L.groups(B) * 32 - B) * T * 2 * H                        # the rest is batch padding, nothing else
    img = L.encode_hx(bits, 0x7E00)
    assert np.array_equal(L.decode_hx(img, B, T, H), bits) and img.size * 2 == L.groups(B) * T * 2 * (H // 8) * 512     # mt_lstm_hx_bytes
    a = bits.astype(np.float32)
    cimg = L.encode_cell(a, np.nan)
    assert np.array_equal(L.decode_cell(cimg, B, T, H), a) and cimg.size == L.groups(B) * T * 2 * (H // 8) * 256       # mt_lstm_cx_bytes / 4
    rows = L.rows_from_h(bits, H - 3 if H > 3 else H, 5, 5 + 2 * H + 3, 0x7BCD)
    assert rows.shape == (T * B, 5 + 2 * H + 3) and rows[(T - 1) * B + (B - 1), 5 + (H - 3) + 1] == bits[B - 1, T - 1, 1, 1]


def test_bf16_rounding_is_torchs():
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[((bits >> 10) & 31) != 31].astype(np.uint16)
    want = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16).float().to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(L.bf16_bits_rne(bits), want)
