"""The resampling kernels of csrc/resample.hip through their two entry points, mt_resample_polyphase (resample_tiled_kernel or the thread-per-output
resample_polyphase_kernel) and mt_resample_poly (resample_poly_kernel, taps in natural order), against the float64 sum of tests/frontend_f64_ref.py
(resample64, checked on the CPU against scipy.signal.resample_poly by tests/test_frontend_f64_ref_cpu.py).

TAPS ARE RANDOM, uniform in [-1, 1] (seeded), and so are the samples: a dropped or misplaced tap moves an output by O(1), where the designed
low-pass of the other tests hides its end taps at 1e-6 of the peak.  int32 samples span the full range, so the 24-bit rounding of the conversion shows.

Bound (derived, not measured; frontend_f64_ref.resample_bound), per output sample, both entry points:
    |got - ref| <= (L + channels + 2) 2^-24 sum_k |x_k h_k|          L = taps per phase
Worst error / bound measured on an MI355X, per rate pair over all its cases (-s prints every case):
  160/441: worst error / bound  polyphase 0.106  natural 0.106
  1/3: worst error / bound  polyphase 0.083  natural 0.099
  2/1: worst error / bound  polyphase 0.083  natural 0.083
  3/2: worst error / bound  polyphase 0.071  natural 0.078
  5/7: worst error / bound  polyphase 0.077  natural 0.096
  320/441: worst error / bound  polyphase 0.157  natural 0.157
  forced fallback 160/441 stereo int16 n_out 5003: error / bound  tiled 0.067  thread-per-output 0.067

Which kernel runs (resample_tile_plan and the dispatch of mt_resample_polyphase; frontend_f64_ref.resample_tile_plan mirrors them and
test_case_list_reaches_every_kernel asserts this table):  P = min(up, 16) lowered to a divisor of 1024, MW = 1024 / P,
W = (MW - 1) down + ((P - 1) down) / up + 2 + L;  tiled if 1024 <= W <= 38912 and n_out >= 4096, else one thread per output.

  up/down    P   W (L = 37 / 64)    n_out < 4096    n_out >= 4096
  160/441   16   27863 / 27890      thread          tiled, 10 phase blocks (up % P = 0)
  1/3        1    3108 /  3135      thread          tiled, n_mblk = 4 .. 8
  2/1        2     550 /   577      thread          thread: W < 1024, the window is smaller than the result tile (the fallback at n_out >= 4096)
  3/2        2    1061 /  1088      thread          tiled, up % P = 1: the second phase of the last block is masked (q_ok, q0 + qq < up)
  5/7        4    1828 /  1855      thread          tiled, up % P = 1
  320/441   16   27842 / 27869      thread          tiled; natural-order taps (82 KB at L = 64) no longer fit resample_poly_kernel's LDS copy
Per pair, four configurations (channels 1, 2, 3, 8; the format rotates so that every (pair, format) and (channels, format) occurs):
  channels 1   L 37   n_pre_remove 0      n_out 1500, 5003, 5120
  channels 2   L 64   the plan's value    n_out 1500, 5003, 5120
  channels 3   L 37   the plan's value    n_out 4099;  an input of 20 frames (< L) with n_out 60 and 4096: both ends of the window hang off the input
  channels 8   L 64   n_pre_remove 0      n_out 700, 8192;  the 20-frame input likewise
The input ends L / 2 frames before the last output's window does, so the last outputs run off the end (k_lo), and with n_pre_remove = 0 the first
run off the start (k_hi).  test_forced_fallback runs 44.1 -> 16 kHz stereo int16, n_out = 5003, in a child process with MT_RESAMPLE_TILED=0.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_f64_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = [(160, 441), (1, 3), (2, 1), (3, 2), (5, 7), (320, 441)]
CHANNELS = [1, 2, 3, 8]
SHORT_IN = 20


def plan_pre_remove(h_len, down):
    """n_pre_remove of scipy.signal.resample_poly's plan for a filter of h_len taps"""
    half_len = (h_len - 1) // 2
    return (half_len + down - half_len % down) // down


def configs(pi):
    """(channels, fmt, L, n_pre_remove, [(n_in or None, n_out)]) of rate pair PAIRS[pi]"""
    up, down = PAIRS[pi]
    out = []
    for ci, ch in enumerate(CHANNELS):
        L = (37, 64)[ci % 2]
        h_len = L * up - up // 3
        npr = (0, plan_pre_remove(h_len, down), plan_pre_remove(h_len, down), 0)[ci]
        runs = [[(None, 1500), (None, 5003), (None, 5120)], [(None, 1500), (None, 5003), (None, 5120)],
                [(None, 4099), (SHORT_IN, 60), (SHORT_IN, 4096)], [(None, 700), (None, 8192), (SHORT_IN, 60), (SHORT_IN, 4096)]][ci]
        out.append((ch, (pi + ci) % 3, L, h_len, npr, runs))
    return out


def make_case(seed, up, down, channels, fmt, L, h_len, npr, n_in, n_out):
    rng = np.random.default_rng(seed)
    if n_in is None:
        n_in = max(L + 1, (n_out + npr) * down // up - L // 2)
    if fmt == 0:
        src = rng.integers(-32768, 32768, (n_in, channels)).astype(np.int16)
    elif fmt == 1:
        src = rng.integers(-2 ** 31, 2 ** 31, (n_in, channels)).astype(np.int32)
    else:
        src = rng.uniform(-1, 1, (n_in, channels)).astype(np.float32)
    h = rng.uniform(-1, 1, h_len).astype(np.float32)
    return src, h


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


GUARD = 64


def run_polyphase(src, channels, fmt, hp, up, down, npr, n_out):
    from music_transcription_amd._lib import lib, check, ptr, stream_ptr
    d_src, d_hp = torch.from_numpy(src).cuda(), torch.from_numpy(hp).cuda()
    y = torch.full((n_out + GUARD,), float("nan"), device="cuda")
    check(lib.mt_resample_polyphase(ptr(d_src), src.shape[0], channels, fmt, ptr(d_hp), hp.shape[1], up, down, npr, ptr(y), n_out, stream_ptr()),
          "mt_resample_polyphase")
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[n_out:]).all()                                       # nothing written past n_out
    return y[:n_out].astype(np.float64)


def run_natural(src, channels, fmt, h, up, down, npr, n_out):
    from music_transcription_amd._lib import lib, check, ptr, stream_ptr
    d_src, d_h = torch.from_numpy(src).cuda(), torch.from_numpy(h).cuda()
    y = torch.full((n_out + GUARD,), float("nan"), device="cuda")
    check(lib.mt_resample_poly(ptr(d_src), src.shape[0], channels, fmt, ptr(d_h), len(h), up, down, npr, ptr(y), n_out, stream_ptr()), "mt_resample_poly")
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[n_out:]).all()
    return y[:n_out].astype(np.float64)


def test_case_list_reaches_every_kernel():
    """the header's table, from the mirrored plan: tiled cases with P = 1, 2, 4 and 16 (two of them with up % P != 0), thread-per-output cases
    below 4096 outputs, and the fallback at n_out >= 4096 where W comes out 0"""
    tiled_P, ragged_P, fallback, small = set(), set(), 0, 0
    for pi, (up, down) in enumerate(PAIRS):
        for ch, fmt, L, h_len, npr, runs in configs(pi):
            assert (h_len + up - 1) // up == L
            P, W = F.resample_tile_plan(L, up, down)
            for n_in, n_out in runs:
                kind = F.resample_kernel(L, up, down, n_out)
                if kind == "tiled":
                    assert 1024 <= W <= 38 * 1024
                    tiled_P.add(P)
                    if up % P:
                        ragged_P.add((up, down))
                elif n_out >= 4096:
                    assert W == 0
                    fallback += 1
                else:
                    small += 1
    assert tiled_P == {1, 2, 4, 16} and ragged_P == {(3, 2), (5, 7)} and fallback >= 1 and small >= 6
    assert {F.resample_tile_plan(L, 2, 1)[1] for L in (37, 64)} == {0}
    seen = {(pi, ch, fmt) for pi in range(len(PAIRS)) for ch, fmt, *_ in configs(pi)}
    assert {(p, c) for p, c, _ in seen} == {(p, c) for p in range(6) for c in CHANNELS}                # pairwise cover
    assert {(p, f) for p, _, f in seen} == {(p, f) for p in range(6) for f in range(3)}
    assert {(c, f) for _, c, f in seen} == {(c, f) for c in CHANNELS for f in range(3)}


@pytest.mark.parametrize("pi", range(len(PAIRS)), ids=[f"{u}_{d}" for u, d in PAIRS])
def test_resamplers_match_float64(mta, pi):
    up, down = PAIRS[pi]
    worst = {"polyphase": 0.0, "natural": 0.0}
    for ci, (ch, fmt, L, h_len, npr, runs) in enumerate(configs(pi)):
        for n_in, n_out in runs:
            src, h = make_case(1000 * pi + 100 * ci + n_out, up, down, ch, fmt, L, h_len, npr, n_in, n_out)
            hp = F.polyphase_table(h, up)
            assert hp.shape == (up, L)
            ref, sabs = F.resample64_polyphase(src, ch, fmt, hp, up, down, npr, n_out)
            bound = F.resample_bound(sabs, L, ch)
            live = bound > 0                                                   # outputs whose window misses the input altogether are exactly 0
            assert live.mean() > (0.5 if n_in is None else 0.0) and np.abs(ref).max() > 0.1
            line = f"\n  {up}/{down} ch {ch} fmt {fmt} L {L} n_pre_remove {npr} n_in {src.shape[0]} n_out {n_out} [{F.resample_kernel(L, up, down, n_out)}]"
            for name, got in (("polyphase", run_polyphase(src, ch, fmt, hp, up, down, npr, n_out)),
                              ("natural", run_natural(src, ch, fmt, h, up, down, npr, n_out))):
                err = np.abs(got - ref)
                assert (got[~live] == 0.0).all(), (line, name)
                ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
                worst[name] = max(worst[name], ratio)
                line += f"  {name} error / bound {ratio:.3f}"
                j = int(np.argmax(err - bound))
                assert (err <= bound).all(), (line, name, j, got[j], ref[j], bound[j])
            print(line, end="")
    print(f"\n  {up}/{down}: worst error / bound  polyphase {worst['polyphase']:.3f}  natural {worst['natural']:.3f}")


# ================================================================== MT_RESAMPLE_TILED=0, read once per process: a child
FALLBACK = dict(up=160, down=441, channels=2, fmt=0, L=37, n_out=5003, seed=4242)


def _fallback_case():
    c = FALLBACK
    h_len = c["L"] * c["up"] - c["up"] // 3
    npr = plan_pre_remove(h_len, c["down"])
    src, h = make_case(c["seed"], c["up"], c["down"], c["channels"], c["fmt"], c["L"], h_len, npr, None, c["n_out"])
    return src, F.polyphase_table(h, c["up"]), npr


def test_forced_fallback(mta, tmp_path):
    c = FALLBACK
    assert F.resample_kernel(c["L"], c["up"], c["down"], c["n_out"]) == "tiled"
    src, hp, npr = _fallback_case()
    out = str(tmp_path / "fallback.npy")
    env = dict(os.environ, MT_RESAMPLE_TILED="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    thread = np.load(out)
    tiled = run_polyphase(src, c["channels"], c["fmt"], hp, c["up"], c["down"], npr, c["n_out"])
    ref, sabs = F.resample64_polyphase(src, c["channels"], c["fmt"], hp, c["up"], c["down"], npr, c["n_out"])
    bound = F.resample_bound(sabs, c["L"], c["channels"])
    assert thread.shape == ref.shape and (bound > 0).all()
    rt, rf = np.abs(tiled - ref) / bound, np.abs(thread - ref) / bound
    print(f"\n  forced fallback 160/441 stereo int16 n_out 5003: error / bound  tiled {rt.max():.3f}  thread-per-output {rf.max():.3f}")
    assert rt.max() <= 1.0 and rf.max() <= 1.0
    assert (np.abs(thread - tiled) <= 2.0 * bound).all()                       # the same sum, both inside the bound


def _child(out_path):
    assert os.environ.get("MT_RESAMPLE_TILED") == "0"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import music_transcription_amd  # noqa: F401
    c = FALLBACK
    src, hp, npr = _fallback_case()
    np.save(out_path, run_polyphase(src, c["channels"], c["fmt"], hp, c["up"], c["down"], npr, c["n_out"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        _child(sys.argv[2])
