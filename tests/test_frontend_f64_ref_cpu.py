"""tests/frontend_f64_ref.py checked on the CPU: mel_power64 against oracle.frontend_ref.melspectrogram (to the float32 level: the oracle rounds the
spectrum to complex64 and multiplies in float32) and against torch.stft in float64 (1e-12), the closed form of the impulse cases against mel_power64,
the float32 yardstick against the figures the GPU tests' factor of 8 was chosen for, resample64 (vectorised, polyphase and as two plain loops)
against scipy.signal.resample_poly (1e-12), the derived resampler bound against a float32 emulation of the kernels' accumulation, and the host-only
mt_mel_filterbank_host against oracle.frontend_ref.mel_filterbank.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_f64_ref as F  # noqa: E402
from oracle import frontend_ref as FR  # noqa: E402

N = 16384


def _inputs():
    t = np.arange(N)
    return {"synth": FR.synth_audio(1, N, seed=3)[0],
            "noise": (0.1 * np.random.default_rng(0).standard_normal(N)).astype(np.float32),
            "tone": (0.5 * np.cos(2 * np.pi * 440.0 * t / 16000 + 0.3)).astype(np.float32)}


# ================================================================== mel
@pytest.mark.parametrize("n_mels", [320, 64])
def test_mel_power64_agrees_with_the_oracle_at_float32_level(n_mels):
    """The oracle keeps the FFT in float64 and rounds afterwards: the spectrum to complex64, |.| and the square in float32, then a float32 product of
    non-negative terms -- a relative error per bin of at most (taps + 6) 2^-24 (taps: the widest filter's non-zeros), no cancellation.
    Measured: e_frame <= 3.2e-7, e_bin <= 4.9e-7.  The float32 yardstick (FFT in float32 as well) measured 2.9e-7 / 3.7e-6 at worst: the level the
    GPU tests multiply by 8."""
    fb = FR.mel_filterbank(16000, 2048, n_mels)
    taps = int((fb != 0).sum(axis=1).max())
    for name, w in _inputs().items():
        ref = F.mel_power64(w, 512, fb)
        assert ref.dtype == np.float64 and ref.shape == (n_mels, 33)
        e_frame, e_bin, live = F.mel_errors(FR.melspectrogram(w, 16000, n_mels, 512), ref)
        assert live.all()
        assert e_frame <= 1e-6 and e_bin <= (taps + 6) * 2.0 ** -24, (name, e_frame, e_bin)
        bf, bb, e32f, e32b = F.mel_bounds(w, 512, fb, ref)
        print(f"n_mels {n_mels} {name}: oracle e_frame {e_frame:.2e} e_bin {e_bin:.2e}; float32 pipeline e_frame {e32f:.2e} e_bin {e32b:.2e}")
        assert 0 < e32f <= 1e-6 and 0 < e32b <= 1e-5, (name, e32f, e32b)          # the yardstick is float32, and no worse than float32
        assert bf == 8 * max(e32f, 1e-7) and bb == 8 * max(e32b, 1e-6)


@pytest.mark.parametrize("hop,n", [(512, N), (160, 4001), (1024, 1), (4096, N)])
def test_mel_power64_equals_torch_stft_float64(hop, n):
    w = FR.synth_audio(2, n, seed=5)
    fb = FR.mel_filterbank(16000, 2048, 64)
    S = torch.stft(torch.from_numpy(w).double(), 2048, hop, 2048, torch.hann_window(2048, periodic=True, dtype=torch.float64), center=True,
                   pad_mode="constant", return_complex=True).abs() ** 2
    want = (torch.from_numpy(fb).double() @ S).numpy()
    got = F.mel_power64(w, hop, fb)
    assert got.shape == want.shape == (2, 64, 1 + n // hop)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.allclose(F.mel_power64(w[1], hop, fb), got[1], rtol=1e-13, atol=0)          # one chunk alone: the same numbers (summation order may move)


def test_mel_errors_metric():
    R = np.array([[1.0, 1e-12, 2.0], [1e-5, 1e-13, 1.0], [0.5, 0.0, 1e-20]])           # (n_mels 3, T 3); frame 1 is below 1e-9: not live
    P = R.copy()
    P[0, 0] *= 1 + 1e-3                 # a strong bin: both metrics see it
    P[1, 0] *= 1.5                      # 1e-5 of the frame maximum: below e_bin's 1e-4 threshold, 5e-6 of the frame
    P[2, 2] = 5e-11                     # under the floor on both sides: no error
    P[1, 1] = 1.0                       # in the dead frame
    e_frame, e_bin, live = F.mel_errors(P, R)
    assert live.tolist() == [True, False, True]
    assert e_frame == pytest.approx(1e-3) and e_bin == pytest.approx(1e-3)
    assert F.mel_errors(R[:, 1:2], R[:, 1:2])[:2] == (0.0, 0.0)


def test_impulse_closed_form_equals_mel_power64():
    fb = FR.mel_filterbank(16000, 2048, 33)
    n = 4097
    for pos in (0, 1, 1023, 1024, 1025, 2600, 2601, n - 2, n - 1):
        w = np.zeros(n, np.float32)
        w[pos] = 1.0
        ref = F.mel_power64(w, 512, fb)
        assert np.abs(F.impulse_power64(n, pos, 512, fb) - ref).max() <= 1e-12 * ref.max(), pos


# ================================================================== filterbank (host only)
@pytest.mark.parametrize("n_mels", [320, 229, 64, 33])
def test_filterbank_host_equals_oracle(n_mels):
    """mt_mel_filterbank_host restates librosa.filters.mel operation by operation, roundings to float32 included.  Measured: array_equal at all four
    sizes (ulp distance 0), so exact equality is what is asserted."""
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as mta
    got, want = mta.mel_filterbank(16000, n_mels), FR.mel_filterbank(16000, 2048, n_mels)
    assert got.dtype == want.dtype == np.float32 and got.shape == (n_mels, 1025)
    assert np.array_equal(got, want)
    assert (got.sum(axis=1) > 0).all()


# ================================================================== resampler
def _random_case(seed, n_in, channels, fmt, h_len):
    rng = np.random.default_rng(seed)
    if fmt == 0:
        src = rng.integers(-32768, 32768, (n_in, channels)).astype(np.int16)
    elif fmt == 1:
        src = rng.integers(-2 ** 31, 2 ** 31, (n_in, channels)).astype(np.int32)
    else:
        src = rng.uniform(-1, 1, (n_in, channels)).astype(np.float32)
    return src, rng.uniform(-1, 1, h_len).astype(np.float32)


def _scipy_plan(h_proto, up, down, n_in):
    """scipy.signal.resample_poly's own padding of a given FIR (its upfirdn conventions) -> (h, n_pre_remove, n_out)"""
    n_out = (n_in * up + down - 1) // down
    half_len = (len(h_proto) - 1) // 2
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    return np.concatenate([np.zeros(n_pre_pad), h_proto.astype(np.float64) * up]), n_pre_remove, n_out


@pytest.mark.parametrize("up,down,channels,fmt,n_in,h_len", [(160, 441, 2, 0, 3000, 160 * 37 + 1), (3, 2, 3, 1, 500, 3 * 64 - 1), (5, 7, 1, 2, 20, 321)])
def test_resample64_equals_scipy_resample_poly(up, down, channels, fmt, n_in, h_len):
    from scipy.signal import resample_poly
    src, proto = _random_case(up + n_in, n_in, channels, fmt, h_len)
    mono = F.mono64(src, channels, fmt)
    want = resample_poly(mono, up, down, window=proto.astype(np.float64))
    h, npr, n_out = _scipy_plan(proto, up, down, n_in)
    assert len(want) == n_out
    got, sabs = F.resample64(src, channels, fmt, h, up, down, npr, n_out)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * scale
    L = (len(h) + up - 1) // up                                           # the polyphase table of the same float64 taps
    hp = np.concatenate([h, np.zeros(L * up - len(h))]).reshape(L, up).T
    got_p, sabs_p = F.resample64_polyphase(src, channels, fmt, hp, up, down, npr, n_out)
    assert np.abs(got_p - want).max() <= 1e-12 * scale and np.allclose(sabs_p, sabs, rtol=1e-12)
    assert (sabs >= np.abs(got) - 1e-12 * scale).all()
    m = min(n_out, 40)                                                    # the header's formula, literally
    assert np.abs(F.resample64_loops(src, channels, fmt, h, up, down, npr, m) - got[:m]).max() <= 1e-12 * scale


@pytest.mark.parametrize("up,down,L", [(160, 441, 37), (3, 2, 64), (2, 1, 37)])
def test_polyphase_sum_equals_natural_sum_and_the_bound_holds_for_float32(up, down, L):
    """the two orders of the taps give the same float64 sum; a float32 emulation of the kernels' loop (float32 mono, sequential fma-free accumulation,
    at least as lossy as fma) stays inside resample_bound, and dropping the last tap of a phase leaves it by orders of magnitude"""
    channels, fmt, n_in, n_out, npr = 3, 1, 700, 600 * up // down, 5
    src, h = _random_case(L * up, n_in, channels, fmt, L * up - 1)
    hp = F.polyphase_table(h, up)
    assert hp.shape == (up, L)
    a, sa = F.resample64(src, channels, fmt, h, up, down, npr, n_out)
    b, sb = F.resample64_polyphase(src, channels, fmt, hp, up, down, npr, n_out)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max() and np.allclose(sa, sb, rtol=1e-12)
    x32 = np.zeros(n_in, np.float32)
    for c in range(channels):
        x32 += src[:, c].astype(np.float32) * np.float32(1.0 / 2147483648.0)
    x32 /= np.float32(channels)
    cpos = (np.arange(n_out, dtype=np.int64) + npr) * down
    i_hi, ph = cpos // up, cpos % up
    acc = np.zeros(n_out, np.float32)
    for k in range(L):
        i = i_hi - k
        ok = (i >= 0) & (i < n_in)
        acc += np.where(ok, x32[np.clip(i, 0, n_in - 1)], np.float32(0)) * hp[ph, k]
    bound = F.resample_bound(sa, L, channels)
    ratio = np.abs(acc - a) / bound
    print(f"float32 emulation {up}/{down} L {L}: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    hp_cut = hp.copy()
    hp_cut[:, L - 2:] = 0.0                                                    # k_hi = L - 2
    c, _ = F.resample64_polyphase(src, channels, fmt, hp_cut, up, down, npr, n_out)
    assert np.median(np.abs(c - a) / bound) > 1e3


def test_tile_plan_mirror():
    """the geometry of resample_tile_plan / the dispatch of mt_resample_polyphase (csrc/resample.hip), on the rate pairs of the GPU test"""
    assert F.resample_tile_plan(37, 160, 441) == (16, 63 * 441 + (15 * 441) // 160 + 2 + 37)
    assert F.resample_tile_plan(495, 160, 441)[1] == 28321                                      # the header's 28.3 k frames
    assert F.resample_tile_plan(37, 1, 3) == (1, 1023 * 3 + 2 + 37)
    assert F.resample_tile_plan(64, 2, 1) == (2, 0)                                             # 511 + 0 + 2 + 64 < 1024: does not fit
    assert F.resample_tile_plan(37, 3, 2)[0] == 2 and F.resample_tile_plan(37, 5, 7)[0] == 4
    assert F.resample_kernel(37, 160, 441, 4095) == "thread" and F.resample_kernel(37, 160, 441, 4096) == "tiled"
    assert F.resample_kernel(37, 160, 441, 5000, tiled_enabled=False) == "thread"


def test_gpu_resample_case_list_reaches_every_kernel():
    """the case list of tests/test_gpu_resample_f64.py against the mirrored plan (importing that module touches no GPU)"""
    import test_gpu_resample_f64 as G
    G.test_case_list_reaches_every_kernel()
