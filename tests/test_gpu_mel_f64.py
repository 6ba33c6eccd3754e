"""The log-mel kernels (csrc/mel_kernel.h: mel_kernel<false> behind mt_mel_db_f32, mel_kernel<true> + mel_clamp_windows_kernel behind
mt_mel_db_windows_f32, mel_clamp_kernel) stage by stage against the float64 pipeline of tests/frontend_f64_ref.py (checked on the CPU by
tests/test_frontend_f64_ref_cpu.py), at shapes of a few KB to a few MB.

The kernel is called with apply_clamp = 0, its dB taken back to power in float64 (P = 10^(dB/10)) and compared with mel_power64 fed the kernel's own
filterbank (mt_mel_filterbank_host).  Per frame
    e_frame = max_m |P - P_ref| / max_m P_ref            e_bin = max |P / P_ref - 1| over the bins with P_ref >= 1e-4 max_m P_ref
Frames whose reference maximum is below 1e-9 are left to the amin floor (where the reference is below half the floor the output must be -100 dB);
outside the silence cases they may be at most 5 % of a case's frames.  NO TOLERANCE IS HARD-CODED: for every input the plain float32 CPU pipeline
(scipy.fft.rfft on float32 frames, float32 filterbank product) is measured against the same reference (e32_frame, e32_bin) and the kernel gets
    e_frame <= 8 max(e32_frame, 1e-7)                    e_bin <= 8 max(e32_bin, 1e-6)
8 = room for the 32 x 32 factorisation with float32 twiddle tables against pocketfft, v_log_f32's ulp of log2 (3e-6 of the power near the floor) and
the four-way split of the ELL reduction.

Measured on an MI355X (python -m pytest tests/test_gpu_mel_f64.py -q -m gpu -s prints every line; the bounds are 8 x the right-hand pair, floored):
  case                                           e_frame  e_bin    | e32_frame e32_bin
  n_mels 320, hop 512, N 16384                   9.51e-07 2.44e-06 | 2.73e-07 2.95e-06
  n_mels 229, hop 512, N 16384                   1.20e-06 2.60e-06 | 2.51e-07 2.29e-06
  n_mels 64, hop 512, N 16384                    7.87e-07 1.21e-06 | 2.56e-07 9.99e-07
  n_mels 33, hop 512, N 16384                    6.66e-07 7.95e-07 | 3.75e-07 6.25e-07
  n_mels 6, hop 512, N 16384                     6.35e-07 6.35e-07 | 1.95e-07 5.40e-07
  hop 256, n_mels 64, N 16384                    9.88e-07 1.32e-06 | 3.26e-07 9.99e-07
  hop 160, n_mels 320, N 16384                   1.13e-06 3.47e-06 | 3.60e-07 6.89e-06
  hop 1024, n_mels 33, N 16384                   7.04e-07 9.65e-07 | 1.81e-07 5.48e-07
  hop 4096, n_mels 229, N 16384                  8.73e-07 2.03e-06 | 1.99e-07 2.37e-06
  N 1, hop 512, n_mels 64                        8.68e-07 8.71e-07 | 1.60e-07 1.60e-07
  N 2, hop 512, n_mels 64                        6.13e-07 8.31e-07 | 1.94e-07 2.43e-07
  N 511, hop 512, n_mels 64                      4.63e-07 7.04e-07 | 1.12e-07 5.17e-07
  N 512, hop 512, n_mels 64                      6.89e-07 1.02e-06 | 1.91e-07 3.47e-07
  N 513, hop 512, n_mels 64                      4.25e-07 6.36e-07 | 1.57e-07 4.01e-07
  N 1023, hop 512, n_mels 64                     6.90e-07 8.71e-07 | 1.36e-07 6.03e-07
  N 1024, hop 512, n_mels 64                     8.38e-07 8.38e-07 | 1.74e-07 8.58e-07
  N 1025, hop 512, n_mels 64                     6.01e-07 6.63e-07 | 1.64e-07 7.29e-07
  N 2047, hop 512, n_mels 64                     8.68e-07 9.85e-07 | 2.12e-07 5.92e-07
  N 2048, hop 512, n_mels 64                     9.32e-07 9.32e-07 | 1.91e-07 8.79e-07
  N 2049, hop 512, n_mels 64                     1.09e-06 1.10e-06 | 1.47e-07 6.77e-07
  N 16383, hop 512, n_mels 64                    9.30e-07 1.46e-06 | 2.65e-07 8.24e-07
  impulses, N 4096, n_mels 320                   1.54e-06 1.72e-06 | 3.01e-07 3.47e-07
  impulses, N 4097, n_mels 320                   1.54e-06 1.72e-06 | 2.82e-07 3.05e-07
  one tone per FFT bin, 1025 x 4096, n_mels 320  1.34e-06 7.33e-06 | 3.60e-07 7.16e-06
  chunk_max: chunk 1 scaled by 1e-3              1.46e-06 2.93e-06 | 3.18e-07 3.59e-06
The kernel sits at 3 .. 7 x the yardstick's e_frame (closest: N 2049 at 7.4 of 8) and at the yardstick's e_bin: about 1e-6 of a frame's strongest bin
is what a float32 dB value near +30 dB resolves (half an ulp of the product, one ulp of log2), before any FFT error.

Window mode (mt_mel_db_windows_f32) is compared bit for bit with mt_mel_db_f32 (clamped) on a zero-filled copy of each window, out of a 40 000 sample
store followed by one NaN, into a NaN-filled output.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_f64_ref as F  # noqa: E402
from oracle import frontend_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
SR, HOP = 16000, 512
N0 = 16384


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _mel(mta, n_mels, hop, wave, clamp=False):
    """(B, N) float32 numpy or device tensor -> (mel (B, n_mels, T) device tensor, chunk_max (B,) device tensor); sentinel-filled output.
    Straight through the C ABI (N = 0 included: the sample buffer then holds one unused float)"""
    from music_transcription_amd import _lib
    fe = mta.get_frontend(SR, n_mels, hop, "cuda")
    w = torch.from_numpy(wave).cuda() if isinstance(wave, np.ndarray) else wave
    assert w.dtype == torch.float32 and w.is_cuda
    B, N = w.shape
    buf = torch.zeros(max(B * N, 1), device="cuda")
    buf[:B * N] = w.reshape(-1)
    out = torch.full((B, n_mels, 1 + N // hop), float("nan"), device="cuda")
    cmax = torch.full((B,), float("nan"), device="cuda")
    _lib.check(_lib.lib.mt_mel_db_f32(_lib.ptr(fe.plan), fe.desc, _lib.ptr(buf), B, N, _lib.ptr(out), _lib.ptr(cmax), 1 if clamp else 0,
                                      _lib.stream_ptr()), "mt_mel_db_f32")
    torch.cuda.synchronize()
    return out, cmax


def _check(mta, tag, n_mels, hop, wave, P_ref=None, silence_case=False):
    """the comparison of the header; returns (mel dB numpy, chunk_max numpy, P_ref, bound on e_frame)"""
    fb = mta.mel_filterbank(SR, n_mels)
    if P_ref is None:
        P_ref = F.mel_power64(wave, hop, fb)
    b_frame, b_bin, e32f, e32b = F.mel_bounds(wave, hop, fb, P_ref)
    mel, cm = _mel(mta, n_mels, hop, wave)
    db = mel.cpu().numpy()
    assert db.shape == P_ref.shape and np.isfinite(db).all()
    e_frame, e_bin, live = F.mel_errors(F.db_to_power(db), P_ref)
    dead = 1.0 - live.mean()
    print(f"\n  {tag:44s} {e_frame:.2e} {e_bin:.2e} | {e32f:.2e} {e32b:.2e}   frames left to the floor {100 * dead:.1f} %")
    if not silence_case:
        assert dead <= 0.05, (tag, dead)
    silent = np.broadcast_to((P_ref.max(axis=-2) < 0.5 * F.AMIN)[..., None, :], db.shape)
    floor = db[silent]                                   # frames under the amin floor: -100 dB, and one value everywhere
    if floor.size:
        assert np.abs(floor - F.SILENCE_DB).max() <= F.SILENCE_TOL_DB and (floor == floor.flat[0]).all(), tag
    assert e_frame <= b_frame, (tag, e_frame, b_frame)
    assert e_bin <= b_bin, (tag, e_bin, b_bin)
    return db, cm.cpu().numpy(), P_ref, b_frame


def _three(N, seed):
    """B = 3, different content in every chunk: the synthetic piano mix, white noise, a pure tone"""
    t = np.arange(N)
    return np.stack([FR.synth_audio(1, N, seed=seed)[0], (0.1 * np.random.default_rng(seed).standard_normal(N)).astype(np.float32),
                     (0.5 * np.cos(2 * np.pi * 440.0 * t / SR + 0.3)).astype(np.float32)])


# ================================================================== shapes
@pytest.mark.parametrize("n_mels", [320, 229, 64, 33, 6])
def test_n_mels(mta, n_mels):
    """33 and 6: the last filter group is padded to 32 lanes (one live lane, six live lanes); T = 33: the second tile holds one live frame.
    6 is the smallest filterbank the kernel takes (604 ELL rows, 162 328 B of LDS): the padded ELL table lives in LDS at 128 B per row, so
    n_mels = 1 .. 3 (1024, 896, 808 rows > ELL_MAX_ROWS) and 4, 5 (more than 160 KB beside the FFT buffers) cannot run --
    test_entry_point_answers pins how they are refused."""
    _check(mta, f"n_mels {n_mels}, hop 512, N 16384", n_mels, HOP, _three(N0, n_mels))


@pytest.mark.parametrize("hop,n_mels", [(256, 64), (160, 320), (1024, 33), (4096, 229)])
def test_hops(mta, hop, n_mels):
    _check(mta, f"hop {hop}, n_mels {n_mels}, N 16384", n_mels, hop, _three(N0, hop))


@pytest.mark.parametrize("N", [1, 2, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 16383])
def test_lengths(mta, N):
    """odd lengths: the last sample's pair partner lies outside the chunk (odd_tail) -- in chunks 0 and 1 it is the next chunk's first sample"""
    _check(mta, f"N {N}, hop 512, n_mels 64", 64, HOP, FR.synth_audio(3, N, seed=100 + N))


# ================================================================== impulses
@pytest.mark.parametrize("N", [4096, 4097])
def test_impulses(mta, N):
    """a unit impulse has a flat spectrum: every frame that sees it at window offset o must be w[o]^2 sum_k fb[m, k] -- sample-to-frame alignment and
    the even / odd packing z = x[2n] + i x[2n+1], free of FFT cancellation; every other frame is -100 dB"""
    pos = [0, 1, 1023, 1024, 1025, 2600, 2601, N - 2, N - 1]
    wave = np.zeros((len(pos), N), np.float32)
    wave[np.arange(len(pos)), pos] = 1.0
    fb = mta.mel_filterbank(SR, 320)
    P_ref = np.stack([F.impulse_power64(N, p, HOP, fb) for p in pos])
    fmax = P_ref.max(axis=1)
    assert ((fmax >= F.LIVE_MIN) | (fmax < 0.5 * F.AMIN)).all()              # every frame is either compared or pinned to the floor
    assert (fmax >= F.LIVE_MIN).sum(axis=1).min() >= 1 and (fmax >= F.LIVE_MIN).sum() >= 2 * len(pos)
    _check(mta, f"impulses, N {N}, n_mels 320", 320, HOP, wave, P_ref=P_ref, silence_case=True)


# ================================================================== one tone per FFT bin; the persistent loop
def test_one_tone_per_fft_bin(mta):
    """1025 chunks of 4096 samples, chunk b = 0.5 cos(2 pi b n / 2048 + phi_b): every filter tap is hit by a tone at and next to its bin; neighbouring
    chunks carry different tones, so a read across a chunk boundary lands in another mel bin of an edge frame; 1025 tiles on 256 workgroups walk
    `ti += gridDim.x` and the cross-tile prefetch four times (and `ti >= n_tiles` of the prefetch in the last round)"""
    B, N = 1025, 4096
    b, n = np.arange(B)[:, None], np.arange(N)[None, :]
    phi = 0.3 + 2.0 * ((np.arange(B) * 0.6180339887498949) % 1.0)[:, None]
    wave = (0.5 * np.cos(2.0 * np.pi * ((b * n) % 2048) / 2048.0 + phi)).astype(np.float32)
    assert np.abs(wave[[0, 1024]]).min() > 0.1                               # DC and Nyquist: the phase sets the level
    _check(mta, "one tone per FFT bin, 1025 x 4096, n_mels 320", 320, HOP, wave)


def test_placement_independence(mta):
    """one chunk alone, then as chunk 0, 255, 256 and 299 of 300 chunks of noise (300 tiles on 256 workgroups): the same bits"""
    N = 512
    rng = np.random.default_rng(7)
    mine = FR.synth_audio(1, N, seed=8)
    alone, cm_alone = _mel(mta, 64, HOP, mine)
    for slot in (0, 255, 256, 299):
        batch = (0.3 * rng.standard_normal((300, N))).astype(np.float32)
        batch[slot] = mine[0]
        mel, cm = _mel(mta, 64, HOP, batch)
        assert torch.equal(mel[slot], alone[0]) and torch.equal(cm[slot], cm_alone[0]), slot
        assert not torch.equal(mel[(slot + 1) % 300], alone[0])


# ================================================================== chunk_max and the clamp
def test_chunk_max_and_clamp(mta):
    wave = _three(N0, 11)
    wave[1] *= 1e-3                                                          # per-CHUNK maxima
    db, cm, P_ref, b_frame = _check(mta, "chunk_max: chunk 1 scaled by 1e-3", 320, HOP, wave)
    want = P_ref.max(axis=(1, 2))
    assert (np.abs(cm.astype(np.float64) - want) <= b_frame * want).all(), (cm, want)
    assert np.abs(10.0 * np.log10(cm.astype(np.float64)) - db.max(axis=(1, 2))).max() <= 1e-5
    assert cm[1] < 1e-5 * cm[0]
    d_wave = torch.from_numpy(wave).cuda()
    raw, cm0 = _mel(mta, 320, HOP, d_wave, clamp=False)
    clamped, cm1 = _mel(mta, 320, HOP, d_wave, clamp=True)
    floor = 10.0 * torch.log10(torch.clamp(cm0, min=1e-10)) - 80.0          # float32, as mel_clamp_kernel computes it
    assert floor.dtype == torch.float32 and torch.equal(cm0, cm1)
    assert torch.equal(clamped, torch.maximum(raw, floor[:, None, None]))
    assert float((clamped == floor[:, None, None]).float().mean()) > 0.01    # the floor is active (the tone's far bins)


# ================================================================== window mode, bit for bit
N_STORE = 40000


def _windows(mta, n_mels, store, wins, T_out):
    """wins: (offset, win_len, rec_end, t_keep) -> (mel (B, n_mels, T_out), chunk_max (B,)) of mt_mel_db_windows_f32, NaN-filled before the call"""
    from music_transcription_amd import _lib
    fe = mta.get_frontend(SR, n_mels, HOP, "cuda")
    off, ln, re, tk = [list(c) for c in zip(*wins)]
    B = len(wins)
    d64 = torch.tensor(off, dtype=torch.int64, device="cuda")
    d32 = torch.tensor([ln, re, tk], dtype=torch.int32, device="cuda")
    mel = torch.full((B, 1, n_mels, T_out), float("nan"), device="cuda")
    cmax = torch.full((B,), float("nan"), device="cuda")
    _lib.check(_lib.lib.mt_mel_db_windows_f32(_lib.ptr(fe.plan), fe.desc, _lib.ptr(store), _lib.ptr(d64), _lib.ptr(d32[0]), _lib.ptr(d32[1]), B,
                                              max(ln), T_out, _lib.ptr(d32[2]), _lib.ptr(mel), _lib.ptr(cmax), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return mel[:, 0], cmax


def _copied(mta, n_mels, store, win, T_out):
    """mt_mel_db_f32 (clamped) on a zero-filled copy of the window, its first min(t_keep, frames) frames, zeros up to T_out"""
    off, n, rec_end, t_keep = win
    w = torch.zeros(1, n, device="cuda")
    k = max(0, min(rec_end, n))
    w[0, :k] = store[off:off + k]
    mel, cmax = _mel(mta, n_mels, HOP, w, clamp=True)
    out = torch.zeros(n_mels, T_out, device="cuda")
    tk = max(0, min(t_keep, mel.shape[-1]))
    out[:, :tk] = mel[0, :, :tk]
    return out, cmax


def _store():
    g = torch.Generator(device="cuda").manual_seed(5)
    backing = torch.full((N_STORE + 1,), float("nan"), device="cuda")        # the readable sample past the end is a NaN: it must not leak
    backing[:N_STORE] = torch.randn(N_STORE, device="cuda", generator=g) * 0.2
    return backing[:N_STORE]


@pytest.mark.parametrize("n_mels", [64, 320])
def test_windows_small(mta, n_mels):
    """win_len 0, 1, 511 (< hop), 512, 513, 2049, 8192; rec_end negative, 0, odd, even, = win_len, > win_len; t_keep 0, 1, the frame count, the
    frame count + 3; a window at store offset 0 and windows that end at the store's last sample; T_out = the longest window's 17 frames + 5"""
    S = N_STORE
    wins = [(0, 8192, 8192, 17), (100, 0, 0, 1), (101, 1, 1, 1), (7, 511, 511, 0), (1000, 512, 300, 2), (1001, 513, 513, 5), (2000, 2049, 2049, 5),
            (3000, 2049, -7, 5), (3001, 2049, 0, 8), (5000, 8192, 4097, 17), (5001, 8192, 9000, 20), (S - 8192, 8192, 8192, 17),
            (S - 2049, 2049, 2049, 5), (S - 513, 513, 600, 1), (20000, 1, 1, 0), (20001, 0, 5, 4), (S - 1, 1, 1, 1)]
    T_out = 1 + 8192 // HOP + 5
    store = _store()
    mel, cmax = _windows(mta, n_mels, store, wins, T_out)
    for b, win in enumerate(wins):
        want, wmax = _copied(mta, n_mels, store, win, T_out)
        assert torch.equal(mel[b], want), (b, win, (mel[b] - want).abs().max())
        assert torch.equal(cmax[b:b + 1], wmax), (b, win)
        tk = max(0, min(win[3], 1 + win[1] // HOP))
        assert float(mel[b, :, tk:].abs().max()) == 0.0                      # the tail is exactly 0.0: the clamp has not touched it


def test_windows_wrap_the_grid(mta):
    """300 windows of 512 samples: 300 tiles on 256 workgroups, mel_kernel<true>'s own walk and prefetch"""
    store = _store()
    wins = [(131 * i, 512, 512, 2) for i in range(299)] + [(N_STORE - 512, 512, 512, 2)]
    mel, cmax = _windows(mta, 64, store, wins, 2)
    copies = torch.stack([store[o:o + 512] for o, _, _, _ in wins])
    want, wmax = _mel(mta, 64, HOP, copies, clamp=True)
    assert torch.equal(mel, want) and torch.equal(cmax, wmax)


# ================================================================== what the entry point answers
def test_entry_point_answers(mta):
    """N = 0 is one frame of silence per chunk; B = 0 touches nothing; an odd hop, a null pointer and a filterbank of fewer than six filters are refused"""
    from music_transcription_amd import _lib
    fe = mta.get_frontend(SR, 64, HOP, "cuda")
    wave = torch.zeros(4, device="cuda")
    out = torch.full((2, 64, 1), float("nan"), device="cuda")
    cm = torch.full((2,), float("nan"), device="cuda")
    assert _lib.lib.mt_mel_db_f32(_lib.ptr(fe.plan), fe.desc, _lib.ptr(wave), 2, 0, _lib.ptr(out), _lib.ptr(cm), 0, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert float((out + 100.0).abs().max()) <= F.SILENCE_TOL_DB and bool((out == out.flatten()[0]).all()) and bool((cm == 0).all())
    out.fill_(float("nan"))
    cm.fill_(float("nan"))
    assert _lib.lib.mt_mel_db_f32(_lib.ptr(fe.plan), fe.desc, _lib.ptr(wave), 0, 4, _lib.ptr(out), _lib.ptr(cm), 1, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(cm).all())
    odd = mta.MelFrontend(SR, 64, 511, "cuda")
    assert _lib.lib.mt_mel_db_f32(_lib.ptr(odd.plan), odd.desc, _lib.ptr(wave), 1, 4, _lib.ptr(out), _lib.ptr(cm), 0, _lib.stream_ptr()) == -4   # MT_EUNSUPPORTED
    assert "hop must be even" in _lib.last_error()
    # filterbanks too wide for the LDS-resident ELL table are refused, not computed wrongly: n_mels = 1 .. 3 by the plan, 4 and 5 by the launch
    for nm in (1, 3):
        desc = _lib.MelDesc()
        plan = torch.empty(_lib.lib.mt_mel_plan_bytes(nm), dtype=torch.uint8, device="cuda")
        assert _lib.lib.mt_mel_plan_init(_lib.ptr(plan), plan.numel(), SR, HOP, nm, desc, _lib.stream_ptr()) == -4 and "too wide" in _lib.last_error()
    five = mta.MelFrontend(SR, 5, HOP, "cuda")
    assert _lib.lib.mt_mel_db_f32(_lib.ptr(five.plan), five.desc, _lib.ptr(wave), 1, 4, _lib.ptr(out), _lib.ptr(cm), 0, _lib.stream_ptr()) == -4
    assert "of LDS" in _lib.last_error()
    assert _lib.lib.mt_mel_db_f32(_lib.ptr(fe.plan), fe.desc, None, 1, 4, _lib.ptr(out), _lib.ptr(cm), 0, _lib.stream_ptr()) == -1             # MT_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
