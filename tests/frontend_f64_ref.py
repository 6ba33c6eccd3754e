"""Float64 references of the audio front end: the log-mel pipeline of csrc/mel_kernel.h / mel.hip / rawbatch.hip and the polyphase resampler of
csrc/resample.hip, with the error metrics and the bounds of tests/test_gpu_mel_f64.py and tests/test_gpu_resample_f64.py.  numpy (and scipy.fft for
the float32 yardstick) only; nothing of the package under test is imported.  tests/test_frontend_f64_ref_cpu.py checks all of it on the CPU
(against oracle.frontend_ref, torch.stft in float64 and scipy.signal.resample_poly).

  mel_power64   zero-pad by 1024 a side, periodic Hann, np.fft.rfft, |.|^2, times the float32 filterbank upcast -- float64 from the first product
                on, nothing is ever rounded to float32.
  mel_power32   the YARDSTICK, not a reference: the same pipeline in plain float32 on the CPU (scipy.fft.rfft keeps float32 frames in float32,
                float32 filterbank product).  Its distance from mel_power64 is what float32 costs on that input; the GPU tests allow the kernel
                8 x that (mel_bounds).
  resample64    y[j] = sum_i mono(x[i]) h[(j + n_pre_remove) down - i up], the sum of resample.hip's header, channel mean and PCM scaling in
                float64; resample64_polyphase is the same sum over a table hp[phase][k] = h[phase + k up].  Both also return sum |x h| per
                output, the scale of the derived rounding bound (resample_bound)."""
import numpy as np

N_FFT = 2048
N_BINS = N_FFT // 2 + 1
AMIN = float(np.float32(1e-10))          # the kernel's floor on the mel power (AMIN = 1e-10f)
LIVE_MIN = 1e-9                          # frames whose reference maximum is below this are governed by the floor, not by arithmetic
BIN_REL = 1e-4                           # e_bin looks at the bins within this factor of their frame's maximum
SILENCE_DB = -100.0
# -100 dB comes out as 3.0103f * log2(1e-10f): one ulp of log2 at 33.2 (3.8e-6) times 3.01 plus half an ulp of the product at 100 (3.8e-6)
SILENCE_TOL_DB = 2e-5


# ================================================================== mel
def hann64(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def num_frames(n_samples, hop):
    return 1 + n_samples // hop


def _frames(wave, hop, dtype):
    """(B, N) -> (B, T, 2048) zero-padded frames; frame t starts at sample t * hop - 1024"""
    wave = np.asarray(wave)
    assert wave.dtype == np.float32 and wave.ndim == 2
    B, N = wave.shape
    yp = np.zeros((B, N + N_FFT), dtype=dtype)
    yp[:, N_FFT // 2:N_FFT // 2 + N] = wave
    idx = hop * np.arange(num_frames(N, hop))[:, None] + np.arange(N_FFT)[None, :]
    return yp[:, idx]


def stft_power64(wave_f32, hop):
    """(B, N) float32 -> (B, T, 1025) float64"""
    spec = np.fft.rfft(_frames(wave_f32, hop, np.float64) * hann64(), axis=-1)
    assert spec.dtype == np.complex128
    return spec.real ** 2 + spec.imag ** 2


def mel_power64(wave_f32, hop, fb_f32):
    """(N,) or (B, N) float32 samples, (n_mels, 1025) float32 filterbank -> (n_mels, T) or (B, n_mels, T) float64 mel power, T = 1 + N // hop"""
    wave = np.asarray(wave_f32)
    one = wave.ndim == 1
    assert np.asarray(fb_f32).dtype == np.float32
    P = np.matmul(stft_power64(wave[None] if one else wave, hop), np.asarray(fb_f32).astype(np.float64).T).transpose(0, 2, 1)
    return P[0] if one else P


def mel_power32(wave_f32, hop, fb_f32):
    """the float32 CPU pipeline (yardstick): same shapes as mel_power64, float32 result"""
    import scipy.fft
    wave = np.asarray(wave_f32)
    one = wave.ndim == 1
    fr = _frames(wave[None] if one else wave, hop, np.float32) * hann64().astype(np.float32)
    assert fr.dtype == np.float32
    spec = scipy.fft.rfft(fr, axis=-1)
    assert spec.dtype == np.complex64
    S = spec.real * spec.real + spec.imag * spec.imag
    P = np.matmul(S, np.asarray(fb_f32).T).transpose(0, 2, 1)
    assert P.dtype == np.float32
    return P[0] if one else P


def db_to_power(db):
    return 10.0 ** (np.asarray(db, dtype=np.float64) / 10.0)


def mel_errors(P, P_ref):
    """P, P_ref (..., n_mels, T).  Both are floored at AMIN first, as the kernel floors what it takes the logarithm of.  Per frame
         e_frame = max_m |P - P_ref| / max_m P_ref          e_bin = max |P / P_ref - 1| over the bins with P_ref >= 1e-4 max_m P_ref
    over the LIVE frames (reference maximum >= 1e-9).  Returns (max e_frame, max e_bin, live mask (..., T)); (0, 0, mask) without a live frame."""
    P = np.maximum(np.asarray(P, dtype=np.float64), AMIN)
    R = np.asarray(P_ref, dtype=np.float64)
    fmax = R.max(axis=-2)
    live = fmax >= LIVE_MIN
    R = np.maximum(R, AMIN)
    if not live.any():
        return 0.0, 0.0, live
    safe = np.where(live, fmax, 1.0)
    e_frame = np.where(live, np.abs(P - R).max(axis=-2) / safe, 0.0)
    sel = (R >= BIN_REL * safe[..., None, :]) & live[..., None, :]
    e_bin = np.where(sel, np.abs(P / R - 1.0), 0.0).max(axis=-2)
    return float(e_frame.max()), float(e_bin.max()), live


FACTOR = 8.0                             # margin over the float32 yardstick: another FFT factorisation with float32 twiddle tables, v_log_f32's
FLOOR_FRAME, FLOOR_BIN = 1e-7, 1e-6      # ulp of log2 on the way through dB, the four-way split of the ELL reduction


def mel_bounds(wave_f32, hop, fb_f32, P_ref=None):
    """(bound on e_frame, bound on e_bin, e32_frame, e32_bin): 8 x what the float32 CPU pipeline loses on this very input"""
    if P_ref is None:
        P_ref = mel_power64(wave_f32, hop, fb_f32)
    e32f, e32b, _ = mel_errors(mel_power32(wave_f32, hop, fb_f32), P_ref)
    return FACTOR * max(e32f, FLOOR_FRAME), FACTOR * max(e32b, FLOOR_BIN), e32f, e32b


def impulse_power64(N, pos, hop, fb_f32):
    """mel power of a unit impulse at sample `pos` of an N-sample chunk, in closed form: the spectrum of a frame that sees the impulse at window
    offset o is flat, |X[k]|^2 = w[o]^2, so the mel power is w[o]^2 sum_k fb[m, k].  -> (n_mels, T) float64"""
    w = hann64()
    rows = np.asarray(fb_f32).astype(np.float64).sum(axis=1)
    o = pos + N_FFT // 2 - hop * np.arange(num_frames(N, hop))
    seen = (o >= 0) & (o < N_FFT)
    return rows[:, None] * np.where(seen, w[np.clip(o, 0, N_FFT - 1)] ** 2, 0.0)[None, :]


# ================================================================== resampler
FMT = {"int16": 0, "int32": 1, "float32": 2}
_PCM_SCALE = {0: 32768.0, 1: 2147483648.0, 2: 1.0}
_PCM_DTYPE = {0: np.int16, 1: np.int32, 2: np.float32}


def mono64(src, channels, fmt):
    """interleaved frames (n_in, channels) of the format's dtype -> float64 channel mean, integer PCM scaled to [-1, 1)"""
    src = np.asarray(src)
    assert src.dtype == _PCM_DTYPE[fmt] and src.shape[1:] == (channels,)
    return src.astype(np.float64).sum(axis=1) / channels / _PCM_SCALE[fmt]


def _tap_sum(x, tap, n_taps, up, down, n_pre_remove, n_out):
    """sum_k x[i_hi - k] tap(phase, k) for j = 0 .. n_out-1, where c = (j + n_pre_remove) down = i_hi up + phase; tap returns 0 past the filter"""
    c = (np.arange(n_out, dtype=np.int64) + n_pre_remove) * down
    i_hi, ph = c // up, c % up
    y, sabs = np.zeros(n_out), np.zeros(n_out)
    for k in range(n_taps):
        i = i_hi - k
        ok = (i >= 0) & (i < len(x))
        term = np.where(ok, x[np.clip(i, 0, len(x) - 1)], 0.0) * tap(ph, k)
        y += term
        sabs += np.abs(term)
    return y, sabs


def resample64(src, channels, fmt, h, up, down, n_pre_remove, n_out):
    """the direct sum over the taps h in natural order -> (y float64 (n_out,), sum_i |x[i] h[..]| (n_out,))"""
    h = np.asarray(h, dtype=np.float64)
    n_taps = (len(h) + up - 1) // up

    def tap(ph, k):
        t = ph + k * up
        return np.where(t < len(h), h[np.minimum(t, len(h) - 1)], 0.0)
    return _tap_sum(mono64(src, channels, fmt), tap, n_taps, up, down, n_pre_remove, n_out)


def resample64_polyphase(src, channels, fmt, hp, up, down, n_pre_remove, n_out):
    """the same sum over the polyphase table hp[phase][k] = h[phase + k up] ((up, L), zero-padded)"""
    hp = np.asarray(hp, dtype=np.float64)
    assert hp.shape[0] == up
    return _tap_sum(mono64(src, channels, fmt), lambda ph, k: hp[ph, k], hp.shape[1], up, down, n_pre_remove, n_out)


def resample64_loops(src, channels, fmt, h, up, down, n_pre_remove, n_out):
    """resample.hip's header formula as two plain loops (slow; the CPU test holds the vectorised sums to it)"""
    x = mono64(src, channels, fmt)
    y = np.zeros(n_out)
    for j in range(n_out):
        c = (j + n_pre_remove) * down
        for i in range(len(x)):
            t = c - i * up
            if 0 <= t < len(h):
                y[j] += x[i] * float(h[t])
    return y


def polyphase_table(h, up):
    """h[phase + k up] -> table[phase][k], zero-padded, float32"""
    L = (len(h) + up - 1) // up
    t = np.zeros(L * up, dtype=np.float32)
    t[:len(h)] = h
    return np.ascontiguousarray(t.reshape(L, up).T)


def resample_bound(sabs, taps_per_phase, channels):
    """|got - ref| <= (L + channels + 2) 2^-24 sum |x h| per output: L sequential float32 fma steps (each rounds a partial sum that never
    exceeds sum |x h|), `channels` roundings in the int -> float conversions and the channel sum, 2 for the scaling and the division."""
    return (taps_per_phase + channels + 2) * 2.0 ** -24 * np.asarray(sabs)


def resample_tile_plan(L, up, down):
    """mirror of resample_tile_plan (csrc/resample.hip): (P phases per workgroup, W floats of LDS window; W = 0: the tiled kernel does not fit)"""
    P = min(up, 16)
    while 1024 % P:
        P -= 1
    MW = 1024 // P
    w = (MW - 1) * down + ((P - 1) * down) // up + 2 + L
    return P, (w if 1024 <= w <= 38 * 1024 else 0)


def resample_kernel(L, up, down, n_out, tiled_enabled=True):
    """which kernel mt_resample_polyphase launches: 'tiled' or 'thread' (the thread-per-output resample_polyphase_kernel)"""
    P, W = resample_tile_plan(L, up, down)
    return "tiled" if (W and tiled_enabled and n_out >= 4096) else "thread"
