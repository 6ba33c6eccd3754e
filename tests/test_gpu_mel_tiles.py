"""mel_kernel (csrc/mel_kernel.h) at the places a re-pipelined kernel can go wrong: the 32-frame tile and the sample prefetch that is handed from
one iteration / tile to the next, a grid smaller than the tile count, odd and very short chunks, every filter-group count, the window path, chunk_max
and state left over from an earlier launch.  Reference, error measures and bound are those of tests/test_gpu_mel_f64.py (its _check: the float64
pipeline of tests/frontend_f64_ref.py, the kernel allowed 8 x what the plain float32 CPU pipeline loses on the same input); nothing is re-derived or
copied here.  Shapes are the smallest that reach each path (a few KB to 0.5 MB of audio)."""
import numpy as np
import pytest
import torch

from test_gpu_mel_f64 import HOP, SR, _check, _mel, _store, _windows, mta  # noqa: F401  (mta is the module's build fixture)
from oracle import frontend_ref as FR

pytestmark = pytest.mark.gpu


def _chunks(B, N, seed):
    """B chunks of the synthetic piano mix, each with its own amplitude and DC offset: a frame that reads across a chunk border picks up a step of
    0.2 .. 0.5 and another level, far outside the bound"""
    w = FR.synth_audio(B, max(N, 1), seed=seed)[:, :N].astype(np.float32)
    amp = np.array([1.0, 0.05, 0.4, 0.7])[np.arange(B) % 4][:, None]
    dc = np.array([0.25, -0.3, 0.05, -0.15])[np.arange(B) % 4][:, None]
    return (w * amp + dc).astype(np.float32)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 16, 17, 32, 33, 34, 65])
def test_frames_against_the_tile(mta, T, B):
    """16 frames per iteration, 32 per tile: T = 16 | 17 ends on / one past the first iteration, 32 | 33 | 34 on / past the first tile, 65 leaves one
    live frame in a third tile; the prefetch of the next iteration / tile then fetches frames that do not exist"""
    N = HOP * (T - 1)
    _check(mta, f"T {T}, B {B}, n_mels 64", 64, HOP, _chunks(B, N, 10 * T + B), silence_case=N == 0)


def test_grid_smaller_than_the_tile_count(mta):
    """the launch has at most 256 workgroups: 520 one-tile chunks (> 2 x 256) make every workgroup walk two or three tiles of different chunks;
    N = 300 is also shorter than n_fft / 2, so every frame is mostly padding"""
    _check(mta, "520 chunks of 300 samples, n_mels 64", 64, HOP, _chunks(520, 300, 3))


@pytest.mark.parametrize("N", [1, 255, 777, 1023, HOP * 33 + 1])
def test_odd_and_short_chunks(mta, N):
    """odd n_samples: the last pair's second sample belongs to the next chunk (odd_tail); N < 1024: no frame is free of padding"""
    _check(mta, f"N {N}, B 3, n_mels 64", 64, HOP, _chunks(3, N, 40 + N % 97))


@pytest.mark.parametrize("hop", [256, 512])
@pytest.mark.parametrize("n_mels", [6, 32, 33, 64, 96, 320])
def test_filter_groups(mta, n_mels, hop):
    """1, 1, 2, 2, 3 and 10 filter groups, i.e. 151, 44, 82, 29, 24 and 22 blocks of the flat reduction: a lone group, a group of one live lane,
    single-block groups in a row (n_mels 320) and block counts of every remainder modulo the three register sets (24 = 0, 151 = 1, 44 = 2)"""
    _check(mta, f"n_mels {n_mels}, hop {hop}, N 8200", n_mels, hop, _chunks(3, 8200, n_mels + hop))


# (offset, win_len, rec_end, t_keep): rec_end < win_len (even, odd, 0), t_keep < frames, t_keep > frames, a window that ends with the store
WINS = [(0, 8192, 8192, 17), (11, 8192, 5001, 17), (12, 8192, 4096, 9), (4001, 16896, 16896, 34), (4002, 16896, 16001, 20), (777, 2049, 1025, 2),
        (778, 2049, 0, 5), (40000 - 16897, 16897, 16897, 40), (3, 513, 513, 1), (5, 300, 299, 1)]


@pytest.mark.parametrize("T_out", [10, 34, 39])
def test_windows(mta, T_out):
    """T_out below, at and above the longest window's 34 frames.  Every window bit for bit the clamped mt_mel_db_f32 of a zero-filled contiguous
    copy (cut or zero-padded to T_out), its chunk_max exactly the copy's although fewer frames are written than counted; the copy itself under the
    float64 bound (frames past rec_end are silence and are held to the -100 dB floor), and its clamped output the unclamped one lifted to a single floor"""
    store = _store()
    mel, cmax = _windows(mta, 64, store, WINS, T_out)
    for b, (off, n, rec_end, t_keep) in enumerate(WINS):
        k = max(0, min(rec_end, n))
        copy = torch.zeros(1, n, device="cuda")
        copy[0, :k] = store[off:off + k]
        _, cm_ref, _, _ = _check(mta, f"window {b}: len {n}, rec_end {rec_end}", 64, HOP, copy.cpu().numpy(), silence_case=k < n)
        raw, cm_raw = _mel(mta, 64, HOP, copy, clamp=False)
        clamped, cm = _mel(mta, 64, HOP, copy, clamp=True)
        lifted = clamped != raw                                              # the clamp only lifts values, to one floor per chunk
        assert torch.equal(cm, cm_raw) and bool((clamped[lifted] > raw[lifted]).all()) and clamped[lifted].unique().numel() <= 1
        assert np.array_equal(cm.cpu().numpy(), cm_ref)
        tk = min(t_keep, 1 + n // HOP, T_out)
        want = torch.zeros(64, T_out, device="cuda")
        want[:, :tk] = clamped[0, :, :tk]
        assert torch.equal(mel[b], want), (b, float((mel[b] - want).abs().max()))
        assert torch.equal(cmax[b:b + 1], cm), b


def test_chunk_max_is_the_kernels_own_maximum(mta):
    """chunk_max is the largest mel power the kernel itself computed over all 1 + N / hop frames: the dB output's maximum to within the rounding of
    the dB value, and the reference's maximum within the frame bound, per chunk"""
    wave = _chunks(3, HOP * 33 + 1, 9)
    db, cm, P_ref, b_frame = _check(mta, "chunk_max, T 34, B 3, n_mels 320", 320, HOP, wave)
    assert np.abs(10.0 * np.log10(cm.astype(np.float64)) - db.max(axis=(1, 2))).max() <= 1e-5
    want = P_ref.max(axis=(1, 2))
    assert (np.abs(cm.astype(np.float64) - want) <= b_frame * want).all()


def test_a_launch_leaves_nothing_behind(mta):
    """two calls into the same output and chunk_max buffers with different audio (the second quieter, so a surviving maximum would show): the
    second result is a fresh call's, bit for bit"""
    from music_transcription_amd import _lib
    fe = mta.get_frontend(SR, 320, HOP, "cuda")
    B, N = 3, HOP * 33 + 1
    first = torch.from_numpy(_chunks(B, N, 1)).cuda()
    second = torch.from_numpy(0.01 * _chunks(B, N, 2)).cuda()
    out = torch.full((B, 320, 1 + N // HOP), float("nan"), device="cuda")
    cm = torch.full((B,), float("nan"), device="cuda")
    for w in (first, second):
        _lib.check(_lib.lib.mt_mel_db_f32(_lib.ptr(fe.plan), fe.desc, _lib.ptr(w), B, N, _lib.ptr(out), _lib.ptr(cm), 0, _lib.stream_ptr()), "mel")
    torch.cuda.synchronize()
    fresh, cm_fresh = _mel(mta, 320, HOP, second)
    assert torch.equal(out, fresh) and torch.equal(cm, cm_fresh)
    assert float(cm.max()) < 0.01 * float(_mel(mta, 320, HOP, first)[1].min())
