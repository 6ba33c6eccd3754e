"""GEMM conformance: every `mt_gemm_*` entry point of csrc/gemm.hip against an exact CPU reference.

fp32 accumulation of integer-valued operands is independent of the summation order and exact while every partial sum stays
below 2^24, so the operands here are small integers (exact in bf16 and f16), the bias is integer-valued, the reference is a
plain CPU matrix product and the comparison is `torch.equal` on every element.  The storage layouts (gx, logits, dh, the hx
image that the AHX loader reads) are restated here in numpy from include/mt_hip.h and the head of gemm.hip; no re-layout kernel
of the library takes part in a reference.  Every output lies between two guard bands in a buffer pre-filled with a sentinel,
and everything that is not a logical element (guard bands, padded batch slots, padded units, columns n >= N up to ldc, the
second half of a gx buffer that holds an f16 image) must still hold the sentinel afterwards.  Operands are sized exactly to the
documented readable extent (rows up to roundup(M or N, 128) - 1) between NaN guard bands, and their pad rows hold NaN / +-Inf.

Each case names the kernel it is meant to reach (`tile`: 128 = gemm_kernel, 256 = gemm256x_kernel); `_tile()` restates the
dispatch conditions of launch_dt / launch_hx and every case asserts its expectation against it, so a changed threshold shows
up here.  gemm256p_kernel (MT_GEMM_PERSIST=1) and the MT_GEMM_TILE=128 fall-back are read from the environment once per
process: those cases run in one fresh child process each (this file run as a script).

Run only this file:  python -m pytest tests/test_gpu_gemm.py -q -m gpu
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, GX_F16 = 0, 1, 0x10             # MT_DT_BF16, MT_DT_F16, MT_GX_F16 (include/mt_hip.h)
EINVAL = -1                                # MT_EINVAL
N_PITCH = 88
GUARD = 4096                               # elements of guard band on either side of every buffer
SENT32 = 0x7FC0BEEF                        # a NaN no kernel produces
SENT16 = 0x7BCD                            # 16-bit outputs: a finite pattern far outside every expected value
NAN, INF = float("nan"), float("inf")


def _api():
    from music_transcription_amd._lib import lib, last_error, stream_ptr
    return lib, last_error, stream_ptr()


def _ok(rc):
    if rc != 0:
        from music_transcription_amd._lib import last_error
        raise AssertionError(f"call failed (code {rc}): {last_error()}")


def _ru(x, m):
    return (x + m - 1) // m * m


def _cdiv(a, b):
    return (a + b - 1) // b


def _tdt(dt):
    return torch.float16 if dt == F16 else torch.bfloat16


def _tile(M, N, batch=1):
    """launch_dt's choice, restated: the 256 x 256 kernel for M >= 1024, N >= 512, 128 | N and >= 128 tiles in the launch."""
    if os.environ.get("MT_GEMM_TILE", "").strip() == "128":
        return 128
    return 256 if (M >= 1024 and N >= 512 and N % 128 == 0 and _cdiv(M, 256) * _cdiv(N, 256) * batch >= 128) else 128


def _persist_ok(B, H, N, K, M, gx16, sched):
    """persist_ok, restated (the buffer-size terms do not bind at these shapes)."""
    return (os.environ.get("MT_GEMM_PERSIST", "").strip() == "1" and sched and bool(gx16) and B % 32 == 0 and H % 256 == 0 and N % 256 == 0
            and K % 256 == 0 and K // 64 >= 16 and M >= 4096)


# ------------------------------------------------------------------ buffers
def _poison(n):
    v = torch.empty(n)
    v[0::3], v[1::3], v[2::3] = NAN, INF, -INF
    return v


def _dev16(body, dt):
    """A 16-bit operand on the device: `body` (f32 values on the CPU) between two NaN guard bands -> (owner, address of the body)"""
    g = torch.full((GUARD,), NAN)
    full = torch.cat([g, body, g]).to(_tdt(dt)).cuda()
    return full, full.data_ptr() + 2 * GUARD


def _dev32(body):
    g = torch.full((GUARD,), NAN)
    full = torch.cat([g, body.float(), g]).cuda()
    return full, full.data_ptr() + 4 * GUARD


def _place(logical, rows_p, ld, s1=0, s2=0, zdiv=1):
    """Storage of a batch of row-major matrices logical[z][R][K]: item z at element offset (z / zdiv) s1 + (z % zdiv) s2, row pitch ld,
    sized exactly to the contract -- readable up to row rows_p - 1 of every item, nothing behind it -- and NaN / +-Inf wherever no
    logical element lies (pad rows, columns K .. ld - 1, gaps between items)."""
    Z, R, K = logical.shape
    offs = [(z // zdiv) * s1 + (z % zdiv) * s2 for z in range(Z)]
    body = _poison(max(offs) + (rows_p - 1) * ld + K)
    for z in range(Z):
        body.as_strided((R, K), (ld, 1), offs[z]).copy_(logical[z])
    return body


class _Out:
    """An output buffer of n elements (f32, or 16-bit) between two guard bands, all of it pre-filled with a sentinel."""

    def __init__(self, n, bits16):
        self.n, self.bits16 = n, bits16
        self.sent = SENT16 if bits16 else SENT32
        self.buf = torch.full((GUARD + n + GUARD,), self.sent, dtype=torch.int16 if bits16 else torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * (2 if bits16 else 4)

    def untouched(self):
        return bool((self.buf == self.sent).all().item())

    def check(self, idx, ref, out_dtype, what=""):
        """Every logical element (body position idx[...]) equals ref[...]; every other element of the buffer is the sentinel."""
        full = self.buf.cpu()
        pos = torch.from_numpy(np.ascontiguousarray(idx).reshape(-1)) + GUARD
        assert int(pos.min()) >= GUARD and int(pos.max()) < GUARD + self.n, "reference index outside the buffer"
        other = torch.ones(full.numel(), dtype=torch.bool)
        other[pos] = False
        assert int((~other).sum()) == pos.numel(), "reference layout maps two logical elements to one slot"
        got = full[pos].view(out_dtype)
        exp = ref.reshape(-1).to(out_dtype)
        if not torch.equal(got, exp):
            bad = torch.nonzero(~(got == exp)).reshape(-1)
            i = int(bad[0])
            N = idx.shape[-1]
            raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; first at logical (row {i // N}, col {i % N}): "
                                 f"got {float(got[i])}, want {float(exp[i])}")
        stray = int((full[other] != self.sent).sum())
        assert stray == 0, f"{what}: {stray} elements outside the logical output were written"


# ------------------------------------------------------------------ references
@functools.lru_cache(maxsize=3)
def _problem(Z, M, N, K, amp, seed, w_keep=1.0, bias_amp=3):
    """Integer operands A[Z][M][K], W[Z][N][K] in [-amp, amp] (W thinned to a share w_keep of non-zeros), bias[N] in [-bias_amp, bias_amp],
    and the exact product ref[Z][M][N] = A W^T + bias as float64."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-amp, amp + 1, (Z, M, K), generator=g).float()
    W = torch.randint(-amp, amp + 1, (Z, N, K), generator=g).float()
    if w_keep < 1.0:
        W = W * (torch.rand(Z, N, K, generator=g) < w_keep)
        assert bool((W.reshape(Z * N, K // 64, 64) != 0).any(-1).sum(0).min() > 0), "a K-tile contributes nothing"
    bias = torch.randint(-bias_amp, bias_amp + 1, (N,), generator=g).float()
    assert K * amp * amp + bias_amp < 2 ** 24                  # every partial sum, in any order, is an exact f32 (and f64) integer
    if Z * M * N * K <= 4e9:
        ref = torch.matmul(A.double(), W.double().transpose(1, 2))
    else:                                                       # integer data: the f32 product is exact too (bound above)
        assert torch.get_float32_matmul_precision() == "highest"
        ref = torch.matmul(A, W.transpose(1, 2)).double()
    return A, W, bias, ref + bias.double()


def _representable(ref, out_dtype):
    assert torch.equal(ref, ref.to(out_dtype).double()), "the reference itself is not exact in the output type"


def _dropout_keep(seed, layer, idx, p):
    """dropout_keep of csrc/mt_common.h in uint64 arithmetic (idx: element index m * 2Hv + n)."""
    G, MASK = 0x9E3779B97F4A7C15, (1 << 64) - 1
    c = (((((seed << 8) ^ layer) & MASK) * G) + G) & MASK
    z = idx.astype(np.uint64) + np.uint64(c)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0) >= np.float32(p)


# ------------------------------------------------------------------ layouts (include/mt_hip.h, head of csrc/gemm.hip)
def _mn(M, N):
    return np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]


def _gx_index(B, T, H):
    """m = t B + b, n = d 4H + p H + j -> gx[b/32][t][d][j/8][p][j%8][b%32]"""
    m, n = _mn(T * B, 8 * H)
    t, b = m // B, m % B
    d, r = n // (4 * H), n % (4 * H)
    p, j = r // H, r % H
    return ((((((b // 32) * T + t) * 2 + d) * (H // 8) + j // 8) * 4 + p) * 8 + j % 8) * 32 + b % 32


def _logits_index(B, T, N):
    """m = t B + b -> out[b][n][t]; with several heads (N = heads * 88) one such block per head: out[n/88][b][n%88][t]"""
    m, n = _mn(T * B, N)
    t, b = m // B, m % B
    return (((n // N_PITCH) * B + b) * N_PITCH + n % N_PITCH) * T + t


def _dh_index(B, T, H, Hv):
    """m = t B + b, n = d Hv + j -> dh[b/32][t][d][j/8][j%8][b%32], H the padded width"""
    m, n = _mn(T * B, 2 * Hv)
    t, b = m // B, m % B
    d, j = n // Hv, n % Hv
    return (((((b // 32) * T + t) * 2 + d) * (H // 8) + j // 8) * 8 + j % 8) * 32 + b % 32


def _hx_index(B, T, Hp):
    """m = t B + b, k = dir Hp + u -> hx[b/32][t][dir][u/16][((u/8)%2) 32 + b%32][u%8] (f16)"""
    m, k = _mn(T * B, 2 * Hp)
    t, b = m // B, m % B
    d, u = k // Hp, k % Hp
    return (((((b // 32) * T + t) * 2 + d) * (Hp // 16) + u // 16) * 64 + ((u // 8) % 2) * 32 + b % 32) * 8 + u % 8


def _hx_image(logical, B, T, Hp):
    """The f16 hx image of a logical [T B][2 Hp] matrix; padded batch slots hold NaN."""
    lib = _api()[0]
    n = lib.mt_lstm_hx_bytes(B, T, Hp) // 2
    body = torch.full((n,), NAN)
    body[torch.from_numpy(_hx_index(B, T, Hp).reshape(-1))] = logical.reshape(-1)
    return body


def test_hx_image_map_matches_lstm_unpack():
    """The numpy description of the hx image, pinned against mt_lstm_unpack_f32 (tested on its own against the recurrence):
    image -> y[b][t][dir H + j] must give back the logical matrix."""
    lib, _, s = _api()
    for B, T, H in ((5, 7, 64), (33, 3, 48), (64, 2, 256)):
        g = torch.Generator().manual_seed(B + T + H)
        logical = torch.randn(T * B, 2 * H, generator=g).half().float()
        own, p = _dev16(_hx_image(logical, B, T, H), F16)
        y = torch.full((B, T, 2 * H), NAN, device="cuda")
        _ok(lib.mt_lstm_unpack_f32(p, y.data_ptr(), B, T, H, s))
        assert torch.equal(y.cpu(), logical.reshape(T, B, 2 * H).transpose(0, 1))


# ------------------------------------------------------------------ row-major outputs (EPI_ROWMAJOR, EPI_ROWMAJOR_BF16), plain and batched
def _run_rowmajor(M, N, K, dt, tile, lda=0, ldw=0, ldc=0, bias=True, out16=False, relu=0, batch=1, zdiv=1, api="dt", w_keep=1.0, seed=1):
    """zdiv == 1: items at block strides with gaps; zdiv > 1: the attention call sites' form (train_step_large.py) -- the z2 items
    (heads) interleaved inside the rows (s?2 = item width, ld = zdiv widths + pad), z1 (batch) a block stride."""
    lib, _, s = _api()
    assert _tile(M, N, batch) == tile, f"dispatch moved: ({M}, {N}, batch {batch}) was meant for the {tile} tile"
    Mp, Np = _ru(M, 128), _ru(N, 128)
    A, W, b, ref = _problem(batch, M, N, K, 1 if out16 else 3, seed + M + N + K, w_keep)
    if not bias:
        ref = ref - b.double()
    if relu:
        ref = ref.clamp(min=0)
    out_dtype = _tdt(dt) if out16 else torch.float32
    _representable(ref, out_dtype)
    if zdiv > 1:
        lda, ldw, ldc = zdiv * K + 8, zdiv * K + 16, zdiv * N + 4
        sA, sW, sC = (Mp * lda + 64, K), (Np * ldw + 128, K), (M * ldc + 12, N)
    else:
        lda, ldw, ldc = lda or K, ldw or K, ldc or N
        one = batch == 1
        sA = (0 if one else _ru((Mp - 1) * lda + K, 8) + 64, 0)
        sW = (0 if one else _ru((Np - 1) * ldw + K, 8) + 128, 0)
        sC = (0 if one else _ru((M - 1) * ldc + N, 2) + 10, 0)
    ownA, pA = _dev16(_place(A, Mp, lda, sA[0], sA[1], zdiv), dt)
    ownW, pW = _dev16(_place(W, Np, ldw, sW[0], sW[1], zdiv), dt)
    ownB, pB = _dev32(b)
    pB = pB if bias else None
    offs = np.array([(z // zdiv) * sC[0] + (z % zdiv) * sC[1] for z in range(batch)], dtype=np.int64)
    m, n = _mn(M, N)
    idx = offs[:, None, None] + (m * ldc + n)[None]
    out = _Out(int(offs.max()) + (M - 1) * ldc + N, out16)
    if api == "plain":
        assert dt == BF16 and batch == 1 and not out16
        _ok(lib.mt_gemm_bf16_f32acc(pA, lda, pW, ldw, pB, out.ptr, ldc, M, N, K, s))
    elif api == "dt":
        assert batch == 1 and not out16
        _ok(lib.mt_gemm_f32acc_dt(pA, lda, pW, ldw, pB, out.ptr, ldc, M, N, K, dt, s))
    elif api == "batched" and not out16:
        if dt == BF16:
            _ok(lib.mt_gemm_batched_f32(pA, lda, sA[0], sA[1], pW, ldw, sW[0], sW[1], pB, out.ptr, ldc, sC[0], sC[1], M, N, K, batch, zdiv, s))
        else:
            _ok(lib.mt_gemm_batched_f32_dt(pA, lda, sA[0], sA[1], pW, ldw, sW[0], sW[1], pB, out.ptr, ldc, sC[0], sC[1], M, N, K, batch, zdiv, dt, s))
    elif api == "batched_plain16":
        assert dt == BF16 and out16
        _ok(lib.mt_gemm_batched_bf16out(pA, lda, sA[0], sA[1], pW, ldw, sW[0], sW[1], pB, out.ptr, ldc, sC[0], sC[1], M, N, K, batch, zdiv, relu, s))
    else:
        assert api == "batched" and out16
        _ok(lib.mt_gemm_batched_h16out_dt(pA, lda, sA[0], sA[1], pW, ldw, sW[0], sW[1], pB, out.ptr, ldc, sC[0], sC[1], M, N, K, batch, zdiv, relu, dt, s))
    out.check(idx, ref, out_dtype, f"rowmajor M={M} N={N} K={K} dt={dt} batch={batch}")


# (M, N, K, dt, tile, keyword arguments)
ROWMAJOR = [
    (128, 128, 64, BF16, 128, dict(api="plain")),                       # one tile, one K-tile: prologue = epilogue
    (128, 128, 64, F16, 128, {}),
    (300, 200, 192, BF16, 128, dict(lda=200, ldw=208, ldc=203)),         # lda, ldw > K, ldc > N (odd: unaligned rows), three K-tiles
    (1000, 88, 1024, F16, 128, dict(bias=False)),
    (2500, 1152, 128, BF16, 128, {}),                                    # 20 x 9 = 180 tiles: the 128 kernel's XCD tile order with a remainder
    # M on both sides of 1024 (N = 8192: 4 or 5 tile rows x 32 columns)
    (1023, 8192, 64, BF16, 128, {}),
    (1024, 8192, 64, BF16, 256, {}),
    (1025, 8192, 128, F16, 256, {}),
    # tile count on both sides of 128.  (127 itself cannot occur: it is prime and N >= 512 makes at least two tile columns.)
    (16128, 512, 64, BF16, 128, {}),                                     # 63 x 2 = 126
    (16384, 512, 64, BF16, 256, {}),                                     # 64 x 2 = 128
    (10752, 640, 64, F16, 128, {}),                                      # 42 x 3 = 126
    (11008, 640, 64, F16, 256, {}),                                      # 43 x 3 = 129
    # N = 512 / 640 / 576 at one M: 576 is no multiple of 128 and stays on the small tile
    (16641, 512, 64, F16, 256, {}),
    (16641, 640, 128, BF16, 256, dict(ldc=644)),
    (16641, 576, 64, BF16, 128, {}),
    # edge tiles of the 256 kernel: M = 256 k + 1 / + 129 / + 255, N = 640 / 1152 (clamped rows), odd K-tile count
    (16385, 640, 192, BF16, 256, dict(lda=200, ldw=256, ldc=641)),
    (8321, 1152, 128, F16, 256, {}),
    (6911, 1152, 64, BF16, 256, dict(bias=False)),
    (4096, 2048, 1024, F16, 256, {}),                                    # 16 K-tiles
]


def _ids(cases):
    return ["-".join(str(x) for x in c[:-1]) + ("-" + "-".join(f"{k}{v}" for k, v in c[-1].items()) if c[-1] else "") for c in cases]


@pytest.mark.parametrize("M,N,K,dt,tile,kw", ROWMAJOR, ids=_ids(ROWMAJOR))
def test_rowmajor_f32_exact(M, N, K, dt, tile, kw):
    _run_rowmajor(M, N, K, dt, tile, **kw)


def test_rowmajor_overlapping_rows():
    """lda < K: rows overlap (the 1 x 1 convolution over 32 channels-last channels runs as K = 64 over 32-element rows with zero
    weight columns for the second half).  What a zero weight multiplies must be finite, so row M (the first pad row, which row M - 1
    overlaps) is finite here; the pad rows behind it are NaN / Inf and the buffer ends with the last pad row's K elements."""
    lib, _, s = _api()
    for M, N, dt, tile in ((1000, 200, BF16, 128), (16385, 512, F16, 256)):
        assert _tile(M, N) == tile
        K, lda, Mp, Np = 64, 32, _ru(M, 128), _ru(N, 128)
        g = torch.Generator().manual_seed(M)
        flat = torch.randint(-3, 4, ((M + 1) * lda,), generator=g).float()
        body = _poison((Mp - 1) * lda + K)
        body[:flat.numel()] = flat
        W = torch.randint(-3, 4, (1, N, K), generator=g).float()
        W[..., 32:] = 0
        bias = torch.randint(-3, 4, (N,), generator=g).float()
        ref = flat[:M * lda].reshape(M, lda).double() @ W[0, :, :32].double().t() + bias.double()
        ownA, pA = _dev16(body, dt)
        ownW, pW = _dev16(_place(W, Np, K), dt)
        ownB, pB = _dev32(bias)
        out = _Out(M * N, False)
        _ok(lib.mt_gemm_f32acc_dt(pA, lda, pW, K, pB, out.ptr, N, M, N, K, dt, s))
        m, n = _mn(M, N)
        out.check(m * N + n, ref, torch.float32, f"overlapping rows M={M}")


BATCHED = [
    # attention-like: heads interleaved in the rows (zdiv = heads), batch a block stride; bias NULL as at the call sites
    (200, 200, 64, BF16, 128, dict(batch=6, zdiv=3, bias=False)),
    (200, 96, 128, F16, 128, dict(batch=4, zdiv=2)),
    (130, 70, 64, BF16, 128, dict(batch=5)),                             # zdiv = 1, gaps between the items
    (1024, 512, 64, BF16, 256, dict(batch=16, zdiv=4, bias=False)),      # 4 x 2 tiles x 16 = 128: the 256 kernel through the batch term
    (1024, 512, 64, F16, 128, dict(batch=15)),                           # 120 tiles
    (1100, 640, 128, F16, 256, dict(batch=9)),                           # 5 x 3 x 9 = 135, edge tiles in both directions
]


@pytest.mark.parametrize("M,N,K,dt,tile,kw", BATCHED, ids=_ids(BATCHED))
def test_batched_f32_exact(M, N, K, dt, tile, kw):
    _run_rowmajor(M, N, K, dt, tile, api="batched", **kw)


H16OUT = [
    (300, 200, 192, BF16, 128, dict(api="batched_plain16", relu=1, ldc=202)),
    (300, 200, 192, F16, 128, dict(relu=0)),
    (200, 96, 128, BF16, 128, dict(batch=4, zdiv=2, relu=1)),
    (130, 70, 64, F16, 128, dict(batch=3, relu=1, bias=False)),
    (16385, 640, 128, BF16, 256, dict(api="batched_plain16", relu=0)),
    (16385, 640, 192, F16, 256, dict(relu=1, ldc=642)),                  # ldc = 642: rows not 8-byte aligned, the element-wise stores
    (8321, 1152, 1024, BF16, 256, dict(relu=1, w_keep=0.2)),
    (1024, 512, 64, F16, 256, dict(batch=16, zdiv=4, relu=1)),
]


@pytest.mark.parametrize("M,N,K,dt,tile,kw", H16OUT, ids=_ids(H16OUT))
def test_batched_h16out_exact(M, N, K, dt, tile, kw):
    kw = dict(kw)
    kw.setdefault("api", "batched")
    _run_rowmajor(M, N, K, dt, tile, out16=True, **kw)


def test_split_k_equals_the_unsplit_product():
    """train_step._gemm's split K: K slices as a batch (sA2 = sW2 = Kc) into partial products, summed by mt_sum_slices_f32 -- exact on
    integer data, so equal to the unsplit product whatever the order.  _split_k's choice for dW_hh at H = 512 (4H x H = 2048 x 512
    outputs: 16 tiles of 256; 236 K-tiles are divisible by 4, not by 8; 16 * 4 workgroups stay under two per CU) is 4."""
    from music_transcription_amd.train_step import _split_k
    lib, _, s = _api()
    assert _split_k(2048, 512, 236 * 64) == 4
    M, N, K = 2048, 512, 4096
    S = _split_k(M, N, K)
    assert S == 8 and _tile(M, N, S) == 256
    Kc = K // S
    A, W, _, ref = _problem(1, M, N, K, 3, 77)
    ownA, pA = _dev16(_place(A, M, K), BF16)
    ownW, pW = _dev16(_place(W, N, K), BF16)
    part = _Out(S * M * N, False)
    out = _Out(M * N, False)
    _ok(lib.mt_gemm_batched_f32(pA, K, 0, Kc, pW, K, 0, Kc, None, part.ptr, N, 0, M * N, M, N, Kc, S, S, s))
    _ok(lib.mt_sum_slices_f32(part.ptr, M * N, N, S, out.ptr, N, M, N, s))
    m, n = _mn(M, N)
    refp = torch.stack([A[0, :, i * Kc:(i + 1) * Kc].double() @ W[0, :, i * Kc:(i + 1) * Kc].double().t() for i in range(S)])
    part.check(np.arange(S, dtype=np.int64)[:, None, None] * (M * N) + (m * N + n)[None], refp, torch.float32, "split-K partial products")
    out.check(m * N + n, ref - _problem(1, M, N, K, 3, 77)[2].double(), torch.float32, "split-K sum")


# ------------------------------------------------------------------ gate pre-activations (EPI_LSTM_GX), f32 and f16 image
def _run_gx(B, T, H, K, dt, gx16, tile, api="dt", ldx=0, ldw=0, sched=False, w_keep=1.0, hprev=0, kernel=None):
    """hprev > 0: A comes from an hx image (AHX loader, f16 operands, K = 2 hprev).  sched: a fresh 64-byte block of non-zero bytes."""
    lib, _, s = _api()
    M, N = T * B, 8 * H
    if hprev:
        K, dt = 2 * hprev, F16
    if sched and _persist_ok(B, H, N, K, M, gx16, True):
        assert kernel == "persist", "this shape takes the persistent kernel"
    else:
        assert kernel != "persist", "this shape was meant for the persistent kernel"
        want = 256 if (hprev and M >= 1024 and N >= 512 and N % 128 == 0 and _cdiv(M, 256) * _cdiv(N, 256) >= 128) else (128 if hprev else _tile(M, N))
        assert want == tile, f"dispatch moved: gx B={B} T={T} H={H} was meant for the {tile} tile"
    A, W, b, ref = _problem(1, M, N, K, 1 if gx16 else 3, 7 + B + T + H + K, w_keep)
    if gx16:            # sum |a| |w| + |bias| <= 2048: every partial result is an integer that f16 holds
        assert float(W.abs().sum(-1).max()) + 3 <= 2048
    out_dtype = torch.float16 if gx16 else torch.float32
    _representable(ref, out_dtype)
    Mp, Np = _ru(M, 128), _ru(N, 128)
    ldx, ldw = ldx or K, ldw or K
    if hprev:
        ownA, pA = _dev16(_hx_image(A[0], B, T, hprev), F16)
    else:
        ownA, pA = _dev16(_place(A, Mp, ldx), dt)
    ownW, pW = _dev16(_place(W, Np, ldw), dt)
    ownB, pB = _dev32(b)
    n_f32 = lib.mt_lstm_gx_bytes(B, T, H) // 4
    assert n_f32 == _cdiv(B, 32) * T * 2 * (H // 8) * 1024
    out = _Out(2 * n_f32 if gx16 else n_f32, gx16)          # an f16 image fills the first half of the buffer
    sch = _Out(16, False) if sched else None
    if sch is not None:
        assert lib.mt_gemm_sched_bytes() == 64
    flag = dt | (GX_F16 if gx16 else 0)
    if hprev:
        if api == "sched":
            _ok(lib.mt_gemm_lstm_gx_from_hx_sched(pA, pW, ldw, pB, out.ptr, B, T, H, hprev, int(gx16), sch.ptr if sch else None, s))
        elif api == "plain":
            assert not gx16
            _ok(lib.mt_gemm_lstm_gx_from_hx(pA, pW, ldw, pB, out.ptr, B, T, H, hprev, s))
        else:
            _ok(lib.mt_gemm_lstm_gx_from_hx_ex(pA, pW, ldw, pB, out.ptr, B, T, H, hprev, int(gx16), s))
    elif api == "sched":
        _ok(lib.mt_gemm_lstm_gx_sched(pA, ldx, pW, ldw, pB, out.ptr, B, T, H, K, flag, sch.ptr if sch else None, s))
    elif api == "plain":
        assert dt == BF16 and not gx16
        _ok(lib.mt_gemm_lstm_gx(pA, ldx, pW, ldw, pB, out.ptr, B, T, H, K, s))
    else:
        _ok(lib.mt_gemm_lstm_gx_dt(pA, ldx, pW, ldw, pB, out.ptr, B, T, H, K, flag, s))
    out.check(_gx_index(B, T, H), ref, out_dtype, f"gx B={B} T={T} H={H} K={K} dt={dt} f16={gx16} hprev={hprev}")
    if sch is not None:
        full = sch.buf.cpu()
        assert bool((full[:GUARD] == SENT32).all()) and bool((full[GUARD + 16:] == SENT32).all()), "the scheduler block's neighbours were written"
        if kernel == "persist":         # 8 queue heads, zeroed by the call, then counted up by the pulls; the other 8 words zero
            body = full[GUARD:GUARD + 16]
            assert bool((body[8:] == 0).all()) and int(body[:8].sum()) >= _cdiv(M, 256) * (N // 256)


# (B, T, H, K, dt, f16 image, tile, keyword arguments)
GX = [
    # 128 tile.  Its epilogue: a 32-row block of one (direction, gate) when H % 32 == 0, else element by element
    (1, 50, 16, 64, BF16, 0, 128, dict(api="plain")),
    (5, 33, 48, 128, F16, 0, 128, {}),
    (5, 33, 48, 128, F16, 1, 128, {}),
    (31, 7, 16, 64, BF16, 1, 128, {}),
    (33, 12, 256, 192, BF16, 0, 128, dict(ldx=200, ldw=256)),
    (70, 11, 48, 64, F16, 0, 128, {}),
    (96, 5, 256, 128, F16, 1, 128, dict(api="sched")),                   # sched = NULL
    (32, 9, 512, 64, BF16, 1, 128, {}),
    # 256 tile.  Epilogues: element by element (B % 4 != 0), 16-byte rows (4 | B), LDS-staged whole tiles (f16, 32 | B, 256 | H, full tile)
    (33, 130, 256, 192, BF16, 0, 256, {}),                               # ragged second group, odd K-tile count
    (33, 130, 256, 64, F16, 1, 256, {}),
    (5, 820, 256, 128, F16, 0, 256, {}),
    (31, 140, 256, 64, BF16, 1, 256, {}),
    (70, 60, 256, 64, F16, 0, 256, {}),
    (96, 44, 256, 128, BF16, 0, 256, dict(ldx=136, ldw=192)),            # 16-byte rows, f32
    (96, 44, 256, 128, F16, 1, 256, {}),                                 # staged; M = 4224 = 16.5 tiles: the last tile row takes the 16-byte rows
    (36, 120, 256, 64, F16, 1, 256, {}),                                 # 4 | B, ragged group, f16: 8-byte stores
    (32, 72, 512, 1024, F16, 1, 256, {}),                                # headline-like, layers 1 and 2
    (32, 72, 512, 1024, BF16, 0, 256, {}),
    (32, 72, 512, 5120, F16, 1, 256, dict(w_keep=0.25)),                 # headline-like, layer 0
    (32, 72, 512, 5120, BF16, 1, 256, dict(w_keep=0.25)),
]


@pytest.mark.parametrize("B,T,H,K,dt,gx16,tile,kw", GX, ids=_ids(GX))
def test_gx_exact(B, T, H, K, dt, gx16, tile, kw):
    _run_gx(B, T, H, K, dt, gx16, tile, **kw)


# (B, T, H, Hprev, f16 image, tile, keyword arguments): A read from an hx image
GX_HX = [
    (5, 33, 48, 64, 0, 128, dict(api="plain")),
    (5, 33, 48, 64, 1, 128, {}),
    (33, 12, 256, 256, 0, 128, dict(ldw=520)),
    (32, 9, 512, 512, 1, 128, dict(api="sched")),                        # sched = NULL
    (33, 130, 256, 64, 1, 256, {}),                                      # one K-tile per direction
    (33, 130, 256, 256, 0, 256, {}),
    (96, 44, 256, 512, 1, 256, {}),
    (32, 72, 512, 512, 1, 256, {}),                                      # layers 1 and 2 of every f16 inference forward
    (70, 60, 256, 256, 0, 256, dict(api="plain")),
]


@pytest.mark.parametrize("B,T,H,hprev,gx16,tile,kw", GX_HX, ids=_ids(GX_HX))
def test_gx_from_hx_exact(B, T, H, hprev, gx16, tile, kw):
    _run_gx(B, T, H, 0, F16, gx16, tile, hprev=hprev, **kw)


# ------------------------------------------------------------------ logits (EPI_LOGITS; 128 tile only)
def _run_logits(B, T, N, K, dt, api="dt", hprev=0):
    lib, _, s = _api()
    M = T * B
    if hprev:
        K, dt = 2 * hprev, F16
    A, W, b, ref = _problem(1, M, N, K, 3, 11 + B + T + N + K)
    ownW, pW = _dev16(_place(W, _ru(N, 128), K), dt)
    ownB, pB = _dev32(b)
    out = _Out(B * N * T, False)
    if hprev:
        ownA, pA = _dev16(_hx_image(A[0], B, T, hprev), F16)
        _ok(lib.mt_gemm_logits_from_hx(pA, pW, K, pB, out.ptr, B, T, N, hprev, s))
    else:
        ownA, pA = _dev16(_place(A, _ru(M, 128), K), dt)
        if api == "plain":
            assert dt == BF16
            _ok(lib.mt_gemm_logits(pA, K, pW, K, pB, out.ptr, B, T, N, K, s))
        else:
            _ok(lib.mt_gemm_logits_dt(pA, K, pW, K, pB, out.ptr, B, T, N, K, dt, s))
    out.check(_logits_index(B, T, N), ref, torch.float32, f"logits B={B} T={T} N={N} K={K} dt={dt} hprev={hprev}")


@pytest.mark.parametrize("B,T,N,K,dt,api,hprev", [
    (3, 50, 88, 64, BF16, "plain", 0), (33, 41, 88, 1024, F16, "dt", 0), (5, 301, 264, 128, BF16, "dt", 0), (32, 72, 264, 192, F16, "dt", 0),
    (3, 50, 88, 0, F16, "hx", 64), (33, 41, 88, 0, F16, "hx", 512), (32, 72, 264, 0, F16, "hx", 256), (5, 301, 264, 0, F16, "hx", 64)])
def test_logits_exact(B, T, N, K, dt, api, hprev):
    _run_logits(B, T, N, K, dt, api, hprev)


# ------------------------------------------------------------------ dh (EPI_LSTM_DH; bf16 operands, no bias, dropout mask)
def _run_dh(B, T, H, Hv, K, p, tile):
    lib, _, s = _api()
    M, N = T * B, 2 * Hv
    assert _tile(M, N) == tile, f"dispatch moved: dh B={B} T={T} Hv={Hv} was meant for the {tile} tile"
    A, W, b, ref = _problem(1, M, N, K, 3, 5 + B + T + Hv + K)
    ref = ref[0] - b.double()
    seed, layer = 1234567, 2
    if p > 0:
        m, n = _mn(M, N)
        keep = _dropout_keep(seed, layer, m * (2 * Hv) + n, p)
        assert 0.4 < keep.mean() < 0.6
        ref = torch.where(torch.from_numpy(keep), ref * (1.0 / (1.0 - p)), torch.zeros_like(ref))       # 1 / (1 - 0.5) = 2: exact
    _representable(ref, torch.float32)
    ownA, pA = _dev16(_place(A, _ru(M, 128), K), BF16)
    ownW, pW = _dev16(_place(W, _ru(N, 128), K), BF16)
    out = _Out(_cdiv(B, 32) * T * 2 * (H // 8) * 256, False)
    _ok(lib.mt_gemm_lstm_dh(pA, K, pW, K, out.ptr, B, T, H, Hv, K, p, seed, layer, s))
    out.check(_dh_index(B, T, H, Hv), ref, torch.float32, f"dh B={B} T={T} H={H} Hv={Hv} K={K} p={p}")


@pytest.mark.parametrize("B,T,H,Hv,K,p,tile", [
    (5, 33, 48, 40, 128, 0.0, 128), (5, 33, 48, 40, 128, 0.5, 128), (33, 12, 256, 256, 64, 0.5, 128), (70, 11, 48, 48, 192, 0.0, 128),
    (64, 256, 264, 256, 128, 0.5, 256),          # the 256 kernel's hoisted path (4 | B), Hv < H
    (36, 456, 256, 256, 64, 0.0, 256),           # hoisted, ragged second group
    (33, 497, 264, 256, 64, 0.5, 256),           # generic path (B % 4 != 0), ragged, Hv < H
    (33, 497, 256, 256, 192, 0.0, 256)])
def test_dh_exact(B, T, H, Hv, K, p, tile):
    _run_dh(B, T, H, Hv, K, p, tile)


# ------------------------------------------------------------------ argument errors
def test_argument_errors_write_nothing():
    lib, last_error, s = _api()
    K, M, N = 64, 128, 128
    own, pa = _dev16(torch.zeros(128 * 256), BF16)
    ownB, pb = _dev32(torch.zeros(1024))
    out = _Out(1 << 16, False)
    calls = {
        "K % 64 != 0": lambda: lib.mt_gemm_f32acc_dt(pa, 96, pa, 96, pb, out.ptr, N, M, N, 96, BF16, s),
        "ldw < K": lambda: lib.mt_gemm_f32acc_dt(pa, 128, pa, 64, pb, out.ptr, N, M, N, 128, BF16, s),
        "lda % 8 != 0": lambda: lib.mt_gemm_bf16_f32acc(pa, 68, pa, 64, pb, out.ptr, N, M, N, K, s),
        "ldc < N": lambda: lib.mt_gemm_f32acc_dt(pa, K, pa, K, pb, out.ptr, N - 1, M, N, K, F16, s),
        "ldc < N (batched)": lambda: lib.mt_gemm_batched_f32(pa, K, 0, 0, pa, K, 0, 0, None, out.ptr, N - 1, 0, 0, M, N, K, 1, 1, s),
        "odd sC (16-bit out)": lambda: lib.mt_gemm_batched_h16out_dt(pa, K, 0, 0, pa, K, 0, 0, None, out.ptr, N, 1, 0, M, N, K, 2, 1, 0, BF16, s),
        "operand type": lambda: lib.mt_gemm_f32acc_dt(pa, K, pa, K, pb, out.ptr, N, M, N, K, 2, s),
        "NULL bias for gx": lambda: lib.mt_gemm_lstm_gx_dt(pa, K, pa, K, None, out.ptr, 4, 4, 16, K, BF16, s),
        "NULL bias for gx from hx": lambda: lib.mt_gemm_lstm_gx_from_hx_ex(pa, pa, 128, None, out.ptr, 4, 4, 16, 64, 0, s),
        "H % 8 != 0 for gx": lambda: lib.mt_gemm_lstm_gx(pa, K, pa, K, pb, out.ptr, 4, 4, 12, K, s),
        "N % 88 != 0 for logits": lambda: lib.mt_gemm_logits_dt(pa, K, pa, K, pb, out.ptr, 4, 4, 96, K, BF16, s),
        "N % 88 != 0 for logits from hx": lambda: lib.mt_gemm_logits_from_hx(pa, pa, 128, pb, out.ptr, 4, 4, 96, 64, s),
        "Hprev % 64 != 0": lambda: lib.mt_gemm_lstm_gx_from_hx(pa, pa, 128, pb, out.ptr, 4, 4, 16, 48, s),
        "Hprev % 64 != 0 (logits)": lambda: lib.mt_gemm_logits_from_hx(pa, pa, 128, pb, out.ptr, 4, 4, 88, 32, s),
        "ldw < 2 Hprev": lambda: lib.mt_gemm_lstm_gx_from_hx_ex(pa, pa, 64, pb, out.ptr, 4, 4, 16, 64, 0, s),
        "Hv > H for dh": lambda: lib.mt_gemm_lstm_dh(pa, K, pa, K, out.ptr, 4, 4, 16, 24, K, 0.0, 1, 1, s),
        "p = 1 for dh": lambda: lib.mt_gemm_lstm_dh(pa, K, pa, K, out.ptr, 4, 4, 16, 16, K, 1.0, 1, 1, s),
        "NULL A": lambda: lib.mt_gemm_f32acc_dt(None, K, pa, K, pb, out.ptr, N, M, N, K, BF16, s),
    }
    for what, call in calls.items():
        assert call() == EINVAL, what
        assert last_error(), what
    torch.cuda.synchronize()
    assert out.untouched()


# ------------------------------------------------------------------ realistic data: the project's f32 bound, and RNE of 16-bit outputs
def _realistic(M, N, K, dt, seed, bias_center=0.0):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(1, M, K, generator=g).to(_tdt(dt)).float()
    W = ((torch.rand(1, N, K, generator=g) * 2 - 1) / np.sqrt(K)).to(_tdt(dt)).float()
    bias = bias_center + (torch.rand(N, generator=g) * 2 - 1) * (500.0 if bias_center else 1.0)
    ref = A[0].double() @ W[0].double().t() + bias.double()          # float64 product of the ROUNDED operands
    return A, W, bias, ref


@pytest.mark.parametrize("M,N,K,dt,tile", [(300, 200, 192, BF16, 128), (1000, 88, 1024, F16, 128), (16385, 640, 192, F16, 256), (4096, 2048, 1024, BF16, 256)])
def test_rowmajor_f32_realistic(M, N, K, dt, tile):
    lib, _, s = _api()
    assert _tile(M, N) == tile
    A, W, bias, ref = _realistic(M, N, K, dt, M + N + K)
    ownA, pA = _dev16(_place(A, _ru(M, 128), K), dt)
    ownW, pW = _dev16(_place(W, _ru(N, 128), K), dt)
    ownB, pB = _dev32(bias)
    C = torch.full((M, N), NAN, device="cuda")
    _ok(lib.mt_gemm_f32acc_dt(pA, K, pW, K, pB, C.data_ptr(), N, M, N, K, dt, s))
    err = (C.double().cpu() - ref).abs().max().item()
    print(f"rowmajor realistic M={M} N={N} K={K} dt={dt}: max err {err:.3e} (bound {2e-4 * np.sqrt(K):.3e})")
    assert err < 2e-4 * np.sqrt(K), err


def _h16_band(ref, K, out_dtype):
    """RNE of the float64 result, and the elements excused from equalling it: those whose float64 result lies within the f32 bound
    2e-4 sqrt(K) of a rounding boundary (there, either neighbour is accepted)."""
    bound = 2e-4 * np.sqrt(K)
    lo, hi, rne = (ref - bound).to(out_dtype), (ref + bound).to(out_dtype), ref.to(out_dtype)
    return lo, hi, rne, lo != hi


@pytest.mark.parametrize("B,T,H,K,dt,gx16,tile", [(5, 33, 48, 128, BF16, 0, 128), (32, 72, 512, 1024, F16, 0, 256),
                                                  (33, 12, 256, 192, F16, 1, 128), (32, 72, 512, 1024, F16, 1, 256), (33, 130, 256, 64, BF16, 1, 256)])
def test_gx_realistic(B, T, H, K, dt, gx16, tile):
    """randn activations, U(+-1/sqrt K) weights.  f32 image: within 2e-4 sqrt(K) of the float64 product of the rounded operands.  f16 image:
    equal to the round-to-nearest-even of that product except where it lies within the same bound of a rounding boundary, and such
    excused elements are at most 1 % of a case.  With a bias of order 1 the f16 spacing (5e-4 near 0.5) is below the bound itself and
    every element would be excused, so the bias of the f16 cases is 6000 +- 500 -- spacing 4 in [4096, 8192), 0.3 % within the bound
    of a boundary at K = 1024 (counted below on the reference alone) -- which leaves the fractional bits of the f32 sum to the rounding."""
    lib, _, s = _api()
    M, N = T * B, 8 * H
    assert _tile(M, N) == tile
    A, W, bias, ref = _realistic(M, N, K, dt, B + T + H + K, 6000.0 if gx16 else 0.0)
    ownA, pA = _dev16(_place(A, _ru(M, 128), K), dt)
    ownW, pW = _dev16(_place(W, _ru(N, 128), K), dt)
    ownB, pB = _dev32(bias)
    n_f32 = lib.mt_lstm_gx_bytes(B, T, H) // 4
    out = _Out(2 * n_f32 if gx16 else n_f32, gx16)
    _ok(lib.mt_gemm_lstm_gx_dt(pA, K, pW, K, pB, out.ptr, B, T, H, K, dt | (GX_F16 if gx16 else 0), s))
    body = out.buf.cpu()[GUARD:GUARD + out.n]
    pos = torch.from_numpy(_gx_index(B, T, H).reshape(-1))
    if not gx16:
        got = body[pos].view(torch.float32).double().reshape(M, N)
        err = (got - ref).abs().max().item()
        print(f"gx realistic f32 B={B} T={T} H={H} K={K}: max err {err:.3e}")
        assert err < 2e-4 * np.sqrt(K), err
        return
    got = body[pos].view(torch.float16).reshape(M, N)
    lo, hi, rne, excused = _h16_band(ref, K, torch.float16)
    share = excused.double().mean().item()
    print(f"gx realistic f16 B={B} T={T} H={H} K={K}: {share:.4%} of the reference within the bound of a boundary")
    assert share <= 0.01, share
    assert torch.equal(got[~excused], rne[~excused])
    ge = got[excused]
    assert bool(((ge == lo[excused]) | (ge == hi[excused])).all())


@pytest.mark.parametrize("M,N,K,dt,relu,tile", [(300, 200, 192, BF16, 1, 128), (16385, 640, 192, F16, 0, 256), (8321, 1152, 1024, BF16, 1, 256)])
def test_h16out_realistic(M, N, K, dt, relu, tile):
    """As the f16 gx case above for the 16-bit row-major output (bias 6000 +- 500: f16 spacing 4, bf16 spacing 32)."""
    lib, _, s = _api()
    assert _tile(M, N) == tile
    A, W, bias, ref = _realistic(M, N, K, dt, M + N + K + 1, 6000.0)
    if relu:
        ref = ref.clamp(min=0)
    ownA, pA = _dev16(_place(A, _ru(M, 128), K), dt)
    ownW, pW = _dev16(_place(W, _ru(N, 128), K), dt)
    ownB, pB = _dev32(bias)
    out = _Out(M * N, True)
    _ok(lib.mt_gemm_batched_h16out_dt(pA, K, 0, 0, pW, K, 0, 0, pB, out.ptr, N, 0, 0, M, N, K, 1, 1, relu, dt, s))
    got = out.buf.cpu()[GUARD:GUARD + out.n].view(_tdt(dt)).reshape(M, N)
    lo, hi, rne, excused = _h16_band(ref, K, _tdt(dt))
    share = excused.double().mean().item()
    print(f"h16out realistic M={M} N={N} K={K} dt={dt}: {share:.4%} of the reference within the bound of a boundary")
    assert share <= 0.01, share
    assert torch.equal(got[~excused], rne[~excused])
    ge = got[excused]
    assert bool(((ge == lo[excused]) | (ge == hi[excused])).all())


# ------------------------------------------------------------------ environment-selected paths: one fresh child process each
# gemm256p_kernel: (B, T, H, K, dt, f16 image, kernel, keyword arguments).  256 CUs; the grid is min(tiles, CUs + tiles / quota) workgroups
# with a quota of 15 tiles at K = 1024 and 3 at K = 5120.
PERSIST = [
    (32, 128, 256, 1024, F16, 1, "persist", {}),                         # 128 tiles: fewer than CUs, one tile per workgroup
    (32, 131, 512, 1024, BF16, 1, "persist", {}),                        # 272 tiles = the grid; M = 4192: the last tile row holds 96 rows
    (32, 256, 512, 1024, F16, 1, "persist", {}),                         # 512 tiles on 291 workgroups: several tiles per workgroup, stealing
    (32, 256, 512, 5120, BF16, 1, "persist", dict(w_keep=0.25)),         # 512 tiles, quota 3: workgroups hand over and leave
    (32, 128, 256, 5120, F16, 1, "persist", dict(w_keep=0.25)),
    (32, 128, 256, 0, F16, 1, "persist", dict(hprev=512)),               # A from hx images
    (32, 131, 512, 0, F16, 1, "persist", dict(hprev=512)),
    (32, 256, 512, 0, F16, 1, "persist", dict(hprev=512)),
    (64, 64, 256, 0, F16, 1, "persist", dict(hprev=2560, w_keep=0.25)),  # K = 5120 through the hx loader, two batch groups
    # just outside persist_ok: the one-tile kernels, same results
    (33, 125, 256, 1024, F16, 1, 256, {}),                               # B % 32 != 0
    (32, 128, 256, 960, F16, 1, 256, {}),                                # 15 K-tiles
    (32, 128, 256, 1024, F16, 0, 256, {}),                               # f32 image
    (32, 127, 256, 1024, BF16, 1, 256, {}),                              # M = 4064 < 4096
    (32, 128, 256, 0, F16, 0, 256, dict(hprev=512)),
]


def _child_persist():
    n = 0
    for B, T, H, K, dt, gx16, kernel, kw in PERSIST:
        tile = kernel if kernel != "persist" else 0
        _run_gx(B, T, H, K, dt, gx16, tile, api="sched", sched=True, kernel=kernel, **kw)
        n += 1
    _run_gx(32, 128, 256, 1024, F16, 1, 256, api="sched", sched=False)      # sched = NULL
    return n + 1


def _child_tile128():
    """The 256-tile cases again on gemm_kernel (large tile counts exercise its XCD tile order).  launch_hx does not read MT_GEMM_TILE."""
    n = 0
    for M, N, K, dt, tile, kw in ROWMAJOR:
        if tile == 256:
            _run_rowmajor(M, N, K, dt, 128, **kw); n += 1
    for M, N, K, dt, tile, kw in BATCHED:
        if tile == 256:
            _run_rowmajor(M, N, K, dt, 128, api="batched", **kw); n += 1
    for M, N, K, dt, tile, kw in H16OUT:
        if tile == 256:
            kw = dict(kw); kw.setdefault("api", "batched")
            _run_rowmajor(M, N, K, dt, 128, out16=True, **kw); n += 1
    for B, T, H, K, dt, gx16, tile, kw in GX:
        if tile == 256:
            _run_gx(B, T, H, K, dt, gx16, 128, **kw); n += 1
    for B, T, H, Hv, K, p in ((64, 256, 264, 256, 128, 0.5), (33, 497, 264, 256, 64, 0.5)):
        _run_dh(B, T, H, Hv, K, p, 128); n += 1
    return n


_CHILDREN = {"persist": (_child_persist, {"MT_GEMM_PERSIST": "1"}, 420), "tile128": (_child_tile128, {"MT_GEMM_TILE": "128"}, 420)}


def _run_child(name):
    env = {k: v for k, v in os.environ.items() if k not in ("MT_GEMM_PERSIST", "MT_GEMM_TILE", "MT_GEMM_PARK", "MT_GEMM_TPW", "MT_GEMM_PDBG")}
    env.update(_CHILDREN[name][1])
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=_CHILDREN[name][2], env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the {name} child did not finish in {_CHILDREN[name][2]} s; nothing further is started on the GPU.\n{(e.stdout or b'')[-3000:]}", returncode=3)
    if r.returncode < 0:
        pytest.exit(f"the {name} child died on signal {-r.returncode}; nothing further is started on the GPU.\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(rf"gemm child {name}: (\d+) cases exact", last)
    assert m and int(m.group(1)) >= 10, r.stdout[-3000:]
    return int(m.group(1))


def test_persistent_kernel_in_a_child_process():
    """MT_GEMM_PERSIST=1: mt_gemm_lstm_gx_sched / mt_gemm_lstm_gx_from_hx_sched on gemm256p_kernel -- tile counts below, equal to and above
    the grid, both operand types, the hx loader -- and shapes just outside persist_ok, all exact and with the sentinel check."""
    assert _run_child("persist") == len(PERSIST) + 1


def test_small_tile_fallback_in_a_child_process():
    """MT_GEMM_TILE=128: the 256-tile cases on the 128 x 128 kernel."""
    _run_child("tile128")


# ------------------------------------------------------------------ every export has a case
def test_every_gemm_export_is_called():
    from music_transcription_amd import _lib
    exported = {n for n in _lib.EXPORTS if n.startswith("mt_gemm_")}
    with open(os.path.abspath(__file__)) as f:
        called = set(re.findall(r"lib\.(mt_gemm_\w+)\(", f.read()))
    assert len(exported) >= 17
    assert called == exported, (sorted(exported - called), sorted(called - exported))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    fn = _CHILDREN[sys.argv[1]][0]
    count = fn()
    torch.cuda.synchronize()
    print(f"gemm child {sys.argv[1]}: {count} cases exact")
