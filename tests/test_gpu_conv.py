"""Convolution conformance: every entry point of csrc/conv.hip and csrc/convg.hip against an exact CPU reference.

The method is that of tests/test_gpu_gemm.py.  Operands are small integers (exact in bf16 and f16) and the biases are integer-valued, so
fp32 accumulation is exact and independent of the summation order while every partial sum stays below 2^24; the reference is
torch.nn.functional.conv2d on the CPU in f32 (+ 1x1 skip, + bias, ReLU, MaxPool2d((2,1)) as applicable) and the comparison is
`torch.equal` on every element.  Every case asserts on the CPU, before anything runs on the GPU, that each value is representable in the
16-bit output type BEFORE it is rounded and that at least a quarter of the post-ReLU outputs are non-zero -- the only exceptions are the
rounding cases, whose values sit on and next to round-to-nearest-even ties and whose reference applies `.to(dtype)`.

Storage layouts are restated here in numpy / torch indexing from include/mt_hip.h and the heads of conv.hip and convg.hip (channels-last
activations, X[(t*B+b)*ldx + fo*Cout + co], W[Cout][(kh*3+kw)*C1 + ci | skip], the tie words); no kernel of the library takes part in a
reference.  Every output lies between two guard bands in a sentinel-filled buffer and everything that is not a logical element (guard
bands, columns Fo*Cout .. ldx-1 of X rows, rows >= T*B, the dropped last frequency row of an odd F under pool) must still hold the
sentinel afterwards.  Every 16-bit input is sized exactly to its documented extent between NaN guard bands; with a position pitch wider
than the channel count the channels outside the slice hold NaN / +-Inf.  Chunks lie back to back with different data, and the `edge`
cases give every chunk's border rows and frames large values: a halo read that leaves chunk b must read zero, not chunk b +- 1.

`_cg_inst()` restates conv_cl_dispatch (with cg_lds_bytes); every mt_conv_cl_* case names the instantiation (KC, BN, NW) it is meant
to reach and asserts that the restatement agrees, so a changed threshold shows up here.  MT_CONVG_WAVES is read once per process: its
`=8` cases run in one fresh child process (this file run as a script).

The reference half alone, without a GPU:  python tests/test_gpu_conv.py cpu
Run only this file:                       python -m pytest tests/test_gpu_conv.py -q -m gpu
"""
import functools
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16 = 0, 1                           # MT_DT_BF16, MT_DT_F16 (include/mt_hip.h)
EINVAL, EUNSUPPORTED = -1, -4              # MT_EINVAL, MT_EUNSUPPORTED
GUARD = 4096                               # elements of guard band on either side of every buffer
SENT32 = 0x7FC0BEEF
SENT16 = 0x7BCD                            # a finite 16-bit pattern far outside every expected value (bf16 2e36, f16 63904)
NAN, INF = float("nan"), float("inf")
LDS = 160 * 1024


def _api():
    from music_transcription_amd._lib import lib, last_error, stream_ptr
    return lib, last_error, stream_ptr()


def _ok(rc):
    if rc != 0:
        from music_transcription_amd._lib import last_error
        raise AssertionError(f"call failed (code {rc}): {last_error()}")


def _ru(x, m):
    return (x + m - 1) // m * m


def _tdt(dt):
    return torch.float16 if dt == F16 else torch.bfloat16


# ------------------------------------------------------------------ dispatch of mt_conv_cl_* (csrc/convg.hip), restated
def _cg_lds(C1, C2, KH, KC, BN):
    """cg_lds_bytes: input tile with halo (row pitch = 18 positions rounded up to whole 256-B bank rows) + skip tile + two weight chunks"""
    nc1 = C1 // 8
    pr1 = max(16 // nc1, 1)
    pitch1 = (18 + pr1 - 1) // pr1 * pr1
    return _ru((16 + KH - 1) * pitch1 * C1 * 2, 1024) + (_ru(16 * 16 * C2 * 2, 1024) if C2 else 0) + 2 * BN * KC * 2


def _waves8():
    m = re.match(r"\s*[+-]?\d+", os.environ.get("MT_CONVG_WAVES", ""))          # atoi
    return bool(m) and int(m.group(0)) == 8


def _cg_inst(C1, C2, Cout, KH, pool=0, accum=0, tie=0, waves8=None):
    """conv_cl_dispatch's choice (KC, BN, NW)."""
    nw = 8 if (_waves8() if waves8 is None else waves8) else 16
    bn256 = Cout % 256 == 0 and not accum and not tie and _cg_lds(C1, C2, KH, 32, 256) <= LDS and (8 if pool else 16) * 16 * 256 * 2 <= LDS
    bn128 = Cout % 128 == 0 and _cg_lds(C1, C2, KH, 32, 128) <= LDS
    kc64 = C1 % 64 == 0 and C2 % 64 == 0 and _cg_lds(C1, C2, KH, 64, 128 if bn128 else 64) <= LDS
    if bn256:
        return (32, 256, nw)
    if kc64 and bn128 and _cg_lds(C1, C2, KH, 64, 64) <= 80 * 1024:
        return (64, 64, 8)
    if kc64 and bn128:
        return (64, 128, nw)
    if kc64:
        return (64, 64, 8)
    if bn128:
        return (32, 128, nw)
    return (32, 64, 8)


ALL_INSTANTIATIONS = {(32, 256, 16), (32, 256, 8), (64, 64, 8), (64, 128, 16), (64, 128, 8), (32, 128, 16), (32, 128, 8), (32, 64, 8)}

# name -> (C1, C2, Cout, KH), and the (KC, BN) each is meant to reach
LAYERS = {
    "fa": ((128, 0, 256, 7), (32, 256)),          # freq_aware_conv
    "rb2c1": ((64, 0, 128, 3), (64, 64)),         # via the 80 KB rule
    "rb2c2": ((128, 64, 128, 3), (64, 128)),
    "dgrad64": ((64, 0, 64, 3), (64, 64)),        # via kc64 alone: the small model's input gradient
    "c32_128": ((32, 0, 128, 3), (32, 128)),
    "rb1c1": ((32, 0, 64, 3), (32, 64)),
    "rb1c2": ((64, 32, 64, 3), (32, 64)),
    "dgrad_rb2": ((128, 128, 128, 3), (32, 64)),  # neither 128-channel tile fits: 164 864 B
}


def _expect_inst(layer, pool=0, accum=0, tie=0, want=None):
    cfg, kcbn = LAYERS[layer]
    want = want or kcbn
    got = _cg_inst(*cfg, pool=pool, accum=accum, tie=tie)
    assert got[:2] == tuple(want), f"dispatch moved: {layer} {cfg} pool={pool} accum={accum} tie={tie} was meant for {want}, restated {got}"
    assert got[2] == (8 if (want[1] == 64 or _waves8()) else 16)
    return got


# ------------------------------------------------------------------ buffers
def _poison(n):
    v = torch.empty(n)
    v[0::3], v[1::3], v[2::3] = NAN, INF, -INF
    return v


def _dev16(body, dt):
    """A 16-bit operand on the device: `body` (f32 values on the CPU) between two NaN guard bands -> (owner, address of the body)"""
    g = torch.full((GUARD,), NAN)
    full = torch.cat([g, body.reshape(-1), g]).to(_tdt(dt)).cuda()
    return full, full.data_ptr() + 2 * GUARD


def _dev32(body):
    g = torch.full((GUARD,), NAN)
    full = torch.cat([g, body.reshape(-1).float(), g]).cuda()
    return full, full.data_ptr() + 4 * GUARD


class _Out:
    """An output buffer of n elements (16-bit, or 32-bit words) between two guard bands, all of it pre-filled with a sentinel."""

    def __init__(self, n, bits16=True):
        self.n, self.bits16 = n, bits16
        self.sent = SENT16 if bits16 else SENT32
        self.buf = torch.full((GUARD + n + GUARD,), self.sent, dtype=torch.int16 if bits16 else torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * (2 if bits16 else 4)

    def preset(self, idx, values, dtype):
        pos = torch.from_numpy(np.ascontiguousarray(idx).reshape(-1)) + GUARD
        self.buf[pos.cuda()] = values.reshape(-1).to(dtype).view(torch.int16).cuda()

    def untouched(self):
        return bool((self.buf == self.sent).all().item())

    def check(self, idx, ref, out_dtype, what=""):
        """Every logical element (body position idx[...]) equals ref[...]; every other element of the buffer is the sentinel."""
        full = self.buf.cpu()
        pos = torch.from_numpy(np.ascontiguousarray(idx).reshape(-1)) + GUARD
        other = torch.ones(full.numel(), dtype=torch.bool)
        if pos.numel():
            assert int(pos.min()) >= GUARD and int(pos.max()) < GUARD + self.n, "reference index outside the buffer"
            other[pos] = False
            assert int((~other).sum()) == pos.numel(), "reference layout maps two logical elements to one slot"
            got = full[pos].view(out_dtype)
            exp = ref.reshape(-1).to(out_dtype)
            if not torch.equal(got, exp):
                bad = torch.nonzero(~(got == exp)).reshape(-1)
                i = int(bad[0])
                where = np.unravel_index(i, idx.shape)
                raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ; first at logical {tuple(int(k) for k in where)} "
                                     f"of {tuple(idx.shape)}: got {got[i].item()}, want {exp[i].item()}")
        stray = int((full[other] != self.sent).sum())
        assert stray == 0, f"{what}: {stray} elements outside the logical output were written"


# ------------------------------------------------------------------ layouts (include/mt_hip.h, heads of conv.hip / convg.hip)
def _cl_index(B, C, Fo, T):
    """channels-last activation: element (b, c, f, t) at ((b Fo + f) T + t) C + c"""
    b, c, f, t = np.ogrid[:B, :C, :Fo, :T]
    return ((b * Fo + f) * T + t) * C + c


def _x_index(B, C, Fo, T, ldx):
    """GEMM-A rows: element (b, c, f, t) at (t B + b) ldx + f C + c"""
    b, c, f, t = np.ogrid[:B, :C, :Fo, :T]
    return (t * B + b) * ldx + f * C + c


def _cl_body(x, pitch=None, off=0):
    """x[B][C][F][T] as channels-last storage with `pitch` elements between positions and the channels at off .. off + C - 1; every other
    channel of the wider tensor holds NaN / +-Inf.  The kernel is given the address of element `off`."""
    B, C, F, T = x.shape
    pitch = pitch or C
    body = _poison(B * F * T * pitch)
    body.view(B * F * T, pitch)[:, off:off + C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    return body


def _pack_w(w, ws=None):
    """w[Cout][C1][KH][3] (+ ws[Cout][C2]) -> W[Cout][(kh*3 + kw)*C1 + ci | skip]"""
    wk = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    return torch.cat([wk, ws], 1).contiguous() if ws is not None else wk.contiguous()


# ------------------------------------------------------------------ exact data and references
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _acts(g, shape, edge):
    """activations in {-2 .. 2}, half of them zeroed; edge: the border rows and frames of every chunk are dense +-{3, 4}"""
    x = _ints(g, shape, -2, 2) * (torch.rand(shape, generator=g) < 0.5)
    if edge:
        big = (_ints(g, shape, 3, 4)) * (1 - 2 * _ints(g, shape, 0, 1))
        m = torch.zeros(shape, dtype=torch.bool)
        m[:, :, 0], m[:, :, -1], m[:, :, :, 0], m[:, :, :, -1] = True, True, True, True
        x = torch.where(m, big, x)
    return x


def _density(K):
    return 0.5 if K <= 320 else 0.25 if K <= 640 else 0.125


def _weights(g, shape, K):
    return _ints(g, shape, -1, 1) * (torch.rand(shape, generator=g) < _density(K) * 1.5)      # a third of {-1, 0, 1} is zero already


@functools.lru_cache(maxsize=2)
def _cg_problem(layer, B, F, T, seed=0, edge=False, pitchA=0, offA=0, pitchS=0, offS=0, bias_kind="int"):
    """A channels-last convolution problem and its exact pre-activation z[B][Cout][F][T] (conv + skip, WITHOUT the bias)."""
    C1, C2, Cout, KH = LAYERS[layer][0]
    K = KH * 3 * C1 + C2
    g = torch.Generator().manual_seed(1000 * seed + 7 * F + 13 * T + B + K)
    x = _acts(g, (B, C1, F, T), edge)
    s = _acts(g, (B, C2, F, T), edge) if C2 else None
    w = _weights(g, (Cout, C1, KH, 3), K)
    ws = _weights(g, (Cout, C2), K) if C2 else None
    bias = _ints(g, (Cout,), -3, 3)
    assert K * 4 * 1 + 4096 < 2 ** 24                                  # every partial sum, in any order, is an exact f32 integer
    z = TF.conv2d(x, w, None, padding=(KH // 2, 1))
    if C2:
        z = z + TF.conv2d(s, ws[:, :, None, None])
    if F * T <= 64:                                                     # small enough: the f32 reference against f64
        z64 = TF.conv2d(x.double(), w.double(), None, padding=(KH // 2, 1)) + (TF.conv2d(s.double(), ws.double()[:, :, None, None]) if C2 else 0)
        assert torch.equal(z.double(), z64)
    if bias_kind != "int":                                              # rounding cases: totals on and next to round-to-nearest-even ties
        base = {BF16: 300.0, F16: 2100.0}[bias_kind]
        bias = base + _ints(g, (Cout,), 0, 7) * 0.5                     # spacing of the output type is 2 there: odd integers are ties
    return SimpleNamespace(layer=layer, B=B, F=F, T=T, C1=C1, C2=C2, Cout=Cout, KH=KH, x=x, s=s, W=_pack_w(w, ws), bias=bias, z=z,
                           pitchA=pitchA or C1, offA=offA, pitchS=pitchS or C2, offS=offS, rounding=bias_kind != "int")


def _epilogue(z, bias, relu, pool):
    v = z + bias[None, :, None, None]
    if pool:
        v = TF.max_pool2d(v, (2, 1)) if v.shape[2] >= 2 else v[:, :, :0]
    return (torch.relu(v) if relu else v), v


def _check_exactness(pre, post_relu, out_dtype, rounding=False, what=""):
    """The conditions under which a 16-bit comparison discriminates: the share of pre-rounding values not representable in the output
    type is 0, and at least a quarter of the post-ReLU outputs are non-zero."""
    if pre.numel() == 0:
        return
    if not rounding:
        assert torch.equal(pre, pre.to(out_dtype).float()), f"{what}: the reference is not exact in {out_dtype} (max |z| {float(pre.abs().max())})"
    share = float((torch.relu(post_relu) != 0).float().mean())
    assert share >= 0.25, f"{what}: only {share:.3f} of the post-ReLU outputs are non-zero"


def _cg_expected(P, dt, relu, pool, prev=None):
    out, pre = _epilogue(P.z, P.bias, relu, pool)
    what = f"{P.layer} B={P.B} F={P.F} T={P.T} dt={dt} relu={relu} pool={pool}"
    _check_exactness(pre, out, _tdt(dt), P.rounding, what)
    if P.rounding:
        frac = float((pre.to(_tdt(dt)).float() != pre).float().mean())
        assert frac > 0.25, f"{what}: the rounding case rounds only {frac:.3f} of its values"
    if prev is not None:
        out = out + prev
        assert torch.equal(out, out.to(_tdt(dt)).float()), f"{what}: the accumulated sum is not exact"
    return out


MODES = ("cl", "x8", "x4")     # channels-last; GEMM rows with ldx % 8 == 0 (staged epilogue); ldx % 8 != 0 (direct epilogue)


def _cg_geometry(P, pool, mode):
    Fo = P.F // 2 if pool else P.F
    if mode == "cl":
        return Fo, 0, _cl_index(P.B, P.Cout, Fo, P.T), P.B * Fo * P.T * P.Cout
    ldx = Fo * P.Cout + (64 if mode == "x8" else 4)
    return Fo, ldx, _x_index(P.B, P.Cout, Fo, P.T, ldx), (P.T * P.B + 3) * ldx        # three rows behind T*B: never written


def _cg_operands(P, dt, cache):
    key = (id(P), dt)
    if key not in cache:
        a = _dev16(_cl_body(P.x, P.pitchA, P.offA), dt)
        s = _dev16(_cl_body(P.s, P.pitchS, P.offS), dt) if P.C2 else (None, None)
        cache[key] = (a, s, _dev16(P.W, dt), _dev32(P.bias))
    return cache[key]


def _cg_run(P, dt, relu, pool, mode, accum=0, cache=None, api=None):
    """One call of mt_conv_cl_{bf16, dt, ex} on problem P, compared element by element."""
    lib, _, st = _api()
    cache = {} if cache is None else cache
    Fo, ldx, idx, n = _cg_geometry(P, pool, mode)
    prev = None
    if accum:
        g = torch.Generator().manual_seed(P.F + P.T)
        prev = _ints(g, (P.B, P.Cout, Fo, P.T), -8, 8)
    exp = _cg_expected(P, dt, relu, pool, prev)
    (ownA, pA), (ownS, pS), (ownW, pW), (ownB, pB) = _cg_operands(P, dt, cache)
    pA += 2 * P.offA
    pS = pS + 2 * P.offS if P.C2 else None
    out = _Out(n)
    if accum:
        out.preset(idx, prev, _tdt(dt))
    plain = P.pitchA == P.C1 and (not P.C2 or P.pitchS == P.C2) and not accum
    api = api or ("ex" if not plain else "bf16" if dt == BF16 and relu else "dt")
    dims = (P.B, P.F, P.T, P.C1, P.C2, P.Cout, P.KH, relu, pool, int(mode != "cl"), ldx)
    if api == "bf16":
        assert plain and dt == BF16
        _ok(lib.mt_conv_cl_bf16(pA, pS, pW, pB, out.ptr, *dims, st))
    elif api == "dt":
        assert plain
        _ok(lib.mt_conv_cl_dt(pA, pS, pW, pB, out.ptr, *dims, dt, st))
    else:
        _ok(lib.mt_conv_cl_ex(pA, P.pitchA, pS, P.pitchS, pW, pB, out.ptr, *dims, accum, dt, st))
    out.check(idx, exp, _tdt(dt), f"{P.layer} B={P.B} F={P.F} T={P.T} dt={dt} relu={relu} pool={pool} mode={mode} accum={accum}")


# ------------------------------------------------------------------ mt_conv_cl_*: every instantiation in every setting
SETTINGS = [(dt, pool, mode, relu) for dt in (BF16, F16) for pool in (0, 1) for mode in MODES for relu in (0, 1)]
SETTINGS_SHAPE = (3, 19, 37)          # B = 3; F = 16 + 3 (odd: a dropped row under pool); T = 2 tiles + 5


def _settings_cases(layer):
    P = _cg_problem(layer, *SETTINGS_SHAPE, edge=True)
    for dt, pool, mode, relu in SETTINGS:
        _cg_expected(P, dt, relu, pool)
        yield P, dt, relu, pool, mode


@pytest.mark.parametrize("layer", list(LAYERS))
def test_conv_cl_every_setting(layer):
    """One instantiation in all 24 settings: both operand types x pool x {channels-last, X staged, X direct} x relu, at a shape with an odd
    F, a ragged T and three chunks back to back whose border rows and frames are large."""
    cache = {}
    for P, dt, relu, pool, mode in _settings_cases(layer):
        _expect_inst(layer, pool=pool)
        _cg_run(P, dt, relu, pool, mode, cache=cache)


# (B, F, T): below one tile, exactly one, one more, several with a ragged last one; each shape takes four of the settings in turn
SHAPES = [(3, 1, 1), (1, 2, 1), (2, 1, 20), (3, 16, 16), (2, 17, 17), (1, 33, 50), (4, 3, 16), (1, 16, 65)]


def _shape_cases(layer):
    k = sum(LAYERS[layer][0])
    for i, (B, F, T) in enumerate(SHAPES):
        P = _cg_problem(layer, B, F, T, seed=1)
        for j in range(4):
            dt, pool, mode, relu = SETTINGS[(k + 7 * i + 5 * j) % len(SETTINGS)]
            _cg_expected(P, dt, relu, pool)
            yield P, dt, relu, pool, mode


@pytest.mark.parametrize("layer", list(LAYERS))
def test_conv_cl_tile_edges(layer):
    """F and T below, at and just above one 16 x 16 tile (F = 1 under pool writes nothing at all)."""
    for P, dt, relu, pool, mode in _shape_cases(layer):
        _expect_inst(layer, pool=pool)
        _cg_run(P, dt, relu, pool, mode)


# CNNRNNModelLarge at n_mels = 320, T = 938 (csrc/model_large.hip): (layer, F, relu, pool, mode, dt)
REAL = [("rb1c1", 160, 1, 0, "cl", F16), ("rb1c2", 160, 1, 1, "cl", F16), ("rb2c1", 80, 1, 0, "cl", F16), ("rb2c2", 80, 1, 0, "cl", BF16),
        ("fa", 80, 1, 1, "x8", F16)]


def _real_case(layer, F, relu, pool):
    P = _cg_problem(layer, 1, F, 938, seed=2)
    return P


@pytest.mark.parametrize("layer,F,relu,pool,mode,dt", REAL, ids=[c[0] for c in REAL])
def test_conv_cl_model_layers_at_their_real_extent(layer, F, relu, pool, mode, dt):
    P = _real_case(layer, F, relu, pool)
    _expect_inst(layer, pool=pool)
    _cg_run(P, dt, relu, pool, mode)


@pytest.mark.parametrize("layer,want", [("fa", (64, 128)), ("rb1c1", (32, 64)), ("c32_128", (32, 128)), ("dgrad_rb2", (32, 64))])
def test_conv_cl_accumulate(layer, want):
    """accum = 1 onto a non-zero integer `out` (always the direct epilogue); it turns the 256-channel tile off."""
    P = _cg_problem(layer, 3, 19, 37, edge=True)
    cache = {}
    for dt, pool, mode, relu in ((BF16, 0, "cl", 0), (F16, 1, "x8", 1), (BF16, 1, "cl", 1), (F16, 0, "x4", 0)):
        _expect_inst(layer, pool=pool, accum=1, want=want)
        _cg_run(P, dt, relu, pool, mode, accum=1, cache=cache)


def _slice_cases():
    # the two half-calls of test_conv_cl_channel_slices_and_accumulate: 128 of 256 channels, offset 0 and 128
    yield _cg_problem("fa", 2, 9, 37, seed=3, pitchA=256, offA=0), 0, (32, 256)
    yield _cg_problem("fa", 2, 9, 37, seed=4, pitchA=256, offA=128), 1, (64, 128)
    # main and skip input both slices of wider tensors
    yield _cg_problem("rb2c2", 3, 17, 21, seed=5, pitchA=192, offA=64, pitchS=200, offS=136), 0, (64, 128)
    yield _cg_problem("rb1c2", 3, 17, 21, seed=6, pitchA=72, offA=8, pitchS=40, offS=0), 1, (32, 64)


def test_conv_cl_channel_slices_exact():
    """Position pitches wider than the channel counts and non-zero channel offsets; the other channels of the wide tensors hold NaN / Inf."""
    for P, accum, want in _slice_cases():
        _expect_inst(P.layer, accum=accum, want=want)
        for dt in (BF16, F16):
            _cg_run(P, dt, 0, 0, "cl", accum=accum)


def _transposed_problem(layer, Cf_out, Cf_in, KH, B, F, T, seed):
    """The input gradient of a forward convolution w_f[Cf_out][Cf_in][KH][3] as both training steps compute it: a convolution of dz
    (Cf_out channels) with W[ci][(kh'*3 + kw')*Cf_out + co] = w_f[co][ci][KH-1-kh'][2-kw'], zero bias.  Reference: conv_transpose2d."""
    g = torch.Generator().manual_seed(seed)
    K = KH * 3 * Cf_out
    dz = _acts(g, (B, Cf_out, F, T), True)
    wf = _weights(g, (Cf_out, Cf_in, KH, 3), K)
    z = TF.conv_transpose2d(dz, wf, padding=(KH // 2, 1))
    W = wf.flip(2, 3).permute(1, 2, 3, 0).reshape(Cf_in, -1).contiguous()
    assert LAYERS[layer][0] == (Cf_out, 0, Cf_in, KH)
    return SimpleNamespace(layer=layer, B=B, F=F, T=T, C1=Cf_out, C2=0, Cout=Cf_in, KH=KH, x=dz, s=None, W=W, bias=torch.zeros(Cf_in), z=z,
                           pitchA=Cf_out, offA=0, pitchS=0, offS=0, rounding=False)


def _transposed_cases():
    yield _transposed_problem("dgrad64", 64, 64, 3, 3, 21, 35, 11)
    yield _transposed_problem("rb2c1", 64, 128, 3, 2, 18, 33, 12)


def test_conv_cl_transposed_convolution_with_flipped_weights():
    for P in _transposed_cases():
        _expect_inst(P.layer)
        _cg_run(P, BF16, 0, 0, "cl", api="bf16")
        _cg_run(P, F16, 0, 0, "cl")


def _rounding_cases():
    for dt in (BF16, F16):
        yield _cg_problem("rb1c1", 2, 17, 20, seed=8, bias_kind=dt), dt


def test_conv_cl_rounds_to_nearest_even():
    """Totals around 300 (bf16) / 2100 (f16), where the output spacing is 2: odd integers are ties, x.5 lies beside them."""
    for P, dt in _rounding_cases():
        for pool, mode in ((0, "cl"), (1, "x4")):
            _cg_expected(P, dt, 0, pool)
            _cg_run(P, dt, 0, pool, mode)


def test_conv_cl_argument_errors_leave_the_output_untouched():
    lib, _, st = _api()
    P = _cg_problem("rb2c2", 1, 4, 4)
    (ownA, pA), (ownS, pS), (ownW, pW), (ownB, pB) = _cg_operands(P, BF16, {})
    out = _Out(4 * 4 * 128)

    def ex(C1=128, C2=64, Cout=128, KH=3, pitchA=128, pitchS=64, S=pS, F=4, T=4):
        return lib.mt_conv_cl_ex(pA, pitchA, S, pitchS, pW, pB, out.ptr, 1, F, T, C1, C2, Cout, KH, 1, 0, 0, 0, 0, BF16, st)

    assert ex(C1=48, pitchA=48) == EUNSUPPORTED
    assert ex(Cout=96) == EUNSUPPORTED
    assert ex(KH=5) == EUNSUPPORTED
    assert ex(pitchA=132) == EINVAL
    assert ex(pitchS=68) == EINVAL
    assert ex(pitchA=120) == EINVAL                                      # narrower than the channel count
    assert ex(S=None) == EUNSUPPORTED
    assert ex(F=8192, T=1024) == EUNSUPPORTED                            # 8192 * 1024 * 128 * 2 B = 2 GB in one chunk
    assert lib.mt_conv_cl_dt(pA, pS, pW, pB, out.ptr, 1, 4, 4, 128, 64, 128, 3, 1, 0, 0, 0, 2, st) == EINVAL     # no such operand type
    assert lib.mt_conv_cl_dt(None, pS, pW, pB, out.ptr, 1, 4, 4, 128, 64, 128, 3, 1, 0, 0, 0, BF16, st) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched()
    assert ex() == 0                                                     # the same arguments, valid
    torch.cuda.synchronize()
    assert not out.untouched()


# ------------------------------------------------------------------ mt_conv_cl_tie
# (layer, B, F, T, instantiation)
TIE = [("rb1c1", 2, 160, 937, (32, 64)),          # the call of train_step.py
       ("c32_128", 3, 17, 37, (32, 128)), ("rb2c1", 2, 19, 16, (64, 64)), ("dgrad64", 3, 2, 5, (64, 64)), ("fa", 2, 9, 21, (64, 128)),
       ("rb1c1", 1, 3, 70, (32, 64))]
TIE_EDGE = ("c32_128", "rb2c1")                   # large border rows (they thin the exact ties out: not on the 7 x 3 case)


def _tie_reference(P):
    """out = conv + bias, raw; tie[(((b (F/2) + fo) T + t) (Cout/32) + co/32) 2 + {0, 1}] bit co % 32 = {z(2fo) > z(2fo+1), z(2fo) < z(2fo+1)}"""
    v = P.z + P.bias[None, :, None, None]
    _check_exactness(v, v, torch.bfloat16, what=f"tie {P.layer}")
    Fh = P.F // 2
    z0, z1 = v[:, :, 0:2 * Fh:2], v[:, :, 1:2 * Fh:2]
    share = float((z0 == z1).float().mean())
    assert share >= 0.01 and bool((z0 > z1).any()) and bool((z0 < z1).any()), f"tie {P.layer}: {share:.4f} exact ties"
    words = []
    for m in (z0 > z1, z0 < z1):
        bits = m.permute(0, 2, 3, 1).reshape(P.B, Fh, P.T, P.Cout // 32, 32).numpy().astype(np.uint64)
        words.append((bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32))
    tie = np.stack(words, -1)                                           # [B][F/2][T][Cout/32][2]
    return v, torch.from_numpy(tie.view(np.int32).copy())


@pytest.mark.parametrize("layer,B,F,T,inst", TIE, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in TIE])
def test_conv_cl_tie_words_are_the_order_of_the_exact_results(layer, B, F, T, inst):
    lib, _, st = _api()
    P = _cg_problem(layer, B, F, T, seed=9, edge=layer in TIE_EDGE)
    v, tie = _tie_reference(P)
    _expect_inst(layer, tie=1, want=inst)
    (ownA, pA), _, (ownW, pW), (ownB, pB) = _cg_operands(P, BF16, {})
    out, words = _Out(B * F * T * P.Cout), _Out(tie.numel(), bits16=False)
    _ok(lib.mt_conv_cl_tie(pA, pW, pB, out.ptr, words.ptr, B, F, T, P.C1, P.Cout, P.KH, st))
    out.check(_cl_index(B, P.Cout, F, T), v, torch.bfloat16, f"tie {layer}: out")
    words.check(np.arange(tie.numel()).reshape(tie.shape), tie, torch.int32, f"tie {layer}: words")     # odd F: the last row has no words


# ------------------------------------------------------------------ mt_conv1_bn_relu_pool(_dt)
# Chunk maxima whose floor 10 log10f(max) - 80 does not depend on the last bit of log10f: ONE -> exactly -80 dB (log10f(1) = 0), with mel
# integers on both sides of it; TINY (and 0) -> about -180 dB through the 1e-10 clamp, below every mel value; BIG -> about +10 dB with
# every mel value of that chunk above it, so that nothing inside the image is clamped and only a border position could show the floor:
# a negative floor cannot tell "0" from "0 clamped", a positive one can.
ONE, TINY, BIG = 1.0, 1e-12, 1e9
# (B, n_mels, T, chunk maxima or None)
CONV1 = [(1, 2, 1, (ONE,)), (2, 3, 63, (TINY, ONE)), (3, 38, 64, (ONE, TINY, BIG)), (4, 64, 65, (ONE, BIG, 0.0, TINY)), (2, 229, 937, (BIG, ONE)),
         (1, 320, 938, (ONE,)), (3, 38, 64, None), (2, 64, 1, None), (2, 2, 5, (BIG, BIG))]


def _zero_sum_taps(g):
    w = torch.zeros(32, 9)
    for c in range(32):
        p = torch.randperm(9, generator=g)
        w[c, p[0]], w[c, p[1]] = 1.0, -1.0
        if c % 2:
            w[c, p[2]], w[c, p[3]] = 1.0, -1.0
    return w


@functools.lru_cache(maxsize=2)
def _c1_problem(B, n_mels, T, cmax, seed=0, bias_kind="int"):
    """mel integers on both sides of -80 dB; every channel's taps sum to zero (one or two +1 / -1 pairs), so the results stay small in the
    interior and a border position shows whether it contributed 0 (zero padding after the clamp) or the floor."""
    g = torch.Generator().manual_seed(seed + 31 * n_mels + T + B)
    mel = _ints(g, (B, n_mels, T), -84, -76) if bias_kind == "int" else _ints(g, (B, n_mels, T), -4, 4)
    for b in range(B):
        if cmax is not None and cmax[b] == BIG:
            mel[b] = _ints(g, (n_mels, T), 11, 19)
    w = _zero_sum_taps(g)
    bias = _ints(g, (32,), -1, 5)
    if bias_kind != "int":
        bias = {BF16: 300.0, F16: 2100.0}[bias_kind] + _ints(g, (32,), 0, 7) * 0.5
    melc = mel.clone()
    if cmax is not None:
        for b in range(B):
            if cmax[b] == ONE:
                melc[b].clamp_(min=-80.0)
                assert bool((mel[b] < -80).any()) and bool((mel[b] > -80).any())
            elif cmax[b] == BIG:
                assert float(mel[b].min()) >= 11.0                      # floor = 10 +- 1e-5
            else:
                assert max(cmax[b], 1e-10) == 1e-10                     # floor near -180: no mel value is close to it
    pre = TF.max_pool2d(TF.conv2d(melc[:, None], w.view(32, 1, 3, 3), padding=1) + bias[None, :, None, None], (2, 1))
    return SimpleNamespace(B=B, n_mels=n_mels, T=T, cmax=cmax, mel=mel, w=w, bias=bias, pre=pre, rounding=bias_kind != "int")


def _c1_expected(P, dt):
    _check_exactness(P.pre, P.pre, _tdt(dt), P.rounding, f"conv1 n_mels={P.n_mels} T={P.T} dt={dt}")
    return torch.relu(P.pre)


def _c1_run(P, dt, plain_api=False):
    lib, _, st = _api()
    exp = _c1_expected(P, dt)
    Fo = P.n_mels // 2
    (om, pm), (ow, pw), (ob, pb) = _dev32(P.mel), _dev32(P.w), _dev32(P.bias)
    oc, pc = _dev32(torch.tensor(P.cmax)) if P.cmax is not None else (None, None)
    out = _Out(P.B * Fo * P.T * 32)
    if plain_api:
        _ok(lib.mt_conv1_bn_relu_pool(pm, pc, pw, pb, out.ptr, P.B, P.n_mels, P.T, st))
    else:
        _ok(lib.mt_conv1_bn_relu_pool_dt(pm, pc, pw, pb, out.ptr, P.B, P.n_mels, P.T, dt, st))
    out.check(_cl_index(P.B, 32, Fo, P.T), exp, _tdt(dt), f"conv1 B={P.B} n_mels={P.n_mels} T={P.T} dt={dt} cmax={P.cmax}")


@pytest.mark.parametrize("B,n_mels,T,cmax", CONV1, ids=[f"{c[0]}-{c[1]}-{c[2]}-{'null' if c[3] is None else 'cmax'}" for c in CONV1])
def test_conv1_exact(B, n_mels, T, cmax):
    """act1 against the exact reference: the 80-dB clamp per chunk (different maxima on the chunks of one batch, NULL), zero padding after
    the clamp, odd n_mels, T around the 64-frame block."""
    P = _c1_problem(B, n_mels, T, cmax)
    _c1_run(P, BF16, plain_api=(n_mels == 38))
    _c1_run(P, F16)


def test_conv1_rounds_to_nearest_even():
    for dt in (BF16, F16):
        _c1_run(_c1_problem(2, 12, 20, None, seed=3, bias_kind=dt), dt)


# ------------------------------------------------------------------ mt_conv2_bn_relu_pool(_dt)
# (B, F1, T, ldx - Fo2*64); 512 persistent workgroups: B * ceil(Fo2/16) * ceil(T/16) tiles
CONV2 = [(3, 2, 16, 64), (2, 3, 37, 8), (3, 19, 48, 24), (5, 32, 17, 0), (2, 33, 64, 64), (1, 160, 938, 64),
         (4, 160, 938, 64),            # 4 * 5 * 59 = 1180 tiles: the persistent loop wraps twice
         (3, 160, 50, 8)]              # 3 * 5 * 4 = 60 tiles: no wrap


def _c2_expected(P, dt):
    return _cg_expected(P, dt, 1, 1)


def _c2_run(P, dt, pad, plain_api=False):
    lib, _, st = _api()
    exp = _c2_expected(P, dt)
    Fo2 = P.F // 2
    ldx = Fo2 * 64 + pad
    (oa, pa), (ow, pw), (ob, pb) = _dev16(_cl_body(P.x), dt), _dev16(P.W, dt), _dev32(P.bias)
    out = _Out((P.T * P.B + 3) * ldx)
    if plain_api:
        _ok(lib.mt_conv2_bn_relu_pool(pa, pw, pb, out.ptr, ldx, P.B, P.F, P.T, st))
    else:
        _ok(lib.mt_conv2_bn_relu_pool_dt(pa, pw, pb, out.ptr, ldx, P.B, P.F, P.T, dt, st))
    out.check(_x_index(P.B, 64, Fo2, P.T, ldx), exp, _tdt(dt), f"conv2 B={P.B} F1={P.F} T={P.T} dt={dt} ldx={ldx}")


@pytest.mark.parametrize("B,F1,T,pad", CONV2, ids=["-".join(map(str, c)) for c in CONV2])
def test_conv2_exact(B, F1, T, pad):
    """X0 in the (t*B+b) row order against the exact reference; sentinel columns behind Fo2*64 and rows behind T*B."""
    n_tiles = B * ((F1 // 2 + 15) // 16) * ((T + 15) // 16)
    assert (n_tiles > 1024) == ((B, F1, T) == (4, 160, 938)) and (B != 3 or n_tiles < 512)
    P = _cg_problem("rb1c1", B, F1, T, seed=20, edge=F1 <= 33)
    _c2_run(P, F16, pad)
    if B * F1 * T < 200000:
        _c2_run(P, BF16, pad, plain_api=(F1 == 19))


def test_conv2_rounds_to_nearest_even():
    for dt in (BF16, F16):
        P = _cg_problem("rb1c1", 2, 18, 20, seed=21, bias_kind=dt)
        lib, _, st = _api()
        pre = TF.max_pool2d(P.z + P.bias[None, :, None, None], (2, 1))
        assert float((pre.to(_tdt(dt)).float() != pre).float().mean()) > 0.25 and bool((pre > 0).all())
        (oa, pa), (ow, pw), (ob, pb) = _dev16(_cl_body(P.x), dt), _dev16(P.W, dt), _dev32(P.bias)
        out = _Out(P.T * P.B * 9 * 64)
        _ok(lib.mt_conv2_bn_relu_pool_dt(pa, pw, pb, out.ptr, 9 * 64, P.B, P.F, P.T, dt, st))
        out.check(_x_index(P.B, 64, 9, P.T, 9 * 64), pre, _tdt(dt), f"conv2 rounding dt={dt}")


# ------------------------------------------------------------------ mt_conv12_bn_relu_pool_dt
# (B, n_mels, T, chunk maxima or None)
CONV12 = [(2, 4, 16, None), (3, 38, 33, (ONE, TINY, ONE)), (1, 64, 50, None), (5, 7, 17, (ONE,) * 5), (2, 229, 100, (TINY, ONE)),
          (2, 320, 938, (ONE, ONE)), (2, 38, 33, (BIG, ONE)), (3, 64, 20, (ONE, BIG, BIG))]


@functools.lru_cache(maxsize=2)
def _c12_problem(B, n_mels, T, cmax):
    """conv1 -> 16-bit -> conv2 on mel in {-4 .. 4}.  ONE / TINY put the clamp floor at -80 / -180 dB, below every mel value (values clamped
    inside the image are pinned by test_conv1_exact and, for the fused kernel, by the bit-identity test of tests/test_gpu_parity.py); a BIG
    chunk has mel in {11 .. 15} above a floor of +10 dB, and zero-sum conv1 taps keep act1 small: a border position must contribute 0."""
    g = torch.Generator().manual_seed(5 * n_mels + T + B)
    mel = _ints(g, (B, n_mels, T), -4, 4)
    w1 = _ints(g, (32, 9), -1, 1) * (torch.rand(32, 9, generator=g) < 0.6)
    if cmax is not None and BIG in cmax:
        w1 = _zero_sum_taps(g)
        for b in range(B):
            if cmax[b] == BIG:
                mel[b] = _ints(g, (n_mels, T), 11, 15)
    b1 = _ints(g, (32,), -3, 3)
    w2 = _weights(g, (64, 32, 3, 3), 640)                               # a quarter non-zero: act1 is non-negative, the sums grow
    b2 = _ints(g, (64,), -3, 3)
    pre1 = TF.max_pool2d(TF.conv2d(mel[:, None], w1.view(32, 1, 3, 3), padding=1) + b1[None, :, None, None], (2, 1))
    act1 = torch.relu(pre1)
    pre2 = TF.max_pool2d(TF.conv2d(act1, w2, None, padding=1) + b2[None, :, None, None], (2, 1))
    return SimpleNamespace(B=B, n_mels=n_mels, T=T, cmax=cmax, mel=mel, w1=w1, b1=b1, W2=_pack_w(w2), b2=b2, pre1=pre1, pre2=pre2)


def _c12_expected(P, dt):
    what = f"conv12 n_mels={P.n_mels} T={P.T} dt={dt}"
    _check_exactness(P.pre1, P.pre1, _tdt(dt), what=what + " (act1)")
    _check_exactness(P.pre2, P.pre2, _tdt(dt), what=what)
    return torch.relu(P.pre2)


@pytest.mark.parametrize("B,n_mels,T,cmax", CONV12, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CONV12])
def test_conv12_exact(B, n_mels, T, cmax):
    lib, _, st = _api()
    P = _c12_problem(B, n_mels, T, cmax)
    Fo2 = n_mels // 4
    ldx = Fo2 * 64 + 64
    for dt in (F16, BF16):
        exp = _c12_expected(P, dt)
        (om, pm), (o1, p1), (ob1, pb1), (ob2, pb2) = _dev32(P.mel), _dev32(P.w1), _dev32(P.b1), _dev32(P.b2)
        ow2, pw2 = _dev16(P.W2, dt)
        oc, pc = _dev32(torch.tensor(cmax)) if cmax is not None else (None, None)
        out = _Out((T * B + 3) * ldx)
        _ok(lib.mt_conv12_bn_relu_pool_dt(pm, pc, p1, pb1, pw2, pb2, out.ptr, ldx, B, n_mels, T, dt, st))
        out.check(_x_index(B, 64, Fo2, T, ldx), exp, _tdt(dt), f"conv12 B={B} n_mels={n_mels} T={T} dt={dt}")


# ------------------------------------------------------------------ MT_CONVG_WAVES=8: one fresh child process
WAVES8_LAYERS = ("fa", "rb2c2", "c32_128", "rb2c1")


def _child_waves8():
    assert _waves8()
    n, reached = 0, set()
    for layer in WAVES8_LAYERS:
        cache = {}
        for P, dt, relu, pool, mode in _settings_cases(layer):
            reached.add(_expect_inst(layer, pool=pool))
            _cg_run(P, dt, relu, pool, mode, cache=cache)
            n += 1
    P = _cg_problem("fa", 3, 19, 37, edge=True)
    reached.add(_expect_inst("fa", accum=1, want=(64, 128)))
    _cg_run(P, F16, 1, 1, "x8", accum=1)
    P = _real_case("fa", 80, 1, 1)
    _cg_run(P, F16, 1, 1, "x8")
    assert reached == {(32, 256, 8), (64, 128, 8), (32, 128, 8), (64, 64, 8)}, reached
    return n + 2


def test_eight_wave_tiles_in_a_child_process():
    """MT_CONVG_WAVES=8: the 16-wave instantiations in their 8-wave form, every setting, exact and with the sentinel check."""
    env = {k: v for k, v in os.environ.items() if k != "MT_CONVG_WAVES"}
    env["MT_CONVG_WAVES"] = "8"
    limit = 600
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "waves8"], capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the waves8 child did not finish in {limit} s; nothing further is started on the GPU.\n{(e.stdout or b'')[-3000:]}", returncode=3)
    if r.returncode < 0:
        pytest.exit(f"the waves8 child died on signal {-r.returncode}; nothing further is started on the GPU.\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}",
                    returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    m = re.fullmatch(r"conv child waves8: (\d+) cases exact", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) == len(WAVES8_LAYERS) * len(SETTINGS) + 2, r.stdout[-3000:]


# ------------------------------------------------------------------ coverage of the family
def test_every_instantiation_is_named_by_a_case():
    reached = set()
    for layer, (cfg, kcbn) in LAYERS.items():
        for pool in (0, 1):
            reached.add(_cg_inst(*cfg, pool=pool, waves8=False))        # test_conv_cl_every_setting
    reached.add(_cg_inst(*LAYERS["fa"][0], accum=1, waves8=False))
    reached.add(_cg_inst(*LAYERS["fa"][0], tie=1, waves8=False))
    for layer in WAVES8_LAYERS:
        reached.add(_cg_inst(*LAYERS[layer][0], waves8=True))           # the child process
    assert reached == ALL_INSTANTIATIONS, (sorted(ALL_INSTANTIATIONS - reached), sorted(reached - ALL_INSTANTIATIONS))
    assert _cg_lds(128, 128, 3, 32, 128) == 164864                      # why 128 + 128 -> 128 runs on 64-channel tiles


def test_every_conv_export_is_called():
    from music_transcription_amd import _lib
    exported = {n for n in _lib.EXPORTS if re.match(r"mt_conv(_cl|1_bn|2_bn|12_bn)", n)}
    with open(os.path.abspath(__file__)) as f:
        called = set(re.findall(r"lib\.(mt_conv\w+)\(", f.read()))
    assert len(exported) == 9
    assert called == exported, (sorted(exported - called), sorted(called - exported))


# ------------------------------------------------------------------ the reference half alone (no GPU), and the child process
def _cpu_reference_half():
    """Builds every case's operands and reference and runs its representability / non-zero-share asserts."""
    n = 0
    for layer in LAYERS:
        n += sum(1 for _ in _settings_cases(layer)) + sum(1 for _ in _shape_cases(layer))
    for layer, F, relu, pool, mode, dt in REAL:
        _cg_expected(_real_case(layer, F, relu, pool), dt, relu, pool); n += 1
    for layer in ("fa", "rb1c1", "c32_128", "dgrad_rb2"):
        P = _cg_problem(layer, 3, 19, 37, edge=True)
        for dt, pool, relu in ((BF16, 0, 0), (F16, 1, 1), (BF16, 1, 1), (F16, 0, 0)):
            Fo = 9 if pool else 19
            _cg_expected(P, dt, relu, pool, _ints(torch.Generator().manual_seed(19 + 37), (3, P.Cout, Fo, 37), -8, 8)); n += 1
    for P, accum, want in _slice_cases():
        prev = _ints(torch.Generator().manual_seed(P.F + P.T), (P.B, P.Cout, P.F, P.T), -8, 8) if accum else None
        _cg_expected(P, BF16, 0, 0, prev); n += 1
    for P in _transposed_cases():
        _cg_expected(P, BF16, 0, 0); n += 1
    for P, dt in _rounding_cases():
        _cg_expected(P, dt, 0, 0), _cg_expected(P, dt, 0, 1); n += 1
    for layer, B, F, T, inst in TIE:
        _tie_reference(_cg_problem(layer, B, F, T, seed=9, edge=layer in TIE_EDGE)); n += 1
    for B, n_mels, T, cmax in CONV1:
        P = _c1_problem(B, n_mels, T, cmax)
        _c1_expected(P, BF16), _c1_expected(P, F16); n += 1
    for B, F1, T, pad in CONV2:
        P = _cg_problem("rb1c1", B, F1, T, seed=20, edge=F1 <= 33)
        _c2_expected(P, F16), _c2_expected(P, BF16); n += 1
    for B, n_mels, T, cmax in CONV12:
        P = _c12_problem(B, n_mels, T, cmax)
        _c12_expected(P, F16), _c12_expected(P, BF16); n += 1
    return n


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "cpu":
        print(f"conv reference half: {_cpu_reference_half()} cases representable and non-trivial")
    else:
        assert sys.argv[1] == "waves8"
        count = _child_waves8()
        torch.cuda.synchronize()
        print(f"conv child waves8: {count} cases exact")
