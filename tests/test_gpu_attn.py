"""The attention, LayerNorm and head kernels of csrc/attn.hip, csrc/attn_fused.hip and csrc/train_large.hip, one by one through the C ABI
against float64 references.

  mt_attn_transpose_v, mt_transpose_bf16_batched, mt_f32_to_bf16_rows, mt_heads_relu_dropout_bwd, the dropout kernels' masks:   EXACT (==)
  mt_attn_fused_clamped, mt_attn_softmax_clamped_dt, mt_attn_softmax_train, mt_attn_clamped_bwd,
  mt_layernorm_residual_dt / _train / _bwd:   float64 (autograd for the backward kernels) within per-element bounds from tests/attn_ref.py
  mt_axpby_rows_f32, dropout values at p = 0.3:   a stated number of ulps

Inputs, references and bounds come from tests/attn_ref.py (CPU only; tests/test_attn_ref_cpu.py checks them, and that each planted mutation
breaks a bound, without a GPU); DESIGN 6i holds the derivations.  Harness, as in tests/test_gpu_train_cnn.py: every output lies in a
sentinel-filled buffer between two guard bands and everything the contract does not write must still hold the sentinel afterwards; every
input is sized exactly between NaN bands, and pad columns of wide rows and regions the contract leaves unread hold NaN.

Every test prints the figure it is about to assert (`-s` shows them).  Run only this file:  python -m pytest tests/test_gpu_attn.py -q -m gpu
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1024                               # elements of guard band on either side of every buffer
NAN = float("nan")
F64 = torch.float64
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_SENT = {2: 0x7BCD, 4: 0x7FC0BEEF, 8: 0x7FF8DEADBEEF1234}      # 16 bits: bf16 2e36 / f16 63904; an f32 NaN; an f64 NaN
SENT16 = 0x7BCD
MT_EINVAL, MT_EUNSUPPORTED = -1, -4
DT = {"f16": 1, "bf16": 0}                 # MT_DT_* of include/mt_hip.h
AXPBY_ULPS = 2                             # alpha a + beta b: the compiler may contract the expression to an fma (one rounding instead of two)
DROPOUT_ULPS = 1                           # x / (1 - p) for p = 0.3: the rounded factor 1/(1-p) and the product, against one rounding of the quotient


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


def _lib():
    from music_transcription_amd._lib import lib, stream_ptr
    return lib, stream_ptr()


def _ok(rc):
    if rc != 0:
        from music_transcription_amd._lib import last_error
        raise AssertionError(f"call failed (code {rc}): {last_error()}")


def _in(body, dtype):
    """An input on the device: `body` between two NaN bands, sized exactly -> (owner, address of the body)"""
    g = torch.full((GUARD,), NAN, dtype=F64)
    full = torch.cat([g.to(dtype), body.reshape(-1).to(dtype), g.to(dtype)]).cuda()
    return full, full.data_ptr() + GUARD * full.element_size()


def _in_words(words):
    """16-bit words as they are, between two bands of bf16 NaN words"""
    g = torch.full((GUARD,), 0x7FC0, dtype=torch.int16)
    full = torch.cat([g, torch.as_tensor(np.ascontiguousarray(words)).reshape(-1), g]).cuda()
    return full, full.data_ptr() + 2 * GUARD


def _rows(v, ld, fill=NAN):
    """v [rows][n] -> storage [rows][ld] with `fill` in the pad columns, cut after the last row's n-th element (sized exactly)"""
    rows, n = v.shape
    body = torch.full((rows, ld), fill, dtype=v.dtype)
    body[:, :n] = v
    return body.reshape(-1)[:(rows - 1) * ld + n]


class _Out:
    """n elements of `size` bytes between two guard bands, all of it pre-filled with a sentinel (the body too)"""

    def __init__(self, n, dtype):
        self.n, self.dtype, self.size = n, dtype, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((2 * GUARD + n,), _SENT[self.size], dtype=_INT[self.size], device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.size

    def preset(self, values):
        self.buf[GUARD:GUARD + self.n] = values.reshape(-1).to(self.dtype).view(_INT[self.size]).cuda()

    def preset_words(self, words, idx):
        """words at the body positions idx; the rest keeps the sentinel"""
        self.buf[torch.as_tensor(np.ascontiguousarray(idx)).reshape(-1).cuda() + GUARD] = torch.as_tensor(np.ascontiguousarray(words)).reshape(-1).cuda()

    def body(self):
        return self.buf[GUARD:GUARD + self.n].cpu().view(self.dtype)

    def words(self):
        return self.buf[GUARD:GUARD + self.n].cpu()

    def untouched(self):
        return bool((self.buf == _SENT[self.size]).all().item())

    def rest_untouched(self, idx=None):
        """everything but the logical elements idx (positions in the body; None: the whole body) still holds the sentinel"""
        other = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        if idx is None:
            other[GUARD:GUARD + self.n] = False
        else:
            pos = torch.as_tensor(np.ascontiguousarray(idx)).reshape(-1)
            assert pos.numel() == 0 or (int(pos.min()) >= 0 and int(pos.max()) < self.n)
            other[pos.cuda() + GUARD] = False
            assert int((~other).sum()) == pos.numel(), "the layout maps two logical elements to one slot"
        return bool((self.buf[other] == _SENT[self.size]).all().item())


def _say(what, **figs):
    print(f"MEASURED {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _ratio(err, bound):
    """largest err / bound; an element with bound 0 must have err 0"""
    assert bool((err[bound == 0] == 0).all()), "an element whose bound is zero differs from the reference"
    return float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def _as16(body16, dt):
    return body16.view(R.TDT[dt]).to(F64)


# ================================================================== 1. mt_attn_transpose_v, exact
@pytest.mark.parametrize("B,T,Tp,heads,dp,use", R.TRANSPOSE_V_CASES)
def test_attn_transpose_v_exact(mta, B, T, Tp, heads, dp, use):
    """VT[(b heads + head)][d][t] == qkv[(t B + b) ld3 + voff + head dp + d] for d < dp, t < T, zero for T <= t < Tp; rows dp .. dpr-1 of every
    slab keep the sentinel.  The words encode the position; everything of qkv outside the V block is NaN."""
    lib, st = _lib()
    P = R.transpose_v_case(B, T, Tp, heads, dp, use)
    qkv = np.full((T, B, P.ld3), 0x7FC0, dtype=np.int16)
    qkv[:, :, P.voff:P.voff + heads * dp] = P.words.reshape(T, B, heads * dp)
    body = qkv.reshape(-1)[:(T * B - 1) * P.ld3 + P.voff + heads * dp]
    oq, pq = _in_words(body)
    VT = _Out(B * heads * P.dpr * Tp, torch.bfloat16)
    _ok(lib.mt_attn_transpose_v(pq, P.ld3, P.voff, VT.ptr, B, T, Tp, heads, dp, st))
    torch.cuda.synchronize()
    got = VT.words().numpy().reshape(B, heads, P.dpr, Tp)
    bad = np.argwhere(got[:, :, :dp, :] != P.want)
    _say(f"transpose_v {B}x{T}x{heads}x{dp} {use}", differing=len(bad))
    assert len(bad) == 0, f"first at (b, head, d, t) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {P.want[tuple(bad[0])]}"
    assert bool((got[:, :, dp:, :] == SENT16).all()), "rows dp .. dpr-1 of a slab were written"
    assert VT.rest_untouched()


# ================================================================== 2. mt_attn_fused_clamped
def _fused_buffers(P):
    """qkv [(t B + b)][ld3] with NaN outside the three blocks, sized exactly; VT [B heads][dpr][Tp]: zero for t >= T, NaN in rows dp .. dpr-1"""
    T, B, H, dp = P.T, P.B, P.heads, P.dp
    qkv = torch.full((T, B, P.ld3), NAN, dtype=F64)
    for i, x in enumerate((P.q, P.k, P.v)):
        qkv[:, :, i * P.Ca:i * P.Ca + H * dp] = x.reshape(T, B, H * dp)
    body = qkv.reshape(-1)[:(T * B - 1) * P.ld3 + 2 * P.Ca + H * dp]
    vt = torch.full((B, H, P.dpr, P.Tp), NAN, dtype=F64)
    vt[:, :, :dp, :] = 0.0
    vt[:, :, :dp, :T] = P.v.permute(1, 2, 3, 0)
    return body, vt


def _fused_call(P, body, vt):
    lib, st = _lib()
    tdt = R.TDT[P.dt]
    oq, pq = _in(body, tdt)
    ov, pv = _in(vt, tdt)
    ao = _Out(P.T * P.B * P.ldo, torch.bfloat16)
    _ok(lib.mt_attn_fused_clamped(pq, P.ld3, P.Ca, pv, P.Tp, P.B, P.T, P.heads, P.dp, P.scale, P.clip, ao.ptr, P.ldo, DT[P.dt], st))
    torch.cuda.synchronize()
    return ao


@pytest.mark.parametrize("dt,dp,T,B,heads", R.fused_cases())
def test_attn_fused_clamped_within_bound_of_float64(mta, dt, dp, T, B, heads):
    """Every output element within R.fused_bound of the float64 softmax(clamp(q k^T scale)) v on the same 16-bit q, k, v.  The inputs are such
    that leaving any one key out of a row moves an output of that row by more than its bound (asserted here for the rows the CPU tests
    sample), so a lost, duplicated or misplaced key cannot hide.  Query rows t >= T do not exist in `ao` (it has T B rows): pad columns
    and guard bands keep the sentinel; two runs are bitwise equal."""
    P = R.fused_case(dt, dp, T, B, heads)
    if T > 1:
        vis = R.fused_key_visibility(P, R.fused_sample_rows(T) if T > 65 else [0, T // 2, T - 1])
        assert vis > 1, f"a key's absence would move no output by more than the bound ({vis:.3g})"
    body, vt = _fused_buffers(P)
    ao = _fused_call(P, body, vt)
    t, b, c = np.ogrid[:T, :B, :heads * dp]
    idx = (t * B + b) * P.ldo + c
    got = _as16(ao.body(), dt)[torch.from_numpy(idx.reshape(-1))].reshape(T, B, heads, dp).permute(1, 2, 0, 3)
    assert bool(torch.isfinite(got).all()), "a NaN of rows dp .. dpr-1 of VT, of a pad column or of a band reached a result"
    r = _ratio((got - P.ref).abs(), R.fused_bound(P))
    _say(f"attn_fused {dt} dp={dp} T={T} B={B} heads={heads}", err_over_bound=r)
    assert r <= 1, f"an output is {r:.3g} times its bound away from float64"
    assert ao.rest_untouched(idx), "a pad column of ao or a guard band was written"
    again = _fused_call(P, body, vt)
    assert torch.equal(again.buf, ao.buf), "two runs differ"


def test_attn_fused_clamped_rows_past_T_keep_the_sentinel(mta):
    """ao with more rows than T (the caller's buffer holds a longer window): the rows t >= T keep the sentinel, for a T inside a query block"""
    lib, st = _lib()
    P = R.fused_case("f16", 64, 40, 3, 1)
    body, vt = _fused_buffers(P)
    oq, pq = _in(body, torch.float16)
    ov, pv = _in(vt, torch.float16)
    ao = _Out(64 * P.B * P.ldo, torch.bfloat16)
    _ok(lib.mt_attn_fused_clamped(pq, P.ld3, P.Ca, pv, P.Tp, P.B, P.T, P.heads, P.dp, P.scale, P.clip, ao.ptr, P.ldo, DT["f16"], st))
    torch.cuda.synchronize()
    t, b, c = np.ogrid[:P.T, :P.B, :P.heads * P.dp]
    assert ao.rest_untouched((t * P.B + b) * P.ldo + c)


@pytest.mark.parametrize("what,code", [("dp96", MT_EUNSUPPORTED), ("ld3", MT_EINVAL), ("misaligned", MT_EINVAL), ("clip", MT_EINVAL), ("Tp", MT_EINVAL)])
def test_attn_fused_clamped_refuses(mta, what, code):
    """each bad argument returns its error code and leaves the output as it was"""
    lib, st = _lib()
    P = R.fused_case("bf16", 128, 40, 1, 1)
    body, vt = _fused_buffers(P)
    oq, pq = _in(body, torch.bfloat16)
    ov, pv = _in(vt, torch.bfloat16)
    ao = _Out(P.T * P.B * P.ldo, torch.bfloat16)
    a = dict(qkv=pq, ld3=P.ld3, Ca=P.Ca, VT=pv, Tp=P.Tp, dp=P.dp, clip=P.clip)
    if what == "dp96":
        a.update(dp=96, Ca=96, ld3=3 * 96)           # (sizes that fit the same buffers and ldo: only the head size is at fault)
    elif what == "ld3":
        a.update(ld3=P.ld3 + 4)
    elif what == "misaligned":
        a.update(qkv=pq + 2)
    elif what == "clip":
        a.update(clip=10.5)
    else:
        a.update(Tp=P.Tp + 32)
    rc = lib.mt_attn_fused_clamped(a["qkv"], a["ld3"], a["Ca"], a["VT"], a["Tp"], P.B, P.T, P.heads, a["dp"], P.scale, a["clip"], ao.ptr, P.ldo, DT["bf16"], st)
    torch.cuda.synchronize()
    _say(f"attn_fused refuses {what}", rc=rc)
    assert rc == code
    assert ao.untouched()


# ================================================================== 3. unfused softmax
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rows,T,extra", R.SOFTMAX_SHAPES)
def test_attn_softmax_clamped_dt_within_bound(mta, rows, T, extra, dt):
    lib, st = _lib()
    P = R.softmax_case(rows, T, extra)
    ref = R.softmax_reference(P)
    oS, pS = _in(_rows(P.S, P.lds), torch.float32)
    out = _Out(rows * P.Tp, torch.bfloat16)
    _ok(lib.mt_attn_softmax_clamped_dt(pS, P.lds, out.ptr, P.Tp, T, rows, P.scale, P.clip, DT[dt], st))
    torch.cuda.synchronize()
    got = _as16(out.body(), dt).reshape(rows, P.Tp)
    r = _ratio((got[:, :T] - ref).abs(), R.softmax_fwd_bound(P, ref, dt))
    _say(f"softmax_clamped {dt} rows={rows} T={T} Tp={P.Tp}", err_over_bound=r)
    assert r <= 1
    assert bool((out.words().reshape(rows, P.Tp)[:, T:] == 0).all()), "columns T .. Tp-1 are not exactly zero"
    assert out.rest_untouched()


@pytest.mark.parametrize("p", R.SOFTMAX_PS)
@pytest.mark.parametrize("rows,T,extra", R.SOFTMAX_SHAPES)
def test_attn_softmax_train_mask_and_values(mta, rows, T, extra, p):
    """the zero pattern == dropout_keep(seed, layer, row T + j, p) of the host replica (T != Tp in every case), the kept values within the
    bound of ref / (1 - p); another (seed, layer) gives another mask"""
    lib, st = _lib()
    P = R.softmax_case(rows, T, extra)
    assert P.Tp != T
    ref = R.softmax_reference(P)
    oS, pS = _in(_rows(P.S, P.lds), torch.float32)
    masks = []
    for seed, layer in ((7, 3), (8, 3), (7, 4)):
        out = _Out(rows * P.Tp, torch.bfloat16)
        _ok(lib.mt_attn_softmax_train(pS, P.lds, out.ptr, P.Tp, T, rows, P.scale, P.clip, p, seed, layer, st))
        torch.cuda.synchronize()
        got = _as16(out.body(), "bf16").reshape(rows, P.Tp)
        keep = R.softmax_keep(P, p, seed, layer) if p > 0 else torch.ones((rows, T), dtype=torch.bool)
        want = ref * keep / (1 - p)
        assert torch.equal(got[:, :T] != 0, keep), "the zero pattern is not dropout_keep(seed, layer, row*T + j, p)"
        r = _ratio((got[:, :T] - want).abs(), R.softmax_fwd_bound(P, want, "bf16", p))
        _say(f"softmax_train rows={rows} T={T} Tp={P.Tp} p={p} seed={seed} layer={layer}", err_over_bound=r, kept=float(keep.double().mean()))
        assert r <= 1
        assert bool((out.words().reshape(rows, P.Tp)[:, T:] == 0).all()) and out.rest_untouched()
        masks.append(keep)
    if p > 0 and rows * T >= 63:
        assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2])


def _softmax_bwd(P, p, seed=7, layer=3):
    lib, st = _lib()
    oS, pS = _in(_rows(P.S, P.lds), torch.float32)
    oG, pG = _in(_rows(P.dP, P.ldp), torch.float32)
    out = _Out(P.rows * P.Tp, torch.bfloat16)
    _ok(lib.mt_attn_clamped_bwd(pS, P.lds, pG, P.ldp, out.ptr, P.Tp, P.T, P.rows, P.scale, P.clip, p, seed, layer, st))
    torch.cuda.synchronize()
    assert bool((out.words().reshape(P.rows, P.Tp)[:, P.T:] == 0).all()) and out.rest_untouched()
    return _as16(out.body(), "bf16").reshape(P.rows, P.Tp)[:, :P.T]


@pytest.mark.parametrize("p", R.SOFTMAX_PS)
@pytest.mark.parametrize("rows,T,extra", R.SOFTMAX_SHAPES)
def test_attn_clamped_bwd_against_float64_autograd(mta, rows, T, extra, p):
    P = R.softmax_case(rows, T, extra)
    R.assert_clip_separated(P)
    keep = R.softmax_keep(P, p, 7, 3) if p > 0 else torch.ones((rows, T), dtype=torch.bool)
    ref = R.softmax_bwd_reference(P, p, keep)
    got = _softmax_bwd(P, p)
    r = _ratio((got - ref).abs(), R.softmax_bwd_bound(P, ref, p, keep))
    _say(f"attn_clamped_bwd rows={rows} T={T} Tp={P.Tp} p={p}", err_over_bound=r)
    assert r <= 1


def test_attn_clamped_bwd_clamp_edge_is_inclusive(mta):
    """scale = 0.25 (exact products), clip = 10: entries at S = +-40 pass the gradient as torch.clamp does, entries at nextafter(+-40, +-inf)
    get exactly 0"""
    P = R.softmax_case(5, 65, 0, scale=0.25, clip=10.0, edge=True)
    R.assert_clip_separated(P)
    keep = torch.ones((5, 65), dtype=torch.bool)
    ref = R.softmax_bwd_reference(P, 0.0, keep)
    bound = R.softmax_bwd_bound(P, ref, 0.0, keep)
    assert bool((ref[0, :2].abs() > 2 * bound[0, :2]).all()) and bool((ref[0, 2:4] == 0).all())
    got = _softmax_bwd(P, 0.0)
    r = _ratio((got - ref).abs(), bound)
    _say("attn_clamped_bwd clamp edge", err_over_bound=r, at_edge=got[0, :4].tolist())
    assert r <= 1
    assert bool((got[0, 2:4] == 0).all()) and bool((got[0, :2] != 0).all())


# ================================================================== 4. LayerNorm(resid + proj)
def _ln_inputs(P):
    return [_in(_rows(P.resid, P.ldr), torch.float32), _in(_rows(P.proj, P.ldp), torch.float32), _in(P.gamma, torch.float32), _in(P.beta, torch.float32)]


def _ln_check(P, y, dt, what):
    n, rows = P.n, P.rows
    got = _as16(y.body(), dt).reshape(rows, P.ldy)[:, :n]
    r = _ratio((got - P.y).abs(), R.ln_fwd_bound(P, dt))
    _say(what, err_over_bound=r)
    assert r <= 1
    if n == 1:
        assert torch.equal(got[:, 0], R.r16(P.beta, dt).expand(rows)), "n = 1 must give beta, rounded"
    m, c = np.ogrid[:rows, :n]
    assert y.rest_untouched(m * P.ldy + c), "a pad column of y or a guard band was written"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("n", R.LN_NS)
def test_layernorm_residual_dt_within_bound(mta, n, rows, dt):
    lib, st = _lib()
    P = R.ln_case(rows, n)
    ins = _ln_inputs(P)
    y = _Out(rows * P.ldy, torch.bfloat16)
    _ok(lib.mt_layernorm_residual_dt(ins[0][1], P.ldr, ins[1][1], P.ldp, ins[2][1], ins[3][1], y.ptr, P.ldy, rows, n, P.eps, DT[dt], st))
    torch.cuda.synchronize()
    _ln_check(P, y, dt, f"layernorm_residual {dt} rows={rows} n={n}")


@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("n", R.LN_NS)
def test_layernorm_residual_train_within_bound_and_stats(mta, n, rows):
    """y as above; stats[row] = {mean, rstd} within R.ln_stats_ulps f32 ulps of float64 (the numbers are printed)"""
    lib, st = _lib()
    P = R.ln_case(rows, n)
    ins = _ln_inputs(P)
    y, stats = _Out(rows * P.ldy, torch.bfloat16), _Out(2 * rows, torch.float32)
    _ok(lib.mt_layernorm_residual_train(ins[0][1], P.ldr, ins[1][1], P.ldp, ins[2][1], ins[3][1], y.ptr, P.ldy, stats.ptr, rows, n, P.eps, st))
    torch.cuda.synchronize()
    _ln_check(P, y, "bf16", f"layernorm_residual_train rows={rows} n={n}")
    s = stats.body().numpy().reshape(rows, 2)
    um, ur = R.ln_stats_ulps(P)
    gm, gr = R.ulps32(s[:, 0], P.mean.reshape(-1).numpy()), R.ulps32(s[:, 1], P.rstd.reshape(-1).numpy())
    _say(f"layernorm stats rows={rows} n={n}", mean_ulp=float(gm.max()), mean_allowed=float(um.min()), rstd_ulp=float(gr.max()), rstd_allowed=float(ur.min()))
    assert bool((torch.from_numpy(gm) <= um).all()) and bool((torch.from_numpy(gr) <= ur).all())
    assert stats.rest_untouched()


def test_layernorm_residual_refuses_n_2049(mta):
    lib, st = _lib()
    P = R.ln_case(1, 2048)
    ins = _ln_inputs(P)
    for dt in ("f16", "bf16"):
        y = _Out(2100, torch.bfloat16)
        assert lib.mt_layernorm_residual_dt(ins[0][1], 2049, ins[1][1], 2049, ins[2][1], ins[3][1], y.ptr, 2049, 1, 2049, P.eps, DT[dt], st) == MT_EINVAL
        torch.cuda.synchronize()
        assert y.untouched()
    y, stats = _Out(2100, torch.bfloat16), _Out(2, torch.float32)
    assert lib.mt_layernorm_residual_train(ins[0][1], 2049, ins[1][1], 2049, ins[2][1], ins[3][1], y.ptr, 2049, stats.ptr, 1, 2049, P.eps, st) == MT_EINVAL
    torch.cuda.synchronize()
    assert y.untouched() and stats.untouched()


@pytest.mark.parametrize("rows,n", R.LN_BWD_SHAPES)
def test_layernorm_residual_bwd_against_float64_autograd(mta, rows, n):
    """stats come from the float64 reference rounded to f32: the kernel alone.  All slices x 2 x n elements of `part` are written (zeros from
    waves without a row included: the buffer starts as the sentinel, an f32 NaN); their float64 sum over the slices meets dgamma and dbeta."""
    lib, st = _lib()
    P = R.ln_case(rows, n, big_mean=False)
    slices = lib.mt_layernorm_residual_bwd_slices()
    assert slices == R.LN_SLICES
    dx_ref, dg_ref, db_ref = R.ln_bwd_reference(P)
    b_dx, b_dg, b_db = R.ln_bwd_bounds(P)
    ins = _ln_inputs(P)
    ostat, pstat = _in(torch.stack([P.mean.reshape(-1), P.rstd.reshape(-1)], 1), torch.float32)
    ldd, ldx = n + 4, n + 5
    ody, pdy = _in(_rows(P.dy, ldd), torch.float32)
    dx, part = _Out(rows * ldx, torch.float32), _Out(slices * 2 * n, torch.float32)
    _ok(lib.mt_layernorm_residual_bwd(ins[0][1], P.ldr, ins[1][1], P.ldp, ins[2][1], pstat, pdy, ldd, dx.ptr, ldx, part.ptr, rows, n, st))
    torch.cuda.synchronize()
    pw = part.body().to(F64).reshape(slices, 2, n)
    assert bool(torch.isfinite(pw).all()), "an element of part was not written"
    if rows < slices:
        assert bool((pw[rows:] == 0).all())
    got = dx.body().to(F64).reshape(rows, ldx)[:, :n]
    figs = dict(dx=_ratio((got - dx_ref).abs(), b_dx), dgamma=_ratio((pw[:, 0].sum(0) - dg_ref).abs(), b_dg),
                dbeta=_ratio((pw[:, 1].sum(0) - db_ref).abs(), b_db))
    _say(f"layernorm_residual_bwd rows={rows} n={n}", **figs)
    assert max(figs.values()) <= 1
    m, c = np.ogrid[:rows, :n]
    assert dx.rest_untouched(m * ldx + c) and part.rest_untouched()


# ================================================================== 5. element-wise and layout helpers
@pytest.mark.parametrize("R_,C", R.TRANSPOSE_RC)
def test_transpose_bf16_batched_exact(mta, R_, C):
    """dst[z][c ldd + r] == src[z][r lds + c]; every dst element with c < Cd, r < ldd is written, zero outside r < R, c < C; the gaps between
    the batch's slabs keep the sentinel (dst) and hold NaN (src)"""
    lib, st = _lib()
    batch, lds, ldd, Cd = 3, C + 3, R_ + 5, C + 2
    sstride, dstride = R_ * lds + 11, Cd * ldd + 13
    words = np.stack([R.position_words(R_, C) + z for z in range(batch)]).astype(np.int16)
    src = np.full((batch, sstride), 0x7FC0, dtype=np.int16)
    r, c = np.ogrid[:R_, :C]
    src[:, (r * lds + c).reshape(-1)] = words.reshape(batch, -1)
    body = src.reshape(-1)[:(batch - 1) * sstride + (R_ - 1) * lds + C]
    osrc, psrc = _in_words(body)
    dst = _Out((batch - 1) * dstride + Cd * ldd, torch.bfloat16)
    _ok(lib.mt_transpose_bf16_batched(psrc, lds, sstride, R_, C, dst.ptr, ldd, dstride, Cd, batch, st))
    torch.cuda.synchronize()
    want = np.zeros((batch, Cd, ldd), dtype=np.int16)
    want[:, :C, :R_] = words.transpose(0, 2, 1)
    z, cc, rr = np.ogrid[:batch, :Cd, :ldd]
    idx = z * dstride + cc * ldd + rr
    got = dst.words().numpy()[idx.reshape(-1)].reshape(batch, Cd, ldd)
    bad = np.argwhere(got != want)
    _say(f"transpose_bf16_batched R={R_} C={C}", differing=len(bad))
    assert len(bad) == 0, f"first at (z, c, r) = {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    assert dst.rest_untouched(idx)


@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0])
@pytest.mark.parametrize("M,N,ld", R.ELEMENTWISE_SHAPES)
def test_f32_to_bf16_rows_bit_exact(mta, M, N, ld, alpha):
    """dst == torch's round-to-nearest-even bf16 of alpha src, bit for bit: a third of the inputs on ties, a third one f32 step beside one;
    +-inf, the canonical quiet NaN, +-FLT_MAX, denormals and zeros at the start"""
    lib, st = _lib()
    src = R.tie_words_f32(M * N, seed=M + N)
    k = min(len(R.SPECIALS_F32), M * N)
    src[:k] = torch.tensor(R.SPECIALS_F32[:k], dtype=torch.float32)
    src = src.reshape(M, N)
    lds, ldd = ld + 1, ld + 3
    osrc, psrc = _in(_rows(src, lds), torch.float32)
    dst = _Out((M - 1) * ldd + N, torch.bfloat16)
    _ok(lib.mt_f32_to_bf16_rows(psrc, lds, dst.ptr, ldd, M, N, alpha, st))
    torch.cuda.synchronize()
    idx = R.rows_index(M, N, ldd)
    got = dst.body()[torch.from_numpy(idx.reshape(-1))].reshape(M, N)
    want = R.f32_to_bf16_reference(src, alpha)
    same = (R.bf16_bits(got) == R.bf16_bits(want)) | (torch.isnan(got) & torch.isnan(want))
    _say(f"f32_to_bf16_rows {M}x{N} alpha={alpha}", differing=int((~same).sum()))
    assert bool(same.all())
    assert dst.rest_untouched(idx)


@pytest.mark.parametrize("p", [0.5, 0.75])
@pytest.mark.parametrize("M,N,ld", R.ELEMENTWISE_SHAPES)
def test_heads_relu_dropout_bwd_exact(mta, M, N, ld, p):
    """dZ == bf16(dY / (1 - p)) where Y > 0, else +0: Y takes +0, -0, the smallest positive bf16, negative and positive numbers; 1 / (1 - p)
    is a power of two, so the product is exact and the bf16 rounding is torch's"""
    lib, st = _lib()
    g = torch.Generator().manual_seed(M + N)
    pool = torch.tensor([0x0000, 0x8000, 0x0001, 0xBF80, 0x3F80, 0x8001, 0x4049, 0xC2C8], dtype=torch.int32).to(torch.int16)
    Yw = pool[torch.randint(0, 8, (M, N), generator=g)]
    Y = Yw.view(torch.bfloat16)
    dY = R.tie_words_f32(M * N, seed=5 + M).reshape(M, N)
    ldd, ldy, ldz = ld + 1, ld + 2, ld + 4
    odY, pdY = _in(_rows(dY, ldd), torch.float32)
    yb = np.full((M, ldy), 0x7FC0, dtype=np.int16)
    yb[:, :N] = Yw.numpy()
    oY, pY = _in_words(yb.reshape(-1)[:(M - 1) * ldy + N])
    dZ = _Out((M - 1) * ldz + N, torch.bfloat16)
    _ok(lib.mt_heads_relu_dropout_bwd(pdY, ldd, pY, ldy, dZ.ptr, ldz, M, N, p, st))
    torch.cuda.synchronize()
    idx = R.rows_index(M, N, ldz)
    got = dZ.body()[torch.from_numpy(idx.reshape(-1))].reshape(M, N)
    want = torch.where(Y.float() > 0, dY * (1.0 / (1.0 - p)), torch.zeros_like(dY)).to(torch.bfloat16)
    nd = int((R.bf16_bits(got) != R.bf16_bits(want)).sum())
    _say(f"heads_relu_dropout_bwd {M}x{N} p={p}", differing=nd, on=float((Y.float() > 0).double().mean()))
    assert nd == 0
    assert dZ.rest_untouched(idx)


def _dropout_expect(x, keep, p):
    """inverted dropout in float64 (exact for p = 0.5, 0.75) of the values x"""
    return torch.where(torch.from_numpy(keep), x.to(F64) / (1 - float(np.float32(p))), torch.zeros_like(x, dtype=F64))


@pytest.mark.parametrize("p", [0.0, 0.3, 0.5, 0.75])
@pytest.mark.parametrize("M,N,ld", R.ELEMENTWISE_SHAPES)
def test_dropout_bf16_rows_mask_and_values(mta, M, N, ld, p):
    """in place on [M][ld]: element (m, n) keeps with dropout_keep(seed, layer, m N + n, p) -- not m ld + n; the values are small non-zero
    integers (x / (1 - p) is a bf16 value for p = 0.5, 0.75: ==; p = 0.3: within DROPOUT_ULPS bf16 ulps); pad columns keep the sentinel;
    p = 0 leaves the buffer bitwise unchanged"""
    lib, st = _lib()
    ld = ld + 3
    g = torch.Generator().manual_seed(M * 3 + N)
    x = (torch.randint(1, 16, (M, N), generator=g) * (torch.randint(0, 2, (M, N), generator=g) * 2 - 1)).to(torch.bfloat16)
    X = _Out((M - 1) * ld + N, torch.bfloat16)
    idx = R.rows_index(M, N, ld)
    X.preset_words(R.bf16_bits(x).numpy(), idx)
    before = X.buf.clone()
    _ok(lib.mt_dropout_bf16_rows(X.ptr, ld, M, N, p, 11, 5, st))
    torch.cuda.synchronize()
    if p == 0.0:
        assert torch.equal(X.buf, before)
        return
    got = X.body()[torch.from_numpy(idx.reshape(-1))].reshape(M, N)
    keep = R.dropout_rows_keep(M, N, p, 11, 5)
    assert torch.equal(got != 0, torch.from_numpy(keep)), "the zero pattern is not dropout_keep(seed, layer, m*N + n, p)"
    want = _dropout_expect(x, keep, p)
    u = float(R.ulps16(got, want, "bf16").max())
    _say(f"dropout_bf16_rows {M}x{N} p={p}", kept=float(keep.mean()), ulps=u)
    assert u == 0 if p in (0.5, 0.75) else u <= DROPOUT_ULPS
    assert X.rest_untouched(idx)


@pytest.mark.parametrize("p", [0.0, 0.3, 0.5, 0.75])
@pytest.mark.parametrize("n", R.DROPOUT_F32_NS)
def test_dropout_f32_mask_and_values(mta, n, p):
    lib, st = _lib()
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    X = _Out(n, torch.float32)
    X.preset(x)
    before = X.buf.clone()
    _ok(lib.mt_dropout_f32(X.ptr, n, p, 12, 6, st))
    torch.cuda.synchronize()
    if p == 0.0:
        assert torch.equal(X.buf, before)
        return
    got = X.body()
    keep = R.dropout_keep(12, 6, np.arange(n, dtype=np.int64), p)
    assert torch.equal(got != 0, torch.from_numpy(keep)), "the zero pattern is not dropout_keep(seed, layer, i, p)"
    u = float(R.ulps32(got.numpy(), _dropout_expect(x, keep, p).numpy()).max())
    _say(f"dropout_f32 n={n} p={p}", kept=float(keep.mean()), ulps=u)
    assert u == 0 if p in (0.5, 0.75) else u <= DROPOUT_ULPS
    assert X.rest_untouched()


@pytest.mark.parametrize("p", [0.0, 0.3, 0.5, 0.75])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 65), (5, 256)])
def test_dropout2d_mask_pattern(mta, B, C, p):
    """mask[b C + c] = 1 / (1 - p) where dropout_keep(seed, layer, b C + c, p), else 0; p = 0: all ones"""
    lib, st = _lib()
    mask = _Out(B * C, torch.float32)
    _ok(lib.mt_dropout2d_mask(mask.ptr, B, C, p, 13, 2, st))
    torch.cuda.synchronize()
    got = mask.body()
    keep = R.dropout_keep(13, 2, np.arange(B * C, dtype=np.int64), p) if p > 0 else np.ones(B * C, dtype=bool)
    assert torch.equal(got != 0, torch.from_numpy(keep))
    u = float(R.ulps32(got.numpy(), _dropout_expect(torch.ones(B * C), keep, p).numpy()).max())
    _say(f"dropout2d_mask {B}x{C} p={p}", kept=float(keep.mean()), ulps=u)
    assert u == 0 if p in (0.0, 0.5, 0.75) else u <= DROPOUT_ULPS
    assert mask.rest_untouched()


@pytest.mark.parametrize("alpha,beta,with_b", [(1.0, 1.0, True), (2.0, -0.5, True), (1.5, 7.0, False), (0.3, 1.7, True)])
@pytest.mark.parametrize("M,N,ld", R.ELEMENTWISE_SHAPES)
def test_axpby_rows_f32(mta, M, N, ld, alpha, beta, with_b):
    """out = alpha a + beta b into a buffer of its own.  (1, 1), (2, -0.5): == (the products are exact, one rounding either way);
    b = NULL: == alpha a, ldb ignored, no beta NaN; general alpha, beta: within AXPBY_ULPS f32 ulps of float64"""
    lib, st = _lib()
    g = torch.Generator().manual_seed(M + 2 * N)
    a, b = torch.randn((M, N), generator=g), torch.randn((M, N), generator=g)
    lda, ldb, ldo = ld + 1, ld + 2, ld + 3
    oa, pa = _in(_rows(a, lda), torch.float32)
    ob, pb = _in(_rows(b, ldb), torch.float32) if with_b else (None, None)
    out = _Out((M - 1) * ldo + N, torch.float32)
    _ok(lib.mt_axpby_rows_f32(pa, lda, pb, ldb if with_b else 0, out.ptr, ldo, M, N, alpha, NAN if not with_b else beta, st))
    torch.cuda.synchronize()
    idx = R.rows_index(M, N, ldo)
    got = out.body()[torch.from_numpy(idx.reshape(-1))].reshape(M, N)
    al, be = float(np.float32(alpha)), float(np.float32(beta))
    want = al * a.to(F64) + (be * b.to(F64) if with_b else 0.0)
    if with_b and (alpha, beta) == (0.3, 1.7):
        # within 2 ulps of the result unless the addends cancel: measure against the spacing at the larger addend
        scale = torch.maximum((al * a.to(F64)).abs(), (be * b.to(F64)).abs())
        u = float((np.abs(got.to(F64).numpy() - want.numpy()) / np.spacing(scale.to(torch.float32).numpy()).astype(np.float64)).max())
        _say(f"axpby_rows {M}x{N} alpha={alpha} beta={beta}", ulps=u)
        assert u <= AXPBY_ULPS
    else:
        nd = int((got != want.to(torch.float32)).sum())
        _say(f"axpby_rows {M}x{N} alpha={alpha} beta={beta} b={'yes' if with_b else 'NULL'}", differing=nd)
        assert nd == 0
    assert out.rest_untouched(idx)
