"""Inference forwards under poisoned allocations (tests/alloc_fill.py): no logit may depend on what torch.empty returned.

Each case builds a fresh model (oracle.model_ref.make_state_dict weights), runs ONE forward with check_status=True and returns the
logits and the hand-off status words; run_under_fills does that under 0x00 twice, 0xFF and 0x47, and the logits must agree bitwise
(the inference path has no atomics: the two control runs agree bitwise, which assert_fill_independent checks first) with every
status word 0.  What this pins, in csrc/model.hip and csrc/model_large.hip: the pad rows M..Mpad of x0 / x1 / rb / ln / sh / ao only
feed GEMM rows nobody reads; the pad COLUMNS of x1 (K1 > 2H), rb and ln (Cp > comb) and sh (Hs > H) are zeroed by the memsets that
run only when such columns exist; the qkv rows up to Tr * B and the P rows past T "only feed masked outputs"; V^T's frames T..Tp.

Shapes: every pad region of plan() / lplan() exists and differs in size from its live region --
  CNNRNNModel (n_mels, H, L, B, T)
    (38, 20, 2, 3, 21)  Hp = 32 > H, K1 = 64 > 2H (x1 memset runs), M = 63 -> Mpad = 128, n_mels // 2 odd
    (40, 32, 3, 5, 33)  M = 165 -> Mpad = 256, 2H = 64 = K1 (x1 memset skipped)
    (32, 64, 2, 2, 19)  f16 operands: the from_hx path (no re-layout, hx ping-pong, mt_gemm_logits_from_hx)
    (38, 20, 1, 3, 21)  one layer: x1's pad columns reach the fc GEMM alone (no recurrence between them and the logits)
  CNNRNNModelLarge
    (32, 16, 2, 3, 24)  comb = 48 -> Cp = 64, Hs = 64 > H
    (32, 24, 2, 2, 37)  Hp = 32 > H, Hl = 12 -> Hlp = 16, comb = 72 -> Cp = 128, Hs = 64 > H, T = 37 -> Tp = 64, Tr = 128
    (32, 520, 1, 2, 19) the UNFUSED attention core: head_dim = 3 H / 8 = 195 -> head_dim_pad = 256, outside {64, 128, 192}; the
                        smallest width the wrapper accepts that reaches it (head_dim > 192 with comb = 3 H a multiple of the
                        8 heads needs H >= 520; comb <= 2048 allows it)
The two-kernel convolution path (MT_CONV_FUSED=0) is read once per process and is left out; conv1 writes act1 whole
(test_gpu_conv.py, guard bands)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alloc_fill import BIG_FILL, NAN_FILL, alloc_fill, assert_fill_independent, run_under_fills
from oracle import model_ref as R
from test_gpu_train_autograd import _batch

SMALL_FWD = [(38, 20, 2, 3, 21), (40, 32, 3, 5, 33), (32, 64, 2, 2, 19), (38, 20, 1, 3, 21)]
LARGE_FWD = [(32, 16, 2, 3, 24), (32, 24, 2, 2, 37)]
LARGE_UNFUSED = (32, 520, 1, 2, 19)
LARGE_VARIANTS = {"default": {}, "no_attention": dict(use_attention=False), "no_heads": dict(use_onset_offset_heads=False)}
MT_EWORKSPACE = -2
BAND = 4096
_ID = lambda s: "nm%d-H%d-L%d-B%d-T%d" % s


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


_SD = {}


def _state_dict(mtype, nm, H, L, **kw):
    key = (mtype, nm, H, L, tuple(sorted(kw.items())))
    if key not in _SD:
        extra = {} if mtype == "cnn_rnn" else dict(use_attention=kw.get("use_attention", True), use_heads=kw.get("use_onset_offset_heads", True))
        _SD[key] = R.make_state_dict(mtype, nm, H, L, 41, **extra)
    return _SD[key]


def _eval_model(mta, mtype, shape, operand, fuse=False, **kw):
    nm, H, L, _, _ = shape
    m = mta.TranscriptionModel(model_type=mtype, n_mels=nm, hidden_size=H, num_layers=L, device="cuda", **kw)
    m.load_state_dict(_state_dict(mtype, nm, H, L, **kw), strict=True)
    m.eval()
    m.model.operand_dtype = operand
    m.model.fuse_input_projection = fuse
    return m


def _status(net, B, T):
    """The hand-off status word of every persistent recurrence launch of the forwards at (B, T): all 0."""
    words = []
    for key, ws in net._ws.items():
        if key[:2] == (B, T):
            words += [ws.view(torch.int32)[o // 4].reshape(1) for _, o in net._status_offsets(B, T)]
    assert words
    return torch.cat(words)


def _forward(m, x):
    B, T = x.shape[0], x.shape[3]
    net = m.model
    with torch.no_grad():
        if getattr(net, "use_onset_offset_heads", False):
            out = dict(net(x, return_all_heads=True, check_status=True))
        else:
            out = {"frame": net(x, check_status=True)}
    out["status"] = _status(net, B, T)
    return out


def _check(res, tag):
    for r in res:
        assert r["status"].tolist() == [0] * r["status"].numel(), (tag, r["status"].tolist())
        for k, v in r.items():
            assert bool(torch.isfinite(v.float()).all()), (tag, k)
    spreads = assert_fill_independent(res, tag=tag)
    assert all(s == 0.0 for s in spreads.values()), (tag, "the inference path has no atomics: the control runs agree bitwise", spreads)


# ------------------------------------------------------------------------------------------------------------------ CNNRNNModel
@pytest.mark.parametrize("fuse", [False, True], ids=["gemm_proj", "xproj"])
@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("shape", SMALL_FWD, ids=_ID)
def test_small_forward(mta, shape, operand, fuse):
    nm, H, L, B, T = shape
    x = _batch(B, nm, T, 5)[0].cuda()
    _check(run_under_fills(lambda: _forward(_eval_model(mta, "cnn_rnn", shape, operand, fuse), x)), (shape, operand, fuse))


# ------------------------------------------------------------------------------------------------------------------ CNNRNNModelLarge
def _direct_large(m, x):
    """mt_cnnrnn_large_forward through the struct _ensure_packed builds: everything on ONE stream (the model forward runs the local
    LSTM branch on a side stream)."""
    from music_transcription_amd import _lib
    net = m.model
    B, T = x.shape[0], x.shape[3]
    w = net._ensure_packed(x.device)["struct"]
    for l in range(net.num_layers):
        w.main_w_ihx[l] = None
    nbytes = _lib.lib.mt_cnnrnn_large_workspace_bytes(w, B, T)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    nh = 3 if net.use_onset_offset_heads else 1
    out = torch.empty(nh, B, 88, T, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.mt_cnnrnn_large_forward(w, _lib.ptr(x), None, B, T, _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr()),
               "mt_cnnrnn_large_forward")
    torch.cuda.synchronize()
    offs = [_lib.lib.mt_cnnrnn_large_status_offset(w, B, T, i) for i in range(net.num_layers + 1)]
    res = {name: out[i] for i, name in enumerate(("frame", "onset", "offset")[:nh])}
    res["status"] = torch.stack([ws.view(torch.int32)[o // 4] for o in offs])
    return res


@pytest.mark.parametrize("side_stream", [True, False], ids=["side_stream", "one_stream"])
@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("variant", list(LARGE_VARIANTS))
@pytest.mark.parametrize("shape", LARGE_FWD, ids=_ID)
def test_large_forward(mta, shape, variant, operand, side_stream):
    nm, H, L, B, T = shape
    x = _batch(B, nm, T, 6)[0].cuda().contiguous()
    run = _forward if side_stream else _direct_large
    res = run_under_fills(lambda: run(_eval_model(mta, "cnn_rnn_large", shape, operand, **LARGE_VARIANTS[variant]), x))
    _check(res, (shape, variant, operand, side_stream))


@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_large_forward_unfused_attention(mta, operand):
    """head_dim_pad = 256: S and P exist in the workspace; P's rows past T of a head "only feed masked outputs" (model_large.hip)."""
    nm, H, L, B, T = LARGE_UNFUSED
    x = _batch(B, nm, T, 7)[0].cuda()

    def fn():
        m = _eval_model(mta, "cnn_rnn_large", LARGE_UNFUSED, operand)
        assert m.model._ensure_packed(x.device)["struct"].head_dim_pad == 256
        return _forward(m, x)
    _check(run_under_fills(fn), (LARGE_UNFUSED, operand))


# ------------------------------------------------------------------------------------------------------------------ workspace reuse
@pytest.mark.parametrize("mtype,shape", [("cnn_rnn", SMALL_FWD[0]), ("cnn_rnn", SMALL_FWD[2]), ("cnn_rnn_large", LARGE_FWD[1])],
                         ids=["small-pad", "small-from_hx", "large"])
@pytest.mark.parametrize("byte", [NAN_FILL, BIG_FILL], ids=["ff", "47"])
def test_same_workspace_other_contents(mta, mtype, shape, byte):
    """A, then B (ten times the amplitude), then A again on ONE model object: the workspace the third forward finds holds B's
    intermediates, and its logits equal the first forward's bitwise."""
    nm, H, L, B, T = shape
    xa = _batch(B, nm, T, 8)[0].cuda()
    xb = (_batch(B, nm, T, 9)[0] * 10.0).cuda()
    with alloc_fill(byte):
        m = _eval_model(mta, mtype, shape, "f16")
        first = _forward(m, xa)
        n_ws = len(m.model._ws)
        ptrs = {k: v.data_ptr() for k, v in m.model._ws.items()}
        other = _forward(m, xb)
        third = _forward(m, xa)
        assert len(m.model._ws) == n_ws and {k: v.data_ptr() for k, v in m.model._ws.items()} == ptrs       # one workspace throughout
    assert not torch.equal(first["frame"], other["frame"])
    for k in first:
        assert torch.equal(first[k].view(torch.int32), third[k].view(torch.int32)), k
        assert k == "status" or bool(torch.isfinite(other[k]).all()), k
    assert first["status"].tolist() == other["status"].tolist() == [0] * first["status"].numel()


# ------------------------------------------------------------------------------------------------------------------ guard bands
def _banded(nbytes, dev, fill):
    """A uint8 tensor of 4 KiB of 0xA5 | nbytes of `fill` | 4 KiB of 0xA5 -> (whole, the middle)."""
    whole = torch.full((BAND + nbytes + BAND,), 0xA5, dtype=torch.uint8, device=dev)
    whole[BAND:BAND + nbytes] = fill
    return whole, whole[BAND:BAND + nbytes]


def _bands_intact(whole, nbytes):
    return bool((whole[:BAND] == 0xA5).all()) and bool((whole[BAND + nbytes:] == 0xA5).all())


@pytest.mark.parametrize("mtype,shape", [("cnn_rnn", SMALL_FWD[0]), ("cnn_rnn_large", LARGE_FWD[0])], ids=["small", "large"])
@pytest.mark.parametrize("operand", ["f16", "bf16"])
def test_forward_stays_inside_workspace_and_logits(mta, mtype, shape, operand):
    """The C forward with a workspace of exactly mt_cnnrnn*_workspace_bytes between two 4 KiB bands, the logits likewise: the bands
    are untouched; with workspace_bytes - 1 it returns MT_EWORKSPACE and launches nothing."""
    from music_transcription_amd import _lib
    lib = _lib.lib
    nm, H, L, B, T = shape
    m = _eval_model(mta, mtype, shape, operand)
    net = m.model
    x = _batch(B, nm, T, 10)[0].cuda().contiguous()
    w = net._ensure_packed(x.device)["struct"]
    small = mtype == "cnn_rnn"
    nbytes = (lib.mt_cnnrnn_workspace_bytes if small else lib.mt_cnnrnn_large_workspace_bytes)(w, B, T)
    fwd = lib.mt_cnnrnn_forward if small else lib.mt_cnnrnn_large_forward
    nh = 1 if small or not net.use_onset_offset_heads else 3
    n_out = nh * B * 88 * T * 4
    assert nbytes > 0 and nbytes % 256 == 0
    ws_all, ws = _banded(nbytes, x.device, 0xFF)
    lg_all, lg = _banded(n_out, x.device, 0x5A)
    before_ws, before_lg = ws_all.clone(), lg_all.clone()
    rc = fwd(w, _lib.ptr(x), None, B, T, lg.data_ptr(), ws.data_ptr(), nbytes - 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == MT_EWORKSPACE, rc
    assert torch.equal(ws_all, before_ws) and torch.equal(lg_all, before_lg)                # nothing was launched
    _lib.check(fwd(w, _lib.ptr(x), None, B, T, lg.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()), "forward")
    torch.cuda.synchronize()
    assert _bands_intact(ws_all, nbytes), "the forward wrote outside its workspace"
    assert _bands_intact(lg_all, n_out), "the forward wrote outside the logits"
    got = lg.view(torch.float32).view(nh, B, 88, T)
    with torch.no_grad():
        want = net(x, return_all_heads=True, check_status=True) if nh == 3 else net(x, check_status=True)
    want = torch.stack([want["frame"], want["onset"], want["offset"]]) if nh == 3 else want[None]
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))        # and it is the model's forward, bit for bit
