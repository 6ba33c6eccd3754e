"""Two workgroup sets when alone (csrc/lstm.hip, lstm_wide_kernel).  A plain inference recurrence with 2 .. 4 batch groups carries a
second set of workgroups; the device decides when the launch starts whether the two sets share the groups (wide: 4 = 2 + 2, 3 = 2 + 1,
2 = 1 + 1) or the second set leaves (narrow, every group in set 0 as before).  The arithmetic per group is the same, so wide and narrow
must agree in every BIT -- the whole hx image, padded batch rows included, and the logits of the model forward -- and that is all this file
compares: forced wide against forced narrow (mt_lstm_set_width_mode), and the device's own choice against both.

Shapes: the smallest that reach every split.  H = 64 (NKSW = 1), T = 7 (the six-slot gx ring wraps with one group per set), B = 64 / 96 /
128 (2, 3, 4 groups), B = 40 and 100 (the last group partly empty: 1 + 1 and 2 + 2); H = 512, T = 5, B = 128 for the register shape of
the benchmark; gx as f16 and as f32.  B <= 32 is one group: no second set, decision word 0.

What a decision word may hold once the stream has drained: 0 (a launch with one set), 1 (narrow), 2 (wide)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GX_F16 = 0x10
NONE, NARROW, WIDE = 0, 1, 2
AUTO, FORCE_NARROW, FORCE_WIDE = 0, 1, 2
SHAPES = [(64, 64, 7), (64, 96, 7), (64, 128, 7), (64, 40, 7), (64, 100, 7), (512, 128, 5)]          # (H, B, T)


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(autouse=True)
def _auto_mode_afterwards(mta):
    from music_transcription_amd._lib import lib
    yield
    assert lib.mt_lstm_set_width_mode(AUTO) == 0
    torch.cuda.synchronize()


_IN = {}


def _inputs(H, B, T, g16):
    """gx in the kernel's own layout (any values will do: random, padded batch slots included) and W_hh ~ U(-1/sqrt(H), 1/sqrt(H)); made once"""
    from music_transcription_amd._lib import lib
    key = (H, B, T, g16)
    if key not in _IN:
        g = torch.Generator(device="cuda").manual_seed(1000 * H + 10 * B + T)
        n = lib.mt_lstm_gx_bytes(B, T, H) // 4
        gx = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
        gx = gx.to(torch.float16) if g16 else gx
        whh = (torch.rand(2 * 4 * H * H, generator=g, device="cuda", dtype=torch.float32) * 2.0 - 1.0) / H ** 0.5
        _IN[key] = (gx, whh)
    return _IN[key]


class _Launch:
    """one mt_lstm_bidir_fwd_ex call on `stream` (None: the current one); nothing is synchronised here"""

    def __init__(self, H, B, T, g16, stream=None):
        from music_transcription_amd._lib import lib, check, stream_ptr
        gx, whh = _inputs(H, B, T, g16)
        self.hx = torch.full((lib.mt_lstm_hx_bytes(B, T, H),), 0x5A, dtype=torch.uint8, device="cuda")
        self.sync = torch.full((lib.mt_lstm_sync_bytes(B, H),), 0x5A, dtype=torch.uint8, device="cuda")
        self.args = (gx.data_ptr(), whh.data_ptr(), self.hx.data_ptr(), self.sync.data_ptr(), self.sync.numel(), B, T, H, GX_F16 if g16 else 0)
        self.st = stream.cuda_stream if stream is not None else stream_ptr()
        self.lib, self.check = lib, check

    def go(self):
        self.check(self.lib.mt_lstm_bidir_fwd_ex(*self.args, self.st))
        return self

    def status(self):
        return int(self.sync[:4].view(torch.int32).item())

    def decision(self):
        o = self.lib.mt_lstm_width_offset()
        return int(self.sync[o:o + 4].view(torch.int32).item())


def _run(mode, H, B, T, g16):
    from music_transcription_amd._lib import lib
    assert lib.mt_lstm_set_width_mode(mode) == 0
    torch.cuda.synchronize()
    r = _Launch(H, B, T, g16).go()
    torch.cuda.synchronize()
    assert r.status() == 0, "hand-off timeout"
    return r


_NARROW = {}


def _narrow(H, B, T, g16):
    """the forced-narrow result of a shape: computed once, compared against by every test"""
    key = (H, B, T, g16)
    if key not in _NARROW:
        r = _run(FORCE_NARROW, H, B, T, g16)
        assert r.decision() == (NARROW if B > 32 else NONE)
        h = r.hx.view(torch.float16)
        assert bool(torch.isfinite(h).all()), "an unpublished (poisoned) word in hx"
        assert float(h.float().abs().max()) > 0.05
        _NARROW[key] = r.hx.clone()
    return _NARROW[key]


def _max_diff(a, b):
    return float((a.view(torch.float16).float() - b.view(torch.float16).float()).abs().max())


@pytest.mark.parametrize("g16", [True, False], ids=["gx_f16", "gx_f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forced_wide_equals_forced_narrow(mta, shape, g16):
    H, B, T = shape
    want = _narrow(H, B, T, g16)
    r = _run(FORCE_WIDE, H, B, T, g16)
    assert r.decision() == WIDE
    d = _max_diff(r.hx, want)
    print(f"MEASURE {shape} g16={g16} max|wide - narrow| = {d}")
    assert d == 0.0 and torch.equal(r.hx, want)


@pytest.mark.parametrize("B", [32, 20, 7])
def test_one_group_has_one_set(mta, B):
    """B <= 32: auto and forced wide run the kernel with one set (decision word 0) and give the same bits"""
    H, T = 64, 7
    want = _narrow(H, B, T, True)
    for mode in (AUTO, FORCE_WIDE):
        r = _run(mode, H, B, T, True)
        assert r.decision() == NONE
        assert torch.equal(r.hx, want), mode


def test_auto_is_wide_on_an_idle_device_every_time(mta):
    """after a synchronize nothing else runs: the decision is wide, and the count returns to zero behind every launch -- ten launches in a
    row on one stream are all wide and all equal to narrow"""
    from music_transcription_amd._lib import lib
    H, B, T = 64, 128, 7
    want = _narrow(H, B, T, True)
    r = _run(AUTO, H, B, T, True)
    assert r.decision() == WIDE
    assert torch.equal(r.hx, want)
    runs = [_Launch(H, B, T, True).go() for _ in range(10)]
    torch.cuda.synchronize()
    assert [x.status() for x in runs] == [0] * 10
    assert [x.decision() for x in runs] == [WIDE] * 10
    assert all(torch.equal(x.hx, want) for x in runs)
    assert lib.mt_persistent_cus_in_flight(None) == 0


def test_two_streams_back_to_back_at_most_one_wide(mta):
    """T = 600 steps (about a millisecond per launch) so that the second launch, enqueued some tens of microseconds behind the first, starts
    while the first runs; that they did overlap is read from events (how far the second one's end lies behind the first one's), and "at
    most one wide" is what overlapping launches owe -- two launches one after the other are both alone and both wide"""
    H, B, T = 64, 128, 600
    want = _narrow(H, B, T, True)
    from music_transcription_amd._lib import lib
    assert lib.mt_lstm_set_width_mode(AUTO) == 0
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a_start, a_end, b_end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a, b = _Launch(H, B, T, True, s1), _Launch(H, B, T, True, s2)
    torch.cuda.synchronize()
    a_start.record(s1)
    a.go(), b.go()
    a_end.record(s1)
    b_end.record(s2)
    torch.cuda.synchronize()
    assert a.status() == 0 and b.status() == 0
    da, db = a.decision(), b.decision()
    dur_a, b_after_a = a_start.elapsed_time(a_end), a_end.elapsed_time(b_end)
    print(f"MEASURE decisions of two launches queued back to back: {da} {db}; the first took {dur_a:.3f} ms, the second ended {b_after_a:.3f} ms behind it")
    assert da in (NARROW, WIDE) and db in (NARROW, WIDE)
    # (the second launch takes at least as long as the first, which started alone: ending less than 0.8 of that behind it, it started inside it)
    if b_after_a < 0.8 * dur_a:
        assert (da == WIDE) + (db == WIDE) <= 1
    assert torch.equal(a.hx, want) and torch.equal(b.hx, want)
    # and the count is back at zero: the next launch alone is wide
    assert _run(AUTO, H, B, T, True).decision() == WIDE


# ---------------------------------------------------------------------------------------------------------------- the model forward
def _logits(mta, mode, operand, B):
    """CNNRNNModel(n_mels 32, H 64, 2 layers) at T = 19: (logits, decision word of every layer)"""
    from music_transcription_amd._lib import lib
    from oracle import model_ref as R
    nm, H, L, T = 32, 64, 2, 19
    m = mta.TranscriptionModel(model_type="cnn_rnn", n_mels=nm, hidden_size=H, num_layers=L, device="cuda")
    m.load_state_dict(R.make_state_dict("cnn_rnn", nm, H, L, 41), strict=True)
    m.eval()
    m.model.operand_dtype = operand
    m.model.fuse_input_projection = False
    g = torch.Generator().manual_seed(B)
    x = (torch.rand(B, 1, nm, T, generator=g) * 60.0 - 70.0).cuda()
    assert lib.mt_lstm_set_width_mode(mode) == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        y = m.model(x, check_status=True)
    torch.cuda.synchronize()
    net, dec = m.model, []
    for key, ws in net._ws.items():
        if key[:2] == (B, T):
            dec += [int(ws.view(torch.int32)[(o + lib.mt_lstm_width_offset()) // 4].item()) for _, o in net._status_offsets(B, T)]
    assert len(dec) == L
    return y.clone(), dec


@pytest.mark.parametrize("operand", ["f16", "bf16"])
@pytest.mark.parametrize("B", [64, 96, 128, 40, 100])
def test_forward_logits_wide_equal_narrow(mta, B, operand):
    """mt_cnnrnn_forward: forced wide, forced narrow and the device's own choice give the same logits bit for bit; alone on the device every
    layer of the forward decides wide (the forward's own place in the count of running launches does not count against it)"""
    yn, dn = _logits(mta, FORCE_NARROW, operand, B)
    yw, dw = _logits(mta, FORCE_WIDE, operand, B)
    ya, da = _logits(mta, AUTO, operand, B)
    assert dn == [NARROW] * 2 and dw == [WIDE] * 2 and da == [WIDE] * 2, (dn, dw, da)
    assert bool(torch.isfinite(yn).all())
    d = float((yw - yn).abs().max())
    print(f"MEASURE B={B} {operand} max|logits wide - narrow| = {d}")
    assert d == 0.0 and torch.equal(yw, yn) and torch.equal(ya, yn)
