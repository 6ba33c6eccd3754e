"""Packed Viterbi paths on the GPU (csrc/smooth.hip, mt_frame_smooth_paths, notes.smooth_frame_paths; DESIGN.md 6c "Smoothing in the decoder
grid") against the literal specification of frame_smooth_ref.py: random rows of 4200 frames (66 windows: past one backward block of 64
windows and past several slabs) over lengths on every boundary, K = 1, 5 and 16 candidates in one call, rows built to carry a state
across a whole block, (0, 0) against the threshold kernel, and the C ABI's refusals.  Integer arithmetic on quantised evidence: every
comparison is exact.  The reference is given the activity the library itself thresholds (mt_predict_threshold), as in
test_gpu_frame_smooth.py."""
import numpy as np
import pytest
import torch

import frame_smooth_ref as FR

pytestmark = pytest.mark.gpu

B, P, T = 3, 3, 4200
W = (T + 63) // 64
LENGTH_SETS = [(0, 1, 63), (64, 65, 1023), (1024, 1025, 4095), (4096, 4097, 4200), None]
PENALTIES = [(0.0, 0.0), (0.5, 0.5), (2.0, 0.0), (0.0, 2.0), (64.0, 64.0)]
THRESHOLDS = (0.3, 0.5, 0.8)
SENTINEL = -7
EINVAL = -1


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _raw():
    from music_transcription_amd import _lib
    return _lib.lib, _lib.ptr, _lib.stream_ptr


def _f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


def raw_paths(x, thr, on, off, lengths=None, K=None):
    """mt_frame_smooth_paths called directly -> rc, paths (K, B, P, W) int64 that started as sentinels."""
    lib, ptr, stream = _raw()
    Bn, Pn, Tn = x.shape
    thr, on, off = _f32(thr), _f32(on), _f32(off)
    K = len(thr) if K is None else K
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device="cuda")
    shape = (max(K, 1), Bn, Pn, (Tn + 63) // 64)
    paths, work = (torch.full(shape, SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2))
    rc = lib.mt_frame_smooth_paths(ptr(x), thr.ctypes.data, on.ctypes.data, off.ctypes.data, K, ptr(ln), Bn, Pn, Tn, ptr(paths), ptr(work), stream())
    torch.cuda.synchronize()
    return rc, paths


def unpack(paths, Tn):
    """(..., W) int64 words -> (..., T) bool and whether any bit past T is set."""
    a = paths.cpu().numpy().view(np.uint64)
    bits = ((a[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(a.shape[:-1] + (-1,))
    return bits[..., :Tn], bool(bits[..., Tn:].any())


def _activity(x, thr):
    from music_transcription_amd import ops
    return ops.predict_from_logits(x.contiguous().float(), thr).cpu().numpy() > 0


def spec_bits(x, thr, on, off, lengths=None):
    """x (B, P, T) on the device -> (B, P, T) bool: where smooth_ref is +64, and 0 at or past a sample's length."""
    xn = x.cpu().numpy()
    want = FR.smooth_ref(xn, thr, on, off, lengths, _activity(x, thr)) == FR.Y_ON
    if lengths is not None:
        for b, L in enumerate(lengths):
            want[b, :, L:] = False
    return want


_CASE = {}


def _random_case():
    """Noisy evidence around Markov runs, as test_gpu_frame_smooth.py's: blips, dropouts and long stretches inside the band at every
    penalty; the first pitch on the 1/64 grid; infinities and +-80.  Built once, nobody writes to it."""
    if not _CASE:
        from offset_decode_ref import markov
        rng = np.random.default_rng(21)
        runs = markov(rng, (B, P, T), 0.05, 0.08)
        x = (rng.normal(0, 1.0, (B, P, T)) + np.where(runs, 1.0, -1.0) * rng.choice([0.3, 1.5], (B, P, 1))).astype(np.float32)
        x[:, 0] = np.round(x[:, 0] * 64) / 64
        x[1, 1, 40], x[1, 1, 700], x[2, 2, 64], x[2, 2, 4187] = np.inf, -np.inf, 80.0, -80.0
        x.setflags(write=False)
        _CASE.update(x=x, dev=torch.from_numpy(x.copy()).cuda(), want={})
    return _CASE


def _poisoned(lengths):
    x = _random_case()["dev"]
    if lengths is None:
        return x
    x = x.clone()
    for b, L in enumerate(lengths):
        x[b, :, L:] = float("nan")                                           # frames that must never be read
    return x


def _want(thr, pen, lengths):
    """The specification on the random case, computed once per (threshold, penalties, lengths) and shared by the tests."""
    cache = _random_case()["want"]
    key = (thr, pen, lengths)
    if key not in cache:
        cache[key] = spec_bits(_poisoned(lengths), thr, *pen, lengths)
        cache[key].setflags(write=False)
    return cache[key]


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_five_candidates_of_one_threshold_equal_the_specification(mta, thr):
    on, off = zip(*PENALTIES)
    changed = 0
    for lengths in LENGTH_SETS:
        x = _poisoned(lengths)
        rc, paths = raw_paths(x, [thr] * 5, on, off, None if lengths is None else list(lengths))
        got, past = unpack(paths, T)
        assert rc == 0 and not past, lengths
        for k, pen in enumerate(PENALTIES):
            want = _want(thr, pen, lengths)
            assert np.array_equal(got[k], want), (lengths, pen, np.argwhere(got[k] != want)[:5])
        for b, L in enumerate(lengths or ()):
            assert not got[:, b, :, L:].any()                                # bits past the length are 0; length 0: all zeros
        if lengths is None:
            act = _activity(x, thr)
            assert np.array_equal(got[0], act)                               # (0, 0) is the threshold
            changed = [int((got[k] != act).sum()) for k in range(1, 5)]
            for k, pen in enumerate(PENALTIES[1:], 1):                       # and the float kernel writes +64 exactly there
                y = mta.smooth_frame_logits(x, thr, *pen)                    # ((0, 0) launches nothing and returns x itself)
                assert np.array_equal(y.cpu().numpy() > 0, got[k]), pen
    assert all(c > 100 for c in changed), changed                            # the penalties do change paths


def test_one_and_sixteen_candidates_in_one_call(mta):
    x = _random_case()["dev"]
    cand = [(thr, pen) for thr in THRESHOLDS for pen in PENALTIES] + [(0.5, (2.0, 0.0))]       # 16: thresholds and penalties mixed
    for lengths in (None, LENGTH_SETS[3], LENGTH_SETS[1]):
        xp = _poisoned(lengths)
        ln = None if lengths is None else list(lengths)
        rc, paths = raw_paths(xp, [c[0] for c in cand], [c[1][0] for c in cand], [c[1][1] for c in cand], ln)
        got, past = unpack(paths, T)
        assert rc == 0 and not past and got.shape == (16, B, P, T)
        for k, (thr, pen) in enumerate(cand):
            assert np.array_equal(got[k], _want(thr, pen, lengths)), (lengths, thr, pen)
        for thr, pen in (cand[7], cand[14]):                                 # K = 1
            rc, one = raw_paths(xp, [thr], [pen[0]], [pen[1]], ln)
            assert rc == 0 and np.array_equal(unpack(one, T)[0][0], _want(thr, pen, lengths)), (lengths, thr, pen)
    # the Python wrapper: one threshold for all pairs, one per pair, more than 16 pairs, (P, T) input, lengths
    got = mta.smooth_frame_paths(x, 0.5, PENALTIES)
    assert got.shape == (5, B, P, W) and got.dtype == torch.int64 and got.is_cuda
    for k, pen in enumerate(PENALTIES):
        assert np.array_equal(unpack(got, T)[0][k], _want(0.5, pen, None))
    many = cand + cand[:4]
    got = mta.smooth_frame_paths(_poisoned(LENGTH_SETS[2]), [c[0] for c in many], [c[1] for c in many], LENGTH_SETS[2])
    assert got.shape == (20, B, P, W)
    for k, (thr, pen) in enumerate(many):
        assert np.array_equal(unpack(got, T)[0][k], _want(thr, pen, LENGTH_SETS[2])), k
    one = mta.smooth_frame_paths(x[0], 0.3, [(2.0, 0.0)])
    assert one.shape == (1, 1, P, W) and np.array_equal(unpack(one, T)[0][0, 0], _want(0.3, (2.0, 0.0), None)[0])
    with pytest.raises(ValueError):
        mta.smooth_frame_paths(x, [0.5, 0.3], PENALTIES)
    with pytest.raises(ValueError):
        mta.smooth_frame_paths(x, 0.5, [])
    with pytest.raises(ValueError):
        mta.smooth_frame_paths(x, 0.5, [(65.0, 0.0)])
    assert np.array_equal(x.cpu().numpy(), _random_case()["x"])              # the input is never written


# ------------------------------------------------------------------------------------------------ rows built for the block carry
def _built_rows():
    """-> x (N, 1, 9000), lengths, names.  Penalties (2, 2): a = b = 128; +-0.1 logits are 6 grid steps, so alternating them keeps d
    inside the band, and a logit of +-5 is decisive on its own.  A block of the backward pass is 64 windows = 4096 frames."""
    Tn = 9000
    wiggle = np.where(np.arange(Tn) % 2 == 0, 0.1, -0.1).astype(np.float32)
    rows, lengths, names = [], [], []

    def add(name, row, L=Tn):
        rows.append(row.astype(np.float32))
        lengths.append(L)
        names.append(name)
    for sign in (1.0, -1.0):
        r = wiggle.copy()
        r[0], r[8500], r[8900] = -5.0 * sign, 5.0 * sign, -5.0 * sign            # 8499 undecided frames below a decisive one: the whole
        r[1], r[8501] = 1.0 * sign, -1.0 * sign                                  # block of frames 4096 .. 8191 holds no decisive frame
        add(f"band{sign:+.0f}", r)
    for L in (9000, 8193, 8192, 4097, 4096, 4095):                               # the only decisive frame is the last: its parity decides
        add(f"last{L}", wiggle.copy(), L)
    r = wiggle.copy()
    r[0], r[1] = 5.0, -1.0                                                       # decisive at frame 0 only (and, by definition, the last)
    add("first", r, 8999)
    r = wiggle.copy()
    r[4095], r[4096], r[8191], r[8192] = np.inf, -np.inf, 80.0, -80.0            # on both sides of the block boundaries
    add("extremes", r)
    return np.stack(rows)[:, None, :], lengths, names


def test_rows_whose_carry_crosses_a_whole_block(mta):
    x, lengths, names = _built_rows()
    dev = torch.from_numpy(x).cuda()
    rc, paths = raw_paths(dev, [0.5, 0.5], [2.0, 0.0], [2.0, 0.0], lengths)
    got, past = unpack(paths, x.shape[-1])
    assert rc == 0 and not past
    want = spec_bits(dev, 0.5, 2.0, 2.0, lengths)
    for n, name in enumerate(names):
        assert np.array_equal(got[0, n], want[n]), (name, np.argwhere(got[0, n] != want[n])[:5])
    assert np.array_equal(got[1], spec_bits(dev, 0.5, 0.0, 0.0, lengths))
    path = {name: want[n, 0, :lengths[n]] for n, name in enumerate(names)}       # and the rows do what they are named for
    for name in ("band+1", "band-1"):
        d = FR.forward_d(FR.quantise(x[names.index(name), 0], 0.5), 128, 128)
        assert (np.abs(d[1:8500]) < 128).all() and (np.abs(d[8501:8900]) < 128).all() and all(abs(d[t]) > 128 for t in (0, 8500, 8900))
    assert not path["band+1"][0] and path["band+1"][1:8501].all() and not path["band+1"][8501:].any()
    assert path["band-1"][0] and not path["band-1"][1:8501].any() and path["band-1"][8501:].all()
    for L in (9000, 8193, 8192, 4097, 4096, 4095):                               # d of the last frame is 6 or 0: one state all along
        assert path[f"last{L}"].all() == (L % 2 == 1) and path[f"last{L}"].any() == (L % 2 == 1)
    assert path["first"][0] and path["first"][1:].all() == path["first"][1:].any()
    y = mta.smooth_frame_logits(dev, 0.5, 2.0, 2.0, lengths).cpu().numpy()
    for n, L in enumerate(lengths):
        assert np.array_equal(y[n, 0, :L] > 0, got[0, n, 0, :L])


# ------------------------------------------------------------------------------------------------ (0, 0) is the threshold
def test_no_penalty_is_the_threshold_activity_bit_for_bit(mta):
    rng = np.random.default_rng(23)
    x = rng.normal(0, 0.05, (2, 3, 1100)).astype(np.float32)                     # crowded around the thresholds' logits
    for i, thr in enumerate(THRESHOLDS):
        c = FR.centre(thr)
        x[0, i, :5] = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)), c - np.float32(1e-3), c + np.float32(1e-3)]
        x[1, i] += c
    dev = torch.from_numpy(x).cuda()
    rc, paths = raw_paths(dev, THRESHOLDS, [0.0] * 3, [0.0] * 3)
    got, past = unpack(paths, 1100)
    assert rc == 0 and not past
    for k, thr in enumerate(THRESHOLDS):
        act = _activity(dev, thr)
        assert np.array_equal(got[k], act) and 0 < act.mean() < 1


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def test_c_abi_refusals_leave_the_paths_alone(mta):
    from music_transcription_amd import _lib
    lib, ptr, stream = _raw()
    x = _random_case()["dev"]
    nan = float("nan")
    bad = [(0.5, -0.5, 0.0), (0.5, 0.0, -1e-3), (0.5, 64.5, 0.0), (0.5, 0.0, 1e9), (0.5, nan, 0.0), (0.5, 0.0, nan), (0.0, 1.0, 1.0), (1.0, 1.0, 1.0),
           (-0.1, 1.0, 1.0), (nan, 1.0, 1.0)]
    for thr, on, off in bad:
        for at in (0, 2):                                                    # the bad candidate first, and after two good ones
            t, a, b = [0.5] * 3, [1.0] * 3, [1.0] * 3
            t[at], a[at], b[at] = thr, on, off
            rc, got = raw_paths(x, t, a, b, [5, 5, 5])
            assert rc == EINVAL and (got == SENTINEL).all(), (thr, on, off, at)
            assert "penalty" in _lib.last_error() or "threshold" in _lib.last_error()
    for K in (0, 17, -1):
        rc, got = raw_paths(x, [0.5] * 17, [1.0] * 17, [1.0] * 17, K=K)
        assert rc == EINVAL and (got == SENTINEL).all(), K
    assert "K" in _lib.last_error()
    paths, work = (torch.full((2, B, P, W), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2))
    h = _f32([0.5, 0.5])
    good = [ptr(x), h.ctypes.data, h.ctypes.data, h.ctypes.data, 2, None, B, P, T, ptr(paths), ptr(work), stream()]
    assert lib.mt_frame_smooth_paths(*good) == 0                             # (the arguments below differ from these in one place)
    torch.cuda.synchronize()
    paths.fill_(SENTINEL)
    for i in (0, 1, 2, 3, 9, 10):
        args = list(good)
        args[i] = None
        assert lib.mt_frame_smooth_paths(*args) == EINVAL and "null" in _lib.last_error(), i
    for dims in ((0, P, T), (B, 0, T), (B, P, 0), (B, -1, T), (1 << 11, 1 << 10, T)):
        args = list(good)
        args[6:9] = dims
        assert lib.mt_frame_smooth_paths(*args) == EINVAL and "dims" in _lib.last_error(), dims
    both = torch.full((4 * B * P * W,), SENTINEL, dtype=torch.int64, device="cuda")
    xf = torch.full((2 * x.numel(),), float(SENTINEL), device="cuda")
    for pa, wa, xa in ((both.data_ptr(), both.data_ptr() + 8 * W, ptr(x)),   # work inside paths
                       (both.data_ptr() + 8, both.data_ptr(), ptr(x)),       # paths inside work
                       (both.data_ptr(), both.data_ptr(), ptr(x)),           # one buffer for both
                       (xf.data_ptr() + 8, ptr(work), xf.data_ptr()),        # paths inside the logits
                       (ptr(paths), xf.data_ptr() + 4 * x.numel() - 8, xf.data_ptr())):       # work begins inside the logits
        args = list(good)
        args[0], args[9], args[10] = xa, pa, wa
        assert lib.mt_frame_smooth_paths(*args) == EINVAL and "overlap" in _lib.last_error()
    torch.cuda.synchronize()
    assert (paths == SENTINEL).all() and (both == SENTINEL).all() and (xf == SENTINEL).all()
