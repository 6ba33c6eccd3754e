"""The weight average inside the fused optimizer pass (mt_adam_clip_step_ema), the in-place buffer exchange (mt_swap_f32), and what
optim.FusedAdamClip, train.evaluate and scripts/train_cnn.py build on them: averaged_weights(), LRSchedule, state_dict() / resume.

  params, exp_avg, exp_avg_sq, stats of mt_adam_clip_step_ema against mt_adam_clip_step_ex; the average outside the keep ranges, on a
  skipped step and at p' == ema; mt_swap_f32; resume; averaged_weights():   EXACT (bit for bit)
  the average itself:   |e' - ref| <= 3 U max(|e|, |p'|) against the float64 rule at the kernel's own p' (optim_ema_ref has the derivation)

Inputs and references come from tests/post_optim_ref.py and tests/optim_ema_ref.py (numpy only).  Every output lies between two guard
bands.  Every test prints the figure it is about to assert (`-s` shows them).
Run only this file:  python -m pytest tests/test_gpu_optim_ema.py -q -m gpu
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ema_ref as E  # noqa: E402
import post_optim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                # elements of guard band on either side of every buffer (1024 bytes: keeps 16-byte alignment)
SENT32 = 0x7FC0BEEF                        # an f32 NaN pattern
MT_EINVAL = -1


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _lib():
    from music_transcription_amd._lib import lib, stream_ptr
    return lib, stream_ptr()


def _ok(rc):
    if rc != 0:
        from music_transcription_amd._lib import last_error
        raise AssertionError(f"call failed (code {rc}): {last_error()}")


def _say(what, **figs):
    print(f"MEASURED {what}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figs.items()))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Out:
    """n float32 words at `offset` words past a guard band, another guard band behind; everything pre-filled with a sentinel"""

    def __init__(self, n, offset=0):
        self.n, self.lo = n, GUARD + offset
        self.buf = torch.full((2 * GUARD + offset + n,), SENT32, dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo * 4

    def preset(self, values):
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)           # (a float32 array keeps its bits, NaN payloads too)
        self.buf[self.lo:self.lo + self.n] = torch.from_numpy(v.view(np.int32).copy()).cuda()
        return self

    def bits(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy().view(np.uint32)

    def body(self):
        return self.bits().view(np.float32)

    def guards_ok(self):
        return bool((self.buf[:self.lo] == SENT32).all().item()) and bool((self.buf[self.lo + self.n:] == SENT32).all().item())


class _Bufs:
    """the device state of one optimizer: p, m, v (and the average) between guard bands, the gradient, stats, workspace"""

    def __init__(self, p, g, m, v, e=None):
        lib, _ = _lib()
        self.n = p.size
        self.p, self.m, self.v = (_Out(p.size).preset(a) for a in (p, m, v))
        self.e = None if e is None else _Out(p.size).preset(e)
        self.g = torch.from_numpy(np.ascontiguousarray(g)).cuda()
        self.stats = _Out(2)
        self.nws = lib.mt_adam_workspace_bytes()
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device="cuda")

    def step(self, h, step, gs=1.0, ranges=None, w=None, ema_null=False):
        """w = None: mt_adam_clip_step_ex; otherwise mt_adam_clip_step_ema with ema_weight = w -> the return code"""
        lib, st = _lib()
        hy = (h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["max_norm"])
        kr = None if ranges is None else torch.tensor(ranges, dtype=torch.int64).reshape(-1)            # a HOST array
        krp, nk = (None, 0) if ranges is None else (kr.data_ptr(), len(ranges))
        if w is None:
            rc = lib.mt_adam_clip_step_ex(self.p.ptr, self.g.data_ptr(), self.m.ptr, self.v.ptr, self.n, *hy, step, float(gs), krp, nk,
                                          self.stats.ptr, self.ws.data_ptr(), self.nws, st)
        else:
            rc = lib.mt_adam_clip_step_ema(self.p.ptr, self.g.data_ptr(), self.m.ptr, self.v.ptr, None if ema_null else self.e.ptr, self.n,
                                           *hy, step, float(gs), krp, nk, float(w), self.stats.ptr, self.ws.data_ptr(), self.nws, st)
        torch.cuda.synchronize()
        assert all(o.guards_ok() for o in (self.p, self.m, self.v, self.stats)) and (self.e is None or self.e.guards_ok())
        return rc

    def all_bits(self):
        return [o.bits() for o in (self.p, self.m, self.v)] + ([self.e.bits()] if self.e is not None else [])


def _ranges(n):
    """three ascending keep ranges: one inside, one EMPTY, one that ends at n"""
    return [[n // 50, n // 3], [n // 3, n // 3], [n // 2, n]]


# ================================================================== 1. mt_adam_clip_step_ema
@pytest.mark.parametrize("n", E.EMA_NS)
def test_ema_step_equals_plain_step_and_average_within_bound(mta, n):
    """p', m', v' and stats are mt_adam_clip_step_ex's bit for bit (with and without keep ranges -- an empty one and one ending at n among
    them --, grad_scale 1 and 0.5, an unclipped and a clipped norm); the average lies within 3 U max(|e|, |p'|) of the float64 rule
    e + w (p' - e) evaluated at the kernel's own p' and the float32 weight (derivation: tests/optim_ema_ref.py); outside the keep ranges it
    keeps a sentinel pattern."""
    worst, k = 0.0, 0
    weights = (E.ema_weight_f32(0.999, 10 ** 6), E.ema_weight_f32(0.999, 1), 1.0)          # 1 - 0.999, 9/11, 1 (decay 0)
    for ranges in (None, _ranges(n)):
        for gs in (1.0, 0.5):
            for norm in (0.5, 30.0):                                                       # max_norm 1: unclipped, clipped
                w, step = weights[k % 3], (1, 2, 1000)[k % 3]
                k += 1
                h = R.hyper(1e-5, 1.0)
                p, g, m, v = R.adam_case(n, norm, False, grad_scale=gs, keep_ranges=ranges)
                keep = R.keep_mask(n, ranges)
                e = E.ema_state(p)
                e.view(np.uint32)[~keep] = SENT32
                a, b = _Bufs(p, g, m, v), _Bufs(p, g, m, v, e)
                _ok(a.step(h, step, gs, ranges))
                _ok(b.step(h, step, gs, ranges, w=w))
                what = f"n={n} ranges={ranges} scale={gs} norm={norm} w={w} step={step}"
                for x, y, name in zip(a.all_bits(), b.all_bits(), "pmv"):
                    assert np.array_equal(x, y), f"{what}: {name} differs from mt_adam_clip_step_ex"
                assert np.array_equal(a.stats.bits(), b.stats.bits()) and b.stats.body()[1] == 1.0, what
                assert (b.stats.body()[0] > 1.0) == (norm > 1.0), what
                assert np.array_equal(_bits(b.g.cpu().numpy()), _bits(g)), "grads was written"
                e1, p1 = b.e.body(), b.p.body()
                assert (b.e.bits()[~keep] == SENT32).all(), f"{what}: the average moved outside the keep ranges"
                ref = E.ema_ref(np.where(keep, e, 0), p1, w, ranges)
                frac = R.ratio(np.abs(e1.astype(np.float64) - ref)[keep], E.ema_bound(e, p1)[keep])
                worst = max(worst, frac)
                assert frac <= 1, (what, frac)
                assert keep.sum() == 0 or not np.array_equal(e1[keep], e[keep]), f"{what}: the average did not move"
    _say(f"ema n={n} largest fraction of the 3 U max(|e|, |p'|) bound", frac=worst)


@pytest.mark.parametrize("n", E.EMA_NS)
def test_ema_invariants(mta, n):
    h = R.hyper(1e-5, 1.0)
    p, g, m, v = R.adam_case(n, 30.0, False)
    # lr = 0, weight_decay = 0, ema = p: p never moves, and e + w (p - e) with p == e is e exactly -- over three steps
    h0 = dict(R.hyper(0.0, 1.0), lr=0.0)
    b = _Bufs(p, g, m, v, p.copy())
    for t in (1, 2, 3):
        _ok(b.step(h0, t, w=E.ema_weight_f32(0.99, t)))
        assert np.array_equal(b.p.bits(), _bits(p)) and np.array_equal(b.e.bits(), _bits(p)), f"step {t}: the average left the parameters"
    assert not np.array_equal(b.m.bits(), _bits(m))                       # (the step itself ran: the moments moved)
    # one NaN in the gradient: the step is skipped, the average with it
    e = E.ema_state(p)
    g2 = g.copy()
    g2[n // 2] = np.nan
    b = _Bufs(p, g2, m, v, e)
    _ok(b.step(h, 3, w=0.25))
    assert b.stats.body()[1] == 0.0 and np.isnan(b.stats.body()[0])
    for got, want, name in zip(b.all_bits(), (p, m, v, e), "pmve"):
        assert np.array_equal(got, _bits(want)), f"{name} moved on a skipped step"
    # refused calls write nothing
    b = _Bufs(p, g, m, v, e)
    for kw in (dict(w=0.25, ema_null=True), dict(w=0.0), dict(w=1.5), dict(w=float("nan")), dict(w=-0.1)):
        assert b.step(h, 1, **kw) == MT_EINVAL, kw
        for got, want, name in zip(b.all_bits(), (p, m, v, e), "pmve"):
            assert np.array_equal(got, _bits(want)), f"{name} was written by a refused call {kw}"
        assert (b.stats.bits() == SENT32).all()


# ================================================================== 2. mt_swap_f32
@pytest.mark.parametrize("n", E.SWAP_NS)
def test_swap_f32_exact(mta, n):
    """both pointers 16-byte aligned, one of them one float further, both one float further (the same offset inside a 16-byte line: the
    vector body with a scalar head), and offsets 1 and 3; guard words stay; two swaps restore the start"""
    lib, st = _lib()
    rng = np.random.default_rng(8000 + n)
    A = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)       # any bit pattern, NaNs included
    B = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    for oa, ob in ((0, 0), (1, 0), (0, 1), (1, 1), (1, 3)):
        a, b = _Out(n, oa).preset(A), _Out(n, ob).preset(B)
        assert a.ptr % 16 == 4 * oa and b.ptr % 16 == 4 * ob
        _ok(lib.mt_swap_f32(a.ptr, b.ptr, n, st))
        torch.cuda.synchronize()
        assert np.array_equal(a.bits(), _bits(B)) and np.array_equal(b.bits(), _bits(A)), (n, oa, ob)
        assert a.guards_ok() and b.guards_ok(), (n, oa, ob)
        _ok(lib.mt_swap_f32(a.ptr, b.ptr, n, st))
        torch.cuda.synchronize()
        assert np.array_equal(a.bits(), _bits(A)) and np.array_equal(b.bits(), _bits(B)) and a.guards_ok() and b.guards_ok(), (n, oa, ob)


def test_swap_f32_rejects_bad_arguments(mta):
    lib, st = _lib()
    a = _Out(64).preset(np.arange(64, dtype=np.float32))
    b = _Out(64).preset(-np.arange(64, dtype=np.float32))
    for args in ((a.ptr, a.ptr, 64), (a.ptr, b.ptr, 0), (a.ptr, b.ptr, -5), (None, b.ptr, 64), (a.ptr, None, 64), (a.ptr, a.ptr + 16, 64)):
        assert lib.mt_swap_f32(*args, st) == MT_EINVAL, args
    torch.cuda.synchronize()
    assert np.array_equal(a.body(), np.arange(64, dtype=np.float32)) and np.array_equal(b.body(), -np.arange(64, dtype=np.float32))


# ================================================================== 3. FusedAdamClip
def _flat_case(n, seed):
    p, g, m, v = R.adam_case(n, 2.0, True, seed=seed)
    return torch.from_numpy(p).cuda(), g


def _grad(n, k):
    return torch.from_numpy(R.adam_case(n, (0.5, 3.0, 0.9, 7.0)[k % 4], True, seed=100 + k)[1]).cuda()


def test_default_optimizer_keeps_no_average_and_is_unchanged(mta):
    from music_transcription_amd.optim import FusedAdamClip
    n = 4099
    opts = []
    for kw in ({}, {}, dict(ema_decay=0.9)):
        p0, _ = _flat_case(n, 1)
        o = FusedAdamClip(p0, torch.zeros_like(p0), lr=1e-3, **kw)
        for k in range(3):
            o.g.copy_(_grad(n, k))
            o.step()
        opts.append(o)
    a, b, c = opts
    assert a.ema is None and a.schedule is None and a.last_lr == 1e-3 and c.ema is not None
    for x, y, z in ((a.p, b.p, c.p), (a.m, b.m, c.m), (a.v, b.v, c.v)):
        assert torch.equal(x, y) and torch.equal(x, z)                      # the average changes nothing about the step itself
    assert not torch.equal(c.ema, c.p)
    with pytest.raises(RuntimeError, match="no weight average"):
        with a.averaged_weights():
            pass
    with pytest.raises(ValueError):
        FusedAdamClip(a.p, a.g, ema_decay=1.0)


def test_resume_from_state_dict_is_bit_exact(mta):
    """four steps straight == two steps, state_dict() into a fresh optimizer over the saved weights, two more steps"""
    from music_transcription_amd.optim import FusedAdamClip, LRSchedule
    n = 4099
    kw = dict(lr=1e-3, ema_decay=0.99)

    def make(p):
        return FusedAdamClip(p, torch.zeros_like(p), schedule=LRSchedule(1e-3, warmup_steps=2, total_steps=6, min_lr=1e-5), **kw)

    def run(o, ks):
        for k in ks:
            o.g.copy_(_grad(n, k))
            o.step()
    a = make(_flat_case(n, 2)[0])
    run(a, range(4))
    b = make(_flat_case(n, 2)[0])
    run(b, range(2))
    state = b.state_dict()
    assert state["t"] == 2 and all(state[k].device.type == "cpu" and state[k].numel() == n for k in ("m", "v", "ema"))
    assert state["schedule"] == dict(base_lr=1e-3, warmup_steps=2, total_steps=6, min_lr=1e-5) and state["hyper"]["ema_decay"] == 0.99
    c = make(b.p.detach().clone())
    c.load_state_dict(state)
    run(c, range(2, 4))
    for name in ("p", "m", "v", "ema"):
        assert torch.equal(getattr(a, name), getattr(c, name)), name
    assert a.t == c.t == 4 and a.last_lr == c.last_lr and a.last_lr == LRSchedule(1e-3, 2, 6, 1e-5).at(4) and a.last_lr < 1e-3
    # what does not fit is refused: another length, a state with an average into an optimizer without one, and the reverse
    plain = FusedAdamClip(b.p.detach().clone(), torch.zeros_like(b.p), lr=1e-3)
    with pytest.raises(ValueError):
        plain.load_state_dict(state)
    with pytest.raises(ValueError):
        c.load_state_dict(plain.state_dict())
    short = make(b.p[:100].detach().clone())
    with pytest.raises(ValueError):
        short.load_state_dict(state)


def _mel_in(B, nm, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, nm, T, generator=g) * 60.0 - 70.0 + 10.0 * torch.randn(B, 1, nm, 1, generator=g))


def _roll_in(B, T, seed, p=0.04):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 88, T, generator=g) < p).float()


NM, HID, LAYERS, T_FRAMES = 32, 16, 2, 40          # the tiny CNNRNNModel of test_gpu_train.py's script test


def test_averaged_weights_swaps_the_model_in_place(mta):
    from oracle import model_ref
    from music_transcription_amd.optim import WEIGHTS_EPOCH
    from music_transcription_amd import train as T
    model = mta.TranscriptionModel(model_type="cnn_rnn", n_mels=NM, hidden_size=HID, num_layers=LAYERS, dropout=0.0, device="cuda")
    model.load_state_dict(model_ref.make_state_dict("cnn_rnn", NM, HID, LAYERS, 5), strict=True)
    data = [(_mel_in(4, NM, T_FRAMES, 20 + k).cuda(), _roll_in(4, T_FRAMES, 30 + k, 0.1).cuda(), torch.full((4,), T_FRAMES, dtype=torch.int64))
            for k in range(3)]
    opt = mta.make_optimizer(model, lr=3e-3, ema_decay=0.5)
    _, losses = mta.train_one_epoch(model, data, opt, torch.device("cuda"))
    assert len(losses) == 3 and opt.t == 3
    live, avg = opt.p.detach().clone(), opt.ema.detach().clone()
    assert not torch.equal(live, avg)

    def flat():
        return torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    x = data[0][0]
    model.eval()
    with torch.no_grad():
        logits_live = model(x).clone()
    e0 = WEIGHTS_EPOCH[0]
    with opt.averaged_weights():
        assert torch.equal(flat(), avg) and torch.equal(opt.ema, live)
        with torch.no_grad():
            logits_avg = model(x).clone()
        saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
        with pytest.raises(RuntimeError, match="averaged_weights"):
            opt.step()
    assert torch.equal(flat(), live) and torch.equal(opt.ema, avg) and WEIGHTS_EPOCH[0] == e0 + 2
    with torch.no_grad():
        assert torch.equal(model(x), logits_live)                          # the packed inference weights followed the exchange back
    second = mta.TranscriptionModel(model_type="cnn_rnn", n_mels=NM, hidden_size=HID, num_layers=LAYERS, device="cuda")
    second.load_state_dict(saved)
    second.eval()
    with torch.no_grad():
        assert torch.equal(second(x), logits_avg)
    assert not torch.equal(logits_avg, logits_live)
    with pytest.raises(KeyError):                                           # the body raises: the live weights come back all the same
        with opt.averaged_weights():
            raise KeyError("body")
    assert torch.equal(flat(), live) and torch.equal(opt.ema, avg) and WEIGHTS_EPOCH[0] == e0 + 4
    # train.evaluate(averaged=True): the same loop under the averaged weights, the live ones back afterwards
    val = [(m.cpu(), r.cpu(), l) for m, r, l in data[:2]]
    v_live = T.evaluate(model, val, torch.device("cuda"))
    v_avg = T.evaluate(model, val, torch.device("cuda"), optimizer=opt, averaged=True)
    assert np.isfinite(v_avg) and v_avg != v_live and torch.equal(flat(), live)
    with pytest.raises(TypeError):
        T.evaluate(model, val, torch.device("cuda"), averaged=True)


# ================================================================== 4. scripts/train_cnn.py
SCRIPT_FLAGS = ["--batch_size", "2", "--lr", "3e-3", "--n_mels", str(NM), "--hidden_size", str(HID), "--num_layers", str(LAYERS), "--dropout", "0.1",
                "--save_every", "3", "--num_workers", "0", "--ema_decay", "0.9", "--warmup_steps", "2", "--lr_decay", "cosine"]


def _train(cache, run, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_cnn.py"), "--cached_dir", cache, "--run_dir", run, *SCRIPT_FLAGS, *extra],
                          capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def straight_run(mta, tmp_path_factory):
    """the tiny cache of test_gpu_train.py::test_train_cnn_script_two_epochs and one two-epoch run on it (4 steps per epoch)"""
    tmp = tmp_path_factory.mktemp("ema_script")
    cache = str(tmp / "cache")
    for split, n in (("train", 8), ("validation", 3)):
        for i in range(n):
            mel = _mel_in(1, NM, T_FRAMES - (i % 3) * 5, 200 + i)[0]
            roll = _roll_in(1, mel.shape[-1], 300 + i, 0.1)[0]
            mta.write_cache_chunk(cache, split, i, mel, roll)
        mta.write_cache_metadata(cache, split, [{} for _ in range(n)], n_mels=NM)
    run = str(tmp / "run")
    r = _train(cache, run, "--epochs", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    return cache, run, json.load(open(os.path.join(run, "history.json"))), tmp


def test_train_cnn_script_with_average_and_schedule(mta, straight_run):
    cache, run, hist, tmp = straight_run
    from oracle import model_ref
    assert len(hist) == 2
    for rec in hist:
        assert all(np.isfinite(rec[k]) for k in ("val_loss", "val_loss_ema", "lr", "opt_step", "train_loss")), rec
    assert [h["opt_step"] for h in hist] == [4, 8] and hist[1]["lr"] == 0.0 and 0.0 < hist[0]["lr"] < 3e-3
    man = model_ref.make_state_dict("cnn_rnn", NM, HID, LAYERS, 0)
    ck = os.path.join(run, "checkpoints")
    for name in ("model_best_ema.pth", "model_final_ema.pth", "model_ema_epoch_2.pth", "model_epoch_2.pth", "model_best.pth", "model_final.pth"):
        sd = torch.load(os.path.join(ck, name))
        assert set(sd) == set(man) and all(sd[k].shape == man[k].shape and sd[k].device.type == "cpu" for k in man), name
    ema, live = torch.load(os.path.join(ck, "model_final_ema.pth")), torch.load(os.path.join(ck, "model_final.pth"))
    assert any(not torch.equal(ema[k], live[k]) for k in man if "running_" not in k and "num_batches" not in k)
    assert all(torch.equal(ema[k], torch.load(os.path.join(ck, "model_ema_epoch_2.pth"))[k]) for k in man)
    state = torch.load(os.path.join(ck, "train_state.pth"))
    assert state["epoch"] == 2 and state["optimizer"]["t"] == 8 and state["optimizer"]["ema"] is not None and len(state["history"]) == 2
    assert state["best_val_loss"] == min(h["val_loss"] for h in hist) and state["best_val_loss_ema"] == min(h["val_loss_ema"] for h in hist)
    e = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "evaluate.py"), "--model", os.path.join(ck, "model_best_ema.pth"),
                        "--cache_dir", cache, "--split", "validation", "--model_type", "cnn_rnn", "--hidden_size", str(HID), "--num_layers", str(LAYERS),
                        "--threshold", "0.3", "--headless"], capture_output=True, text=True, timeout=300)
    assert e.returncode == 0, e.stderr[-2000:]
    assert e.stdout.strip().startswith("EVAL_MEAN_F1="), e.stdout
    both = _train(cache, str(tmp / "both"), "--epochs", "1", "--resume", os.path.join(ck, "model_final.pth"), "--resume_state", os.path.join(ck, "train_state.pth"))
    assert both.returncode == 2 and "--resume_state" in both.stderr


def test_train_cnn_script_resume_state(mta, straight_run):
    """--epochs 1, then --epochs 2 --resume_state: the second epoch starts at the optimizer step, and ends at the learning rate, of the
    straight two-epoch run.  The loss is only required to be finite: bitwise determinism of a step across processes is not claimed."""
    cache, _, hist, tmp = straight_run
    run = str(tmp / "resumed")
    r1 = _train(cache, run, "--epochs", "1")
    assert r1.returncode == 0, r1.stderr[-2000:]
    state_path = os.path.join(run, "checkpoints", "train_state.pth")
    assert torch.load(state_path)["optimizer"]["t"] == 4
    r2 = _train(cache, run, "--epochs", "2", "--resume_state", state_path)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert "Resumed from" in r2.stdout
    h2 = json.load(open(os.path.join(run, "history.json")))
    assert [h["epoch"] for h in h2] == [1, 2]
    assert h2[1]["opt_step"] == hist[1]["opt_step"] == 8 and h2[1]["lr"] == hist[1]["lr"]
    assert all(np.isfinite(h2[1][k]) for k in ("train_loss", "val_loss", "val_loss_ema"))
    assert torch.load(state_path)["optimizer"]["t"] == 8
