"""The HIP training steps (train_step.CnnRnnTrainFn, train_step_large.CnnRnnLargeTrainFn) under torch's autograd contract, not only
under the one forward + backward + step() pattern of the training loop: steps in flight together, gradient accumulation, graphs
dropped without a backward, an inference forward between a forward and its backward, shape changes with steps in flight, and the
optimizer's flat gradient buffer under each of them.

Every case is an autograd PROGRAM over two (or four) batches that differ in mel, roll and ragged lengths -- with identical batches
another step's partial products would be the right numbers.  It runs on the HIP model and, through torch autograd, on the CPU
oracle (same state dict, train-mode BatchNorm updating the running statistics in place):
  * CNNRNNModel: the bounds of test_gpu_train.py (GRAD_REL / GRAD_COS against the oracle with the HIP path's bf16 rounding
    points, GRAD_REL_FP32 with the sweep's per-key bounds against the fp32 oracle);
  * CNNRNNModelLarge: the oracle-noise-floor bound of test_gpu_train_large.py as a sanity check, and the tight check against the
    same HIP steps run in ISOLATION (a fresh model per step, gradients summed on the host): 1e-3 of each tensor's largest entry,
    or 2x the spread measured between two isolated runs of one step where that is larger (atomics in the bias and BatchNorm
    statistic sums), capped at 1e-2.  The BatchNorm running statistics follow from the isolated runs exactly (momentum algebra).
Dropout has no oracle: with dropout on, the programs are compared against the isolated HIP steps under the same seeds, also at
the canonical width of CNNRNNModel (H = 512, L = 3, B = 16, T = 937: a 0.5 GB BPTT workspace per step).
Observed spread between two isolated runs of one step (max |g1 - g2| / max |g1| over tensors): 0 at every shape here, the
canonical width with dropout included, so every bound stays at 1e-3.
At the oracle shapes the backward recurrence's producers stay ahead of their consumers, so a workspace another step has filled is
overwritten before it is read; at the canonical width it is not: there, CNNRNNModel with one pooled BPTT workspace per shape and
no lease was 3 - 12 % off in its convolution gradients with two steps in flight."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model_ref as R
from test_gpu_train import GRAD_COS, GRAD_COS_FP32, GRAD_REL, GRAD_REL_FP32, GRAD_REL_FP32_BY_KEY_SWEEP, ZERO_GRAD_KEYS
from test_gpu_train_large import ZERO_GRAD as ZERO_GRAD_LARGE, _bound, FLOOR_AMP, FLOOR_SEEDS, GRAD_COS as GRAD_COS_LARGE

SMALL = [(40, 32, 1, 3, 33), (40, 32, 3, 2, 29), (38, 20, 2, 4, 21)]     # (n_mels, H, L, B, T): L = 1, L = 3, Hp = 32 > H = 20
LARGE_SHAPE = (32, 16, 2, 3, 24)
LARGE_KW = [dict(), dict(use_attention=False)]
HIP_REL, HIP_REL_CAP = 1e-3, 1e-2
# Against the bf16-EMULATING oracle, conv2's weight gradient (a heavily cancelling sum) carries the pool's tie routing: the HIP path
# routes a pooled pair by the order of its f32 results (mt_conv_cl_tie), the oracle by the rounded bf16 values.  Observed 0.036 for
# a single step at n_mels = 38 (odd n_mels // 2); the fp32 comparison keeps the sweep's bound for it.
GRAD_REL_EMU_BY_KEY = {"model.cnn.4.weight": 5e-2}
BN_TOL = 3e-3


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _batch(B, nm, T, seed):
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, 1, nm, T, generator=g) * 60.0 - 70.0 + 10.0 * torch.randn(B, 1, nm, 1, generator=g)
    roll = (torch.rand(B, 88, T, generator=g) < 0.1).float()
    lengths = torch.tensor([T - (3 * seed + 5 * b) % (T // 2) for b in range(B)], dtype=torch.int64)
    for b in range(B):
        mel[b, :, :, lengths[b]:] = 0.0
        roll[b, :, lengths[b]:] = 0.0
    return mel, roll, lengths


def _pair(B, nm, T):
    a, b = _batch(B, nm, T, 11), _batch(B, nm, T, 12)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])
    return a, b


def _model(mta, mtype, nm, H, L, seed, dropout=0.0, **kw):
    m = mta.TranscriptionModel(model_type=mtype, n_mels=nm, hidden_size=H, num_layers=L, dropout=dropout, device="cuda", **kw)
    sd = R.make_state_dict(mtype, nm, H, L, seed, **({} if mtype == "cnn_rnn" else
                                                       dict(use_attention=kw.get("use_attention", True), use_heads=kw.get("use_onset_offset_heads", True))))
    m.load_state_dict(sd, strict=True)
    if mtype == "cnn_rnn_large":
        m.model.dropout2d_p = (0.1, 0.1, 0.15) if dropout > 0.0 else (0.0, 0.0, 0.0)
    m.train()
    return m, sd


# ------------------------------------------------------------------------------------------------------------- runners
class _Hip:
    """Runs a program on the HIP model; `probe(tag)` records the busy flags of the step workspace pool."""

    def __init__(self, m, seeds=None):
        self.m, self.seeds, self.n, self.probes = m, seeds, 0, {}

    def loss(self, batch):
        if self.seeds is not None:
            torch.manual_seed(self.seeds[self.n])
        self.n += 1
        mel, roll, lengths = batch
        return self.m.compute_loss(self.m(mel.cuda()), roll.cuda(), lengths)

    def infer(self, batch):
        self.m.eval()
        with torch.no_grad():
            out = self.m(batch[0].cuda()).cpu()
        self.m.train()
        return out

    def probe(self, tag):
        self.probes[tag] = [getattr(e, "busy", None) for e in _pool(self.m).values()]


class _Oracle:
    def __init__(self, mtype, sd, emulate):
        self.mtype, self.o = mtype, R.Opts(gemm_bf16=emulate)
        self.sd = {k: v.clone() for k, v in sd.items()}
        self.keys = [k for k, v in self.sd.items() if v.dtype.is_floating_point and "running_" not in k]
        for k in self.keys:
            self.sd[k].requires_grad_(True)

    def _fwd(self, x, train):
        if self.mtype == "cnn_rnn":
            return R.cnnrnn_forward(self.sd, x, self.o, train=train)
        return R.cnnrnn_large_forward(self.sd, x, o=self.o, train=train)

    def loss(self, batch):
        mel, roll, lengths = batch
        return R.compute_loss(self._fwd(mel, True), roll, lengths)

    def infer(self, batch):
        with torch.no_grad():
            return R.cnnrnn_forward(self.sd, batch[0]) if self.mtype == "cnn_rnn" else R.cnnrnn_large_forward(self.sd, batch[0])

    def probe(self, tag):
        pass

    def grads(self):
        return {k: (self.sd[k].grad.clone() if self.sd[k].grad is not None else torch.zeros_like(self.sd[k])) for k in self.keys}


def _pool(m):
    net = m.model
    return net.__dict__.get("_bptt_parts" if type(net).__name__ == "CNNRNNModel" else "_train_ws", {})


# ------------------------------------------------------------------------------------------------------------- programs
def p_sequential(r, a, b):          # 1. accumulation: no zero_grad between the two steps
    la = r.loss(a)
    la.backward()
    lb = r.loss(b)
    lb.backward()


def p_summed(r, a, b):              # 2. two steps in flight, one backward through both
    (r.loss(a) + r.loss(b)).backward()


def p_ab(r, a, b):                  # 3. two steps in flight, their backwards in forward order ...
    la, lb = r.loss(a), r.loss(b)
    la.backward()
    lb.backward()


def p_ba(r, a, b):                  # ... and in reverse order
    la, lb = r.loss(a), r.loss(b)
    lb.backward()
    la.backward()


def p_dropped(r, a, b):             # 4. a's graph is dropped without a backward
    la = r.loss(a)
    r.probe("a")
    del la
    r.probe("dropped")
    lb = r.loss(b)
    r.probe("b")
    lb.backward()
    r.probe("end")


def p_eval_between(r, a, b):        # 5. an inference forward between a's forward and its backward
    la = r.loss(a)
    r.out_b = r.infer(b)
    la.backward()


PROGRAMS = {"sequential": (p_sequential, "ab"), "summed": (p_summed, "ab"), "ab": (p_ab, "ab"), "ba": (p_ba, "ab"),
            "dropped": (p_dropped, "b"), "eval_between": (p_eval_between, "a")}     # -> (program, whose gradients it leaves)


# ------------------------------------------------------------------------------------------------------------- comparisons
def _hip_grads(m, opt=None):
    """{oracle key: gradient} from p.grad (None -> zeros); with `opt`, ALSO from its flat buffer after _reattach_grad_views()."""
    out = {"model." + n: (p.grad.detach().float().cpu().clone() if p.grad is not None else torch.zeros(p.shape))
           for n, p in m.model.named_parameters()}
    if opt is None:
        return out, None
    opt._reattach_grad_views()
    names = {id(p): "model." + n for n, p in m.model.named_parameters()}
    flat = {names[id(p)]: opt.g[o:o + k].view(p.shape).float().cpu().clone() for p, o, k in opt._views}
    assert set(flat) == set(out)
    return out, flat


def _worst(got, ref, zero_keys):
    w, fa, fb = {}, [], []
    for k, b in ref.items():
        a = got[k].double().numpy()
        b = b.detach().double().numpy()
        assert a.shape == b.shape, k
        if k[len("model."):] in zero_keys:
            continue
        s = np.abs(b).max()
        if s == 0.0:                        # no gradient path (frame-only loss: the onset / offset heads): exactly zero here too
            assert np.abs(a).max() == 0.0, k
            continue
        w[k] = float(np.abs(a - b).max() / s)
        fa.append(a.ravel()); fb.append(b.ravel())
    fa, fb = np.concatenate(fa), np.concatenate(fb)
    return w, float(fa @ fb / (np.linalg.norm(fa) * np.linalg.norm(fb)))


def _check_small_vs_oracle(got, sd, batches, prog, tag):
    for emulate in (True, False):
        o = _Oracle("cnn_rnn", sd, emulate)
        prog(o, *batches)
        w, cos = _worst(got, o.grads(), ZERO_GRAD_KEYS)
        if emulate:
            bad = {k: v for k, v in w.items() if v > GRAD_REL_EMU_BY_KEY.get(k, GRAD_REL)}
            assert not bad and cos > GRAD_COS, (tag, "bf16-emulating oracle", bad, cos)
        else:
            bad = {k: v for k, v in w.items() if v > GRAD_REL_FP32_BY_KEY_SWEEP.get(k, GRAD_REL_FP32)}
            assert not bad and cos > GRAD_COS_FP32, (tag, "fp32 oracle", bad, cos)
    return o


def _check_bn(m, sd_ref, tol=BN_TOL):
    got = m.state_dict()
    n = 0
    for k, b in sd_ref.items():
        if "running_" in k:
            a = got[k].float().cpu()
            assert float((a - b.float()).abs().max()) <= tol * max(float(b.abs().max()), 1.0), k
            n += 1
        elif "num_batches_tracked" in k:
            assert int(got[k]) == int(b), (k, int(got[k]), int(b))
    assert n > 0


# ------------------------------------------------------------------------------------------------------------- CNNRNNModel
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "nm%d-H%d-L%d-B%d-T%d" % s)
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_small_program_matches_oracle(mta, shape, name):
    nm, H, L, B, T = shape
    prog, which = PROGRAMS[name]
    m, sd = _model(mta, "cnn_rnn", nm, H, L, seed=21)
    a, b = _pair(B, nm, T)
    r = _Hip(m)
    prog(r, a, b)
    got, _ = _hip_grads(m)
    probes = dict(r.probes)
    iso = [_isolated(mta, "cnn_rnn", shape, {}, 21, x) for x in (a, b)]
    again = _isolated(mta, "cnn_rnn", shape, {}, 21, a, again=True)
    _check_vs_isolated(got, [iso[i][0] for i, c in enumerate("ab") if c in which], _spread(iso[0][0], again[0]), name)
    o = _check_small_vs_oracle(got, sd, (a, b), prog, name)
    _check_bn(m, o.sd)                                  # (the fp32 oracle's running statistics: the same forwards)
    if name == "eval_between":
        assert float((r.out_b - _eval_after(sd, a, "cnn_rnn")(b[0])).abs().max()) < 3e-2
    if name == "dropped":
        assert probes["a"] == [True] and probes["dropped"] == [False], probes            # the graph's drop released the lease ...
        assert probes["b"] == [True] and probes["end"] == [False], probes                # ... and b took the pooled workspace
    assert all(not e.busy for e in _pool(m).values())
    m.model.raise_on_train_handoff_timeout()


def _eval_after(sd, a, mtype):
    """The oracle's eval-mode forward with the running statistics after a train-mode forward of batch a."""
    sdo = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        if mtype == "cnn_rnn":
            R.cnnrnn_forward(sdo, a[0], train=True)
            return lambda x: R.cnnrnn_forward(sdo, x)
        R.cnnrnn_large_forward(sdo, a[0], train=True)
        return lambda x: R.cnnrnn_large_forward(sdo, x)


_ACQ = []


def _acquisitions(monkeypatch):
    """Records every step_pool.acquire: (key, pooled entry leased?)."""
    from music_transcription_amd import step_pool
    rec, orig = _ACQ, step_pool.acquire
    rec.clear()

    def acquire(pool, key, make, fresh, max_entries=2):
        ws, lease = orig(pool, key, make, fresh, max_entries)
        rec.append((key, lease is not None, id(ws)))
        return ws, lease
    monkeypatch.setattr(step_pool, "acquire", acquire)
    return rec


@pytest.mark.parametrize("shape", [SMALL[1], SMALL[2]], ids=lambda s: "nm%d-H%d-L%d-B%d-T%d" % s)
def test_small_shape_changes_with_steps_in_flight(mta, shape, monkeypatch):
    """6. Forwards at T1, T2, T3 and T2 again before any backward: the two-shape pool is full of leased entries at T3 and T2's entry
    is leased at the fourth -- both must get private workspaces, and no pending step's workspace may be evicted or handed out."""
    nm, H, L, B, T = shape
    rec = _acquisitions(monkeypatch)
    m, sd = _model(mta, "cnn_rnn", nm, H, L, seed=22)
    bs = [_batch(B, nm, t, 30 + i) for i, t in enumerate((T, T - 4, T + 5, T - 4))]

    def prog(r, *bs):
        ls = [r.loss(x) for x in bs]
        for i in (2, 0, 3, 1):
            ls[i].backward()
    prog(_Hip(m), *bs)
    got, _ = _hip_grads(m)
    rec = list(rec)
    iso = [_isolated(mta, "cnn_rnn", shape, {}, 22, x) for x in bs]
    again = _isolated(mta, "cnn_rnn", shape, {}, 22, bs[0], again=True)
    _check_vs_isolated(got, [g for g, _ in iso], _spread(iso[0][0], again[0]), "shapes")
    o = _check_small_vs_oracle(got, sd, bs, prog, "shapes")
    _check_bn(m, o.sd)
    assert [h for _, h, _ in rec] == [True, True, False, False], rec
    assert len(_pool(m)) == 2 and all(not e.busy for e in _pool(m).values())
    n0 = len(_ACQ)                                      # the pool serves the next single step at T2
    m.compute_loss(m(bs[1][0].cuda()), bs[1][1].cuda(), bs[1][2]).backward()
    assert [h for _, h, _ in _ACQ[n0:]] == [True]


# ------------------------------------------------------------------------------------------------------------- optimizer
def _opt_variant(mta, m, mode, monkeypatch):
    if mode == "no_direct":
        monkeypatch.setenv("MT_DIRECT_GRADS", "0")
    opt = mta.make_optimizer(m, lr=1e-4)
    assert (getattr(m.model, "_grad_target", None) is None) == (mode == "no_direct")
    if mode == "set_to_none":
        m.zero_grad(set_to_none=True)
    else:
        opt.zero_grad()
    return opt


@pytest.mark.parametrize("mode", ["direct", "no_direct", "set_to_none"])
@pytest.mark.parametrize("name", ["sequential", "summed", "ab", "ba"])
def test_small_optimizer_flat_gradient(mta, name, mode, monkeypatch):
    """7. Patterns 1 - 3 with the optimizer attached: its direct gradient targets, MT_DIRECT_GRADS=0, model.zero_grad(set_to_none=True)
    (the reference loop's call).  p.grad and the flat buffer after _reattach_grad_views() hold the oracle's accumulated gradient."""
    nm, H, L, B, T = SMALL[1]
    prog = PROGRAMS[name][0]
    m, sd = _model(mta, "cnn_rnn", nm, H, L, seed=23)
    opt = _opt_variant(mta, m, mode, monkeypatch)
    a, b = _pair(B, nm, T)
    prog(_Hip(m), a, b)
    got, flat = _hip_grads(m, opt)
    for g in (got, flat):
        o = _check_small_vs_oracle(g, sd, (a, b), prog, f"{name}/{mode}")
    _check_bn(m, o.sd)


def test_small_second_backward_raises(mta):
    nm, H, L, B, T = SMALL[0]
    m, _ = _model(mta, "cnn_rnn", nm, H, L, seed=24)
    a, _ = _pair(B, nm, T)
    la = _Hip(m).loss(a)
    la.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        la.backward()
    assert all(not e.busy for e in _pool(m).values())


def test_handoff_status_covers_every_step_in_flight(mta):
    """raise_on_train_handoff_timeout reads the status words of every step since its last call -- here two steps in flight --
    not only the latest forward's, and forgets them afterwards.  (No timeout is provoked: after the clean check, a status word of
    the EARLIER step is set by hand to a timeout code, which the check must report.)"""
    for mtype, shape in (("cnn_rnn", SMALL[1]), ("cnn_rnn_large", LARGE_SHAPE)):
        nm, H, L, B, T = shape
        m, _ = _model(mta, mtype, nm, H, L, seed=25)
        a, b = _pair(B, nm, T)
        nl = 2 * L if mtype == "cnn_rnn" else 2 * (L + 1)      # persistent launches per step: forward + backward recurrences
        for fake in (False, True):
            r = _Hip(m)
            la, lb = r.loss(a), r.loss(b)
            lb.backward()
            la.backward()
            pending = list(m.model._train_syncs)
            assert len(pending) == 2 and pending[0][0].data_ptr() != pending[1][0].data_ptr()
            for buf, stride in pending:             # every launch of both steps zeroed its own slot and reported no timeout
                assert buf.view(torch.int32)[:: stride // 4].cpu().tolist() == [0] * nl
            if not fake:
                m.model.raise_on_train_handoff_timeout()
            else:
                buf, stride = pending[0]
                buf.view(torch.int32)[(nl - 1) * (stride // 4)] = 0x40000003
                with pytest.raises(mta.MtError, match=r"training step 1 of 2 .* launch %d timed out" % (nl - 1)):
                    m.model.raise_on_train_handoff_timeout()
            assert m.model._train_syncs == []
            m.model.raise_on_train_handoff_timeout()    # nothing pending


def test_plain_training_loop_reuses_pooled_workspaces(mta, monkeypatch):
    """The single-step path: in train_one_epoch every step leases the ONE pooled workspace of its shape, for both models."""
    rec = _acquisitions(monkeypatch)
    for mtype, shape, kw in (("cnn_rnn", SMALL[1], {}), ("cnn_rnn_large", LARGE_SHAPE, {})):
        nm, H, L, B, T = shape
        m, _ = _model(mta, mtype, nm, H, L, seed=26, **kw)
        opt = mta.make_optimizer(m, lr=1e-4)
        rec.clear()
        data = []
        for i in range(4):
            mel, roll, lengths = _batch(B, nm, T, 40 + i)
            data.append((mel.cuda(), roll.cuda(), lengths))
        mta.train_one_epoch(m, data, opt, torch.device("cuda"))
        assert len(rec) == 4 and all(h for _, h, _ in rec) and len({w for _, _, w in rec}) == 1, rec
        assert all(not e.busy for e in _pool(m).values())


# ------------------------------------------------------------------------------------------------------------- skipped batch
def _nan_epoch(mta, m, a, b, monkeypatch):
    """4 through train_one_epoch: batch a's roll holds a NaN (non-finite loss, clean forward: skipped), then batch b."""
    rec = _acquisitions(monkeypatch)
    opt = mta.make_optimizer(m, lr=1e-4)
    roll_a = a[1].clone()
    roll_a[0, 3, 2] = float("nan")
    data = [(a[0].cuda(), roll_a.cuda(), a[2]), (b[0].cuda(), b[1].cuda(), b[2])]
    _, losses = mta.train_one_epoch(m, data, opt, torch.device("cuda"), max_grad_norm=1e9)
    assert len(losses) == 1 and math.isfinite(losses[0])
    assert len(_pool(m)) == 1 and all(not e.busy for e in _pool(m).values())       # the skipped step's lease went back ...
    assert [h for _, h, _ in rec] == [True, True] and rec[0][2] == rec[1][2], rec      # ... and b reused the pooled workspace
    for bn in [mod for mod in m.model.modules() if isinstance(mod, torch.nn.BatchNorm2d)]:
        assert torch.isfinite(bn.running_mean).all() and torch.isfinite(bn.running_var).all()
    opt._reattach_grad_views()
    names = {id(p): "model." + n for n, p in m.model.named_parameters()}
    return {names[id(p)]: opt.g[o:o + k].view(p.shape).float().cpu().clone() for p, o, k in opt._views}


@pytest.mark.parametrize("shape", [SMALL[0], SMALL[1]], ids=lambda s: "nm%d-H%d-L%d-B%d-T%d" % s)
def test_small_skipped_nan_batch_in_training_loop(mta, shape, monkeypatch):
    nm, H, L, B, T = shape
    m, sd = _model(mta, "cnn_rnn", nm, H, L, seed=27)
    a, b = _pair(B, nm, T)
    flat = _nan_epoch(mta, m, a, b, monkeypatch)
    o = _check_small_vs_oracle(flat, sd, (a, b), p_dropped, "nan epoch")    # the gradient of b alone (the step does not clear it)
    _check_bn(m, o.sd)                                                      # both forwards updated the running statistics


# ------------------------------------------------------------------------------------------------------------- CNNRNNModelLarge
_ISO = {}


def _isolated(mta, mtype, shape, kw, sd_seed, batch, dropout=0.0, seed=None, again=False):
    """The HIP step of one batch on a fresh model: (grads, running statistics).  Cached per configuration; again=True runs it anew."""
    key = (mtype, shape, tuple(sorted(kw.items())), sd_seed, float(batch[0].double().sum()), float(batch[1].sum()), tuple(batch[2].tolist()),
           dropout, seed)
    if key in _ISO and not again:
        return _ISO[key]
    nm, H, L, B, T = shape
    m, _ = _model(mta, mtype, nm, H, L, seed=sd_seed, dropout=dropout, **kw)
    _Hip(m, None if seed is None else [seed]).loss(batch).backward()
    out = (_hip_grads(m)[0], {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items() if "running_" in k})
    if not again:
        _ISO[key] = out
    return out


def _spread(g1, g2):
    return {k: float((g1[k] - g2[k]).abs().max()) / max(float(g1[k].abs().max()), 1e-30) for k in g1}


def _check_vs_isolated(got, parts, spread, tag):
    """got == sum of the isolated steps' gradients within max(1e-3, 2 x spread) of each tensor's largest entry, capped at 1e-2."""
    want = {k: sum(p[k] for p in parts) for k in parts[0]}
    bad = {}
    for k, w in want.items():
        s = float(w.abs().max())
        if s == 0.0:
            assert float(got[k].abs().max()) == 0.0, (tag, k)
            continue
        bound = max(HIP_REL, min(2.0 * spread.get(k, 0.0), HIP_REL_CAP))
        e = float((got[k] - w).abs().max()) / s
        if e > bound:
            bad[k] = (e, bound)
    assert not bad, (tag, bad)


def _bn_from_isolated(r0, iso_stats):
    """Running statistics after forwards of batches 1..n from the same start r0: r_n = 0.9^n r0 + sum_i 0.1 * 0.9^(n-i) mu_i, where
    each isolated step gives 0.1 mu_i = r_i - 0.9 r0 (BatchNorm momentum 0.1)."""
    n = len(iso_stats)
    out = {}
    for k in iso_stats[0]:
        v = (0.9 ** n) * r0[k]
        for i, st in enumerate(iso_stats):
            v = v + (0.9 ** (n - 1 - i)) * (st[k] - 0.9 * r0[k])
        out[k] = v
    return out


_FLOOR = {}


def _program_floor(sd, batches, prog):
    """The emulating oracle's distance from ITSELF over the whole program (test_gpu_train_large._oracle_noise_floor: every 16-bit
    rounding of an activation preceded by a relative perturbation of 2^-20, three seeds): ({tensor: max distance}, smallest cosine)."""
    o = _Oracle("cnn_rnn_large", sd, True)
    prog(o, *batches)
    ref = o.grads()
    floor, cos_min = {}, 1.0
    orig = R._bf16_round
    for seed in FLOOR_SEEDS:
        gen = torch.Generator().manual_seed(seed)

        def dithered(x, gen=gen):
            if not (x.is_leaf and x.requires_grad):
                x = x + x.detach() * (FLOOR_AMP * (2.0 * torch.rand(x.shape, generator=gen) - 1.0))
            return orig(x)
        R._bf16_round = dithered
        try:
            od = _Oracle("cnn_rnn_large", sd, True)
            prog(od, *batches)
        finally:
            R._bf16_round = orig
        w, c = _worst(od.grads(), ref, ZERO_GRAD_LARGE)
        for k, v in w.items():
            floor[k] = max(floor.get(k, 0.0), v)
        cos_min = min(cos_min, c)
    return o, floor, cos_min


def _large_vs_oracle(got, sd, batches, prog, tag):
    """Sanity check against the oracle: within the oracle's own noise floor over the same program (test_gpu_train_large's bound)."""
    o, floor, cos_floor = _program_floor(sd, batches, prog)
    w, cos = _worst(got, o.grads(), ZERO_GRAD_LARGE)
    bad = {k: (v, floor.get(k)) for k, v in w.items() if v > _bound(floor, k)}
    assert not bad and cos > min(GRAD_COS_LARGE, cos_floor - 1e-3), (tag, bad, cos, cos_floor)
    return o


def _large_expected(mta, kw, sd_seed, batches, which, dropout=0.0, seeds=None):
    """(list of isolated gradient dicts to sum, spread, isolated running statistics of every forward)"""
    iso = [_isolated(mta, "cnn_rnn_large", LARGE_SHAPE, kw, sd_seed, x, dropout, None if seeds is None else seeds[i]) for i, x in enumerate(batches)]
    again = _isolated(mta, "cnn_rnn_large", LARGE_SHAPE, kw, sd_seed, batches[0], dropout, None if seeds is None else seeds[0], again=True)
    spread = _spread(iso[0][0], again[0])
    parts = [iso[i][0] for i, c in enumerate("ab") if c in which]
    return parts, spread, [s for _, s in iso]


@pytest.mark.parametrize("kw", LARGE_KW, ids=["default", "no_attention"])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_large_program_matches_isolated_steps_and_oracle(mta, name, kw):
    nm, H, L, B, T = LARGE_SHAPE
    prog, which = PROGRAMS[name]
    m, sd = _model(mta, "cnn_rnn_large", nm, H, L, seed=31, **kw)
    r0 = {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items() if "running_" in k}
    a, b = _pair(B, nm, T)
    r = _Hip(m)
    prog(r, a, b)
    got, _ = _hip_grads(m)
    parts, spread, stats = _large_expected(mta, kw, 31, (a, b), which)
    _check_vs_isolated(got, parts, spread, name)
    fwd = (a, b) if name != "eval_between" else (a,)          # (the inference forward leaves the running statistics alone)
    want_bn = _bn_from_isolated(r0, stats[:len(fwd)])
    sdm = m.state_dict()
    for k, v in want_bn.items():
        assert float((sdm[k].float().cpu() - v).abs().max()) <= 1e-5 * max(float(v.abs().max()), 1.0), k
    o = _large_vs_oracle(got, sd, (a, b), prog, name)
    _check_bn(m, o.sd)
    if name == "eval_between":
        assert float((r.out_b - _eval_after(sd, a, "cnn_rnn_large")(b[0])).abs().max()) < 3e-2
    if name == "dropped":                               # the drop of a's graph released its lease, and b took the pooled workspace
        assert r.probes["a"] == [True] and r.probes["dropped"] == [False], r.probes
        assert r.probes["b"] == [True] and r.probes["end"] == [False], r.probes
    assert all(not e.busy for e in _pool(m).values())
    m.model.raise_on_train_handoff_timeout()


def test_large_shape_changes_with_steps_in_flight(mta, monkeypatch):
    nm, H, L, B, T = LARGE_SHAPE
    rec = _acquisitions(monkeypatch)
    m, sd = _model(mta, "cnn_rnn_large", nm, H, L, seed=32)
    bs = [_batch(B, nm, t, 30 + i) for i, t in enumerate((T, T - 4, T + 5, T - 4))]
    ls = [_Hip(m).loss(x) for x in bs]
    for i in (2, 0, 3, 1):
        ls[i].backward()
    got, _ = _hip_grads(m)
    rec = list(rec)
    iso = [_isolated(mta, "cnn_rnn_large", LARGE_SHAPE, {}, 32, x) for x in bs]
    again = _isolated(mta, "cnn_rnn_large", LARGE_SHAPE, {}, 32, bs[0], again=True)
    _check_vs_isolated(got, [g for g, _ in iso], _spread(iso[0][0], again[0]), "shapes")
    assert [h for _, h, _ in rec] == [True, True, False, False], rec
    assert len(_pool(m)) == 2 and all(not e.busy for e in _pool(m).values())


@pytest.mark.parametrize("mode", ["direct", "no_direct", "set_to_none"])
@pytest.mark.parametrize("name", ["sequential", "summed", "ab", "ba"])
def test_large_optimizer_flat_gradient(mta, name, mode, monkeypatch):
    nm, H, L, B, T = LARGE_SHAPE
    prog = PROGRAMS[name][0]
    m, sd = _model(mta, "cnn_rnn_large", nm, H, L, seed=33)
    opt = _opt_variant(mta, m, mode, monkeypatch)
    a, b = _pair(B, nm, T)
    prog(_Hip(m), a, b)
    got, flat = _hip_grads(m, opt)
    parts, spread, _ = _large_expected(mta, {}, 33, (a, b), "ab")
    for g in (got, flat):
        _check_vs_isolated(g, parts, spread, f"{name}/{mode}")
    _large_vs_oracle(flat, sd, (a, b), prog, f"{name}/{mode}")


def test_large_second_backward_raises(mta):
    nm, H, L, B, T = LARGE_SHAPE
    m, _ = _model(mta, "cnn_rnn_large", nm, H, L, seed=34)
    a, _ = _pair(B, nm, T)
    la = _Hip(m).loss(a)
    la.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        la.backward()
    assert all(not e.busy for e in _pool(m).values())


@pytest.mark.parametrize("kw", LARGE_KW, ids=["default", "no_attention"])
def test_large_skipped_nan_batch_in_training_loop(mta, kw, monkeypatch):
    nm, H, L, B, T = LARGE_SHAPE
    m, sd = _model(mta, "cnn_rnn_large", nm, H, L, seed=35, **kw)
    a, b = _pair(B, nm, T)
    flat = _nan_epoch(mta, m, a, b, monkeypatch)
    parts, spread, _ = _large_expected(mta, kw, 35, (a, b), "b")
    _check_vs_isolated(flat, parts, spread, "nan epoch")


# ------------------------------------------------------------------------------------------------------------- dropout, canonical width
@pytest.mark.parametrize("name", ["summed", "ab", "ba"])
@pytest.mark.parametrize("mtype", ["cnn_rnn", "cnn_rnn_large"])
def test_dropout_programs_match_isolated_steps(mta, mtype, name):
    """9. Dropout masks have no oracle: the program with dropout on (the same torch seeds in front of each forward) against the
    same two HIP steps run in isolation."""
    shape = SMALL[1] if mtype == "cnn_rnn" else LARGE_SHAPE
    nm, H, L, B, T = shape
    seeds = (101, 202)
    m, _ = _model(mta, mtype, nm, H, L, seed=36, dropout=0.3)
    a, b = _pair(B, nm, T)
    PROGRAMS[name][0](_Hip(m, seeds), a, b)
    got, _ = _hip_grads(m)
    iso = [_isolated(mta, mtype, shape, {}, 36, x, 0.3, s) for x, s in zip((a, b), seeds)]
    again = _isolated(mta, mtype, shape, {}, 36, a, 0.3, seeds[0], again=True)
    _check_vs_isolated(got, [g for g, _ in iso], _spread(iso[0][0], again[0]), f"{mtype} dropout {name}")
    other = _isolated(mta, mtype, shape, {}, 36, a, 0.3, 999)                # (the masks DO depend on the seed)
    assert max(float((other[0][k] - iso[0][0][k]).abs().max()) for k in other[0]) > 0.0


CANON = (229, 512, 3, 16, 937)


def _canon_check(mta, got, bs, seeds, tag):
    iso = [_isolated(mta, "cnn_rnn", CANON, {}, 37, x, 0.3, sd_) for x, sd_ in zip(bs, seeds)]
    again = _isolated(mta, "cnn_rnn", CANON, {}, 37, bs[0], 0.3, seeds[0], again=True)
    spread = _spread(iso[0][0], again[0])
    print("\n[canonical width, %s] spread between two isolated runs: max %.3g" % (tag, max(spread.values())))
    _check_vs_isolated(got, [g for g, _ in iso], spread, "canonical " + tag)


@pytest.mark.parametrize("name", ["summed", "ab", "ba"])
def test_canonical_width_steps_in_flight_match_isolated(mta, name):
    """CNNRNNModel at the canonical width (H = 512, L = 3, B = 16, T = 937) with dropout: two steps in flight, against the two
    steps run in isolation (HIP against HIP)."""
    nm, H, L, B, T = CANON
    seeds = (7, 8)
    a, b = _batch(B, nm, T, 51), _batch(B, nm, T, 52)
    m, _ = _model(mta, "cnn_rnn", nm, H, L, seed=37, dropout=0.3)
    PROGRAMS[name][0](_Hip(m, seeds), a, b)
    got, _ = _hip_grads(m)
    del m
    _canon_check(mta, got, (a, b), seeds, name)


def test_canonical_width_shape_changes_with_steps_in_flight(mta):
    nm, H, L, B, T = CANON
    seeds = (7, 8, 9, 10)
    bs = [_batch(B, nm, t, 60 + i) for i, t in enumerate((T, T - 36, T + 23, T - 36))]
    m, _ = _model(mta, "cnn_rnn", nm, H, L, seed=37, dropout=0.3)
    r = _Hip(m, seeds)
    ls = [r.loss(x) for x in bs]
    for i in (2, 0, 3, 1):
        ls[i].backward()
    got, _ = _hip_grads(m)
    del m, ls
    _canon_check(mta, got, bs, seeds, "shapes")
    _ISO.clear()
