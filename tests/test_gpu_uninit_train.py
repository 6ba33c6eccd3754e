"""The training steps and the fused optimizer under poisoned allocations (tests/alloc_fill.py).

One step = train-mode forward, compute_loss with ragged lengths, backward, on a freshly built model; run_under_fills runs it under
0x00 twice, 0xFF and 0x47.  Compared: the logits, the loss and its parts, every parameter's gradient, the BatchNorm running
statistics -- bitwise where the two control runs agree bitwise, else within twice their spread capped at 1e-3 of the largest entry
(alloc_fill.assert_fill_independent; the float atomics of the BatchNorm and bias sums in train.hip / train_large.hip are the only
known source of a spread).  The hand-off status word of every persistent launch is 0 under every fill.

What this pins in train_step.py / train_step_large.py / step_pool.py: the ~95 torch.empty tensors of the two steps -- the pad rows
of X0 / dG / dGT ("only feed discarded GEMM outputs, but must be finite for the transposed use": X0[M:].zero_(), dG[M:].zero_(),
dGT[:, M:].zero_(), dGT[8 * Hp:].zero_()), the regions of _StepWorkspace "zeroed ONCE ... no kernel ever writes there", _FreshZeros
for a second step in flight, and the kernel workspaces of the losses (ops.py) and of the optimizer (optim.py).

Control-to-control spread observed on an MI355X at these shapes: 0 for every tensor of every case in the runs made (printed per case
with -s).  It is not asserted to be 0: the float atomics may order their additions differently in another run, and the rule above
allows for that."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from alloc_fill import alloc_fill, assert_fill_independent, mismatches, run_under_fills
from test_gpu_train_autograd import LARGE_KW, LARGE_SHAPE, SMALL, _acquisitions, _batch, _model, _pair, _Hip

LARGE_PAD = (32, 24, 2, 2, 37)      # Hp = 32 > H, Hl = 12 -> Hlp = 16, comb = 72 -> Cp = 128, Hs = 64 > H, T = 37 -> Tp = 64
STEP_CASES = ([("cnn_rnn", s, {}) for s in SMALL] + [("cnn_rnn_large", LARGE_SHAPE, kw) for kw in LARGE_KW]
              + [("cnn_rnn_large", LARGE_PAD, {})])
_CASE_ID = lambda c: "%s-nm%d-H%d-L%d-B%d-T%d" % ((c[0],) + c[1]) + ("-no_attention" if c[2] else "")


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _loss_config():
    from music_transcription_amd import ops
    return ops.LossConfig(head_weights=(0.6, 0.3, 0.1), pos_weight=(2.0, 3.0, 1.5), focal_gamma=(1.5, 2.0, 0.5))


def _status_words(m):
    """The status word of every persistent launch of every step since the last check (all must be 0); the check itself follows."""
    pending = list(getattr(m.model, "_train_syncs", []))
    assert pending
    words = torch.cat([buf.view(torch.int32)[:: stride // 4] for buf, stride in pending]).cpu()
    m.model.raise_on_train_handoff_timeout()
    return words


def _forward_loss(m, batch, fused_loss, seed=None):
    """-> (named logits, loss, named loss parts) of one training forward; loss=None is the masked_bce path (one call per head)."""
    from music_transcription_amd import ops
    if seed is not None:
        torch.manual_seed(seed)
    mel, roll, lengths = batch
    heads = m.model_type == "cnn_rnn_large" and m.use_onset_offset_heads
    logits = m(mel.cuda(), return_all_heads=True) if heads else m(mel.cuda())
    named = {"logits." + k: v for k, v in logits.items()} if isinstance(logits, dict) else {"logits": logits}
    parts = {}
    if fused_loss:
        loss = m.compute_loss(logits, roll.cuda(), lengths, loss=_loss_config())
        parts["loss.parts"] = ops.heads_loss.last_parts
    else:
        terms, orig = [], ops.masked_bce

        def recording(*a, **k):
            terms.append(orig(*a, **k))
            return terms[-1]
        ops.masked_bce = recording
        try:
            loss = m.compute_loss(logits, roll.cuda(), lengths)
        finally:
            ops.masked_bce = orig
        assert len(terms) == (3 if heads else 1)
        parts["loss.parts"] = torch.stack([t.detach() for t in terms])
    return named, loss, parts


def _grads_and_stats(m):
    out = {}
    for n, p in m.model.named_parameters():
        out["grad." + n] = torch.zeros_like(p) if p.grad is None else p.grad.detach()
    for k, v in m.state_dict().items():
        if "running_" in k:
            out["bn." + k] = v.detach()
    return out


def _step_outputs(mta, case, batch, fused_loss, dropout=0.0, seed=None):
    mtype, (nm, H, L, B, T), kw = case
    m, _ = _model(mta, mtype, nm, H, L, seed=61, dropout=dropout, **kw)
    named, loss, parts = _forward_loss(m, batch, fused_loss, seed)
    loss.backward()
    out = {k: v.detach() for k, v in named.items()}
    out["loss"] = loss.detach().reshape(1)
    out.update(parts)
    out.update(_grads_and_stats(m))
    out["status"] = _status_words(m)
    return out


def _check(res, tag):
    for r in res:
        assert r["status"].tolist() == [0] * r["status"].numel(), (tag, r["status"].tolist())
    for k, v in res[0].items():                             # the control itself is finite
        assert bool(torch.isfinite(v.double()).all()), (tag, k)
    spreads = assert_fill_independent(res, tag=tag)
    print("\n[%s] control-to-control spread: max %.3g %s" % (tag, max(spreads.values()), {k: v for k, v in spreads.items() if v}))
    return spreads


@pytest.mark.parametrize("fused_loss", [False, True], ids=["bce", "heads_loss"])
@pytest.mark.parametrize("case", STEP_CASES, ids=_CASE_ID)
def test_step(mta, case, fused_loss):
    nm, H, L, B, T = case[1]
    batch = _batch(B, nm, T, 11)
    assert len(set(batch[2].tolist())) > 1 and int(batch[2].min()) < T                 # ragged lengths
    res = run_under_fills(lambda: _step_outputs(mta, case, batch, fused_loss))
    _check(res, _CASE_ID(case))
    if not fused_loss:
        assert float(res[0]["loss"]) > 0.0 and any(float(v.abs().max()) > 0.0 for k, v in res[0].items() if k.startswith("grad."))


@pytest.mark.parametrize("case", [STEP_CASES[1], STEP_CASES[3], STEP_CASES[5]], ids=_CASE_ID)
def test_step_with_dropout(mta, case):
    """Dropout on, the same torch seed in front of every forward: the kept sets must not change with the fill (the gradients would)."""
    nm, H, L, B, T = case[1]
    batch = _batch(B, nm, T, 12)
    res = run_under_fills(lambda: _step_outputs(mta, case, batch, False, dropout=0.3, seed=101))
    _check(res, "dropout " + _CASE_ID(case))
    with alloc_fill(0x00):
        other = _step_outputs(mta, case, batch, False, dropout=0.3, seed=999)
    assert any(not torch.equal(other[k].cpu(), res[0][k]) for k in res[0] if k.startswith("grad."))    # (the masks DO depend on the seed)


@pytest.mark.parametrize("case", [STEP_CASES[1], STEP_CASES[3], STEP_CASES[5]], ids=_CASE_ID)
def test_two_steps_in_flight(mta, case, monkeypatch):
    """The "ab" program of test_gpu_train_autograd.py: two forwards, then their backwards -- the first step leases the pooled
    workspace, the second cannot and gets fresh tensors (_FreshZeros for the zeroed-once regions): step_pool.acquire is recorded in
    every run, so both kinds of allocation are shown to run under every fill."""
    mtype, (nm, H, L, B, T), kw = case
    a, b = _pair(B, nm, T)
    rec = _acquisitions(monkeypatch)
    leased = []

    def fn():
        rec.clear()
        m, _ = _model(mta, mtype, nm, H, L, seed=62, **kw)
        r = _Hip(m)
        la, lb = r.loss(a), r.loss(b)
        busy = [e.busy for e in _pool_of(m).values()]
        la.backward()
        lb.backward()
        leased.append(([h for _, h, _ in rec], len({w for _, _, w in rec}), busy, [e.busy for e in _pool_of(m).values()]))
        out = _grads_and_stats(m)
        out["status"] = _status_words(m)
        return out
    res = run_under_fills(fn)
    assert leased == [([True, False], 2, [True], [False])] * 4, leased       # pooled + private workspace in each of the four runs
    _check(res, "ab " + _CASE_ID(case))


@pytest.mark.parametrize("case", [STEP_CASES[2], STEP_CASES[3], STEP_CASES[5]], ids=_CASE_ID)
def test_step_a_b_a_on_one_model(mta, case):
    """A, B (ten times the amplitude), A on ONE model with no optimizer step between, on a fresh model under 0x00, 0x00 again, 0xFF
    and 0x47: the third step leases the pooled workspace that B's step has used, "zeroed ONCE" regions included.  The spread is that
    of the two independent control FIRST steps; every third step (the control fills' too) and every poisoned first step is compared
    with the first control's first step under the rule of alloc_fill.mismatches -- bitwise where those two first steps agree."""
    mtype, (nm, H, L, B, T), kw = case
    a, b = _pair(B, nm, T)
    b = (b[0] * 10.0, b[1], b[2])
    firsts, thirds = [], []
    for byte in (0x00, 0x00, 0xFF, 0x47):
        with alloc_fill(byte):
            m, _ = _model(mta, mtype, nm, H, L, seed=63, **kw)
            runs = []
            for batch in (a, b, a):
                m.zero_grad(set_to_none=True)
                named, loss, _ = _forward_loss(m, batch, False)
                loss.backward()
                out = {k: v.detach().cpu().clone() for k, v in named.items()}
                out["loss"] = loss.detach().reshape(1).cpu()
                out.update({k: v.cpu().clone() for k, v in _grads_and_stats(m).items() if k.startswith("grad.")})
                runs.append(out)
            assert _status_words(m).tolist() == [0] * _status_words_count(m, 3)
            assert len(_pool_of(m)) == 1                                                   # one pooled workspace served all three
        assert not torch.equal(runs[0]["loss"], runs[1]["loss"])
        firsts.append(runs[0])
        thirds.append(runs[2])
    tag = "A, B, A " + _CASE_ID(case)
    # (mismatches labels its last two runs "0xFF" / "0x47": here they are the runs named in each message)
    bad, spreads = mismatches([firsts[0], firsts[1], firsts[2], firsts[3]])
    assert not bad, (tag, "first steps under 0xFF / 0x47", bad, {k: v for k, v in spreads.items() if v})
    bad, _ = mismatches([firsts[0], firsts[1], thirds[0], thirds[1]])
    assert not bad, (tag, "third steps under the two control fills against the first step", bad)
    bad, _ = mismatches([firsts[0], firsts[1], thirds[2], thirds[3]])
    assert not bad, (tag, "third steps under 0xFF / 0x47 against the control's first step", bad)


def _pool_of(m):
    net = m.model
    return net.__dict__.get("_bptt_parts" if type(net).__name__ == "CNNRNNModel" else "_train_ws", {})


def _status_words_count(m, steps):
    net = m.model
    per_step = 2 * net.num_layers if type(net).__name__ == "CNNRNNModel" else 2 * (net.num_layers + 1)
    return steps * per_step


# ------------------------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("nan_grad", [False, True], ids=["taken", "skipped"])
@pytest.mark.parametrize("case", [STEP_CASES[1], STEP_CASES[3]], ids=_CASE_ID)
def test_fused_clip_adam_ema_step(mta, case, nan_grad):
    """One mt_adam_clip_step_ema after a backward: parameters, both moments, the average and the returned {norm, taken} under every
    fill.  With one NaN gradient the step is skipped: parameters, moments and average are what they were, bit for bit."""
    mtype, (nm, H, L, B, T), kw = case
    batch = _batch(B, nm, T, 13)

    def fn():
        m, _ = _model(mta, mtype, nm, H, L, seed=64, **kw)
        opt = mta.make_optimizer(m, lr=1e-3, max_grad_norm=0.5, ema_decay=0.99)
        opt.zero_grad()
        _, loss, _ = _forward_loss(m, batch, False)
        loss.backward()
        opt._reattach_grad_views()
        if nan_grad:
            opt.g[opt.g.numel() // 2] = float("nan")
        before = {k: getattr(opt, k).detach().clone() for k in ("p", "m", "v", "ema")}
        stats = opt.step().detach().clone()
        out = {"adam." + k: getattr(opt, k).detach() for k in ("p", "m", "v", "ema")}
        out["adam.stats"] = stats
        out["status"] = _status_words(m)
        for k, v in before.items():
            same = torch.equal(v.view(torch.int32), out["adam." + k].view(torch.int32))
            assert same == nan_grad, (k, "a skipped step leaves everything unchanged" if nan_grad else "the step was not taken")
        return out
    res = run_under_fills(fn)
    for r in res:
        assert r["status"].tolist() == [0] * r["status"].numel()
        taken = r["adam.stats"][1].item()
        assert taken == (0.0 if nan_grad else 1.0), r["adam.stats"]
        for k in ("p", "m", "v", "ema"):
            assert bool(torch.isfinite(r["adam." + k]).all()), k
    if nan_grad:                                            # (the norm of a skipped step is the non-finite value itself: NaN == NaN bitwise)
        assert not bool(torch.isfinite(res[0]["adam.stats"][0]))
    spreads = assert_fill_independent(res, tag="adam " + _CASE_ID(case))
    print("\n[adam %s] control-to-control spread: max %.3g" % (_CASE_ID(case), max(spreads.values())))
