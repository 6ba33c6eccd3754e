"""GPU parity tests for CNNRNNModelLarge: op-level (conv, attention pieces) and whole-model against the
CPU oracle and the reference-generated goldens."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from oracle import model_ref as R


@pytest.fixture(scope="module")
def mta():
    import music_transcription_amd as m
    return m


def _mel_in(B, nm, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, nm, T, generator=g) * 60.0 - 70.0 + 10.0 * torch.randn(B, 1, nm, 1, generator=g))


def _bf(x):
    return x.bfloat16().float()


@pytest.mark.parametrize("C1,C2,Cout,KH,pool,F,T", [(32, 0, 64, 3, 0, 20, 37), (64, 32, 64, 3, 1, 20, 37), (64, 0, 128, 3, 0, 10, 50),
                                                    (128, 64, 128, 3, 0, 9, 33), (128, 0, 256, 7, 1, 12, 40), (128, 0, 256, 7, 1, 7, 16)])
def test_conv_cl_matches_torch(mta, C1, C2, Cout, KH, pool, F, T):
    """mt_conv_cl_bf16 on random bf16 data against torch at the bf16 output rounding, and the two output modes against each other.
    (Every instantiation, epilogue and operand type against an exact CPU reference, with guard bands: tests/test_gpu_conv.py,
    test_conv_cl_every_setting.)"""
    from music_transcription_amd._lib import lib, check, ptr, stream_ptr
    g = torch.Generator().manual_seed(C1 + Cout + KH)
    B = 2
    x = _bf(torch.randn(B, C1, F, T, generator=g))
    s = _bf(torch.randn(B, C2, F, T, generator=g)) if C2 else None
    w = _bf(torch.randn(Cout, C1, KH, 3, generator=g) / np.sqrt(C1 * KH * 3))
    ws = _bf(torch.randn(Cout, C2, 1, 1, generator=g) / np.sqrt(max(C2, 1))) if C2 else None
    bias = torch.randn(Cout, generator=g)
    ref = TF.conv2d(x, w, bias, padding=(KH // 2, 1))
    if C2:
        ref = ref + TF.conv2d(s, ws)
    ref = torch.relu(ref)
    if pool:
        ref = R.pool_f2(ref)
    Fo = ref.shape[2]
    xa = x.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    sa = s.permute(0, 2, 3, 1).contiguous().bfloat16().cuda() if C2 else None
    wk = w.permute(0, 2, 3, 1).reshape(Cout, -1)
    if C2:
        wk = torch.cat([wk, ws.reshape(Cout, C2)], 1)
    wk = wk.contiguous().bfloat16().cuda()
    out = torch.zeros(B, Fo, T, Cout, dtype=torch.bfloat16, device="cuda")
    bias_d = bias.cuda()
    check(lib.mt_conv_cl_bf16(ptr(xa), ptr(sa), ptr(wk), ptr(bias_d), ptr(out), B, F, T, C1, C2, Cout, KH, 1, pool, 0, 0, stream_ptr()))
    got = out.float().cpu().permute(0, 3, 1, 2)
    err = (got - ref).abs().max().item()
    assert err < 2e-2 * max(1.0, ref.abs().max().item()), err          # bf16 output rounding
    # GEMM-row output mode: X[(t*B+b)][fo*Cout+co]
    ld = Fo * Cout
    X = torch.zeros(T * B, ld, dtype=torch.bfloat16, device="cuda")
    check(lib.mt_conv_cl_bf16(ptr(xa), ptr(sa), ptr(wk), ptr(bias_d), ptr(X), B, F, T, C1, C2, Cout, KH, 1, pool, 1, ld, stream_ptr()))
    assert torch.equal(X.view(T, B, Fo, Cout).permute(1, 2, 0, 3).contiguous(), out)


def test_attention_pieces(mta):
    """(Both operand types, more shapes, wide rows and per-element bounds: tests/test_gpu_attn.py.)"""
    from music_transcription_amd._lib import lib, check, ptr, stream_ptr
    g = torch.Generator().manual_seed(0)
    rows, T, Tp = 37, 50, 64
    S = torch.randn(rows, Tp, generator=g) * 30.0
    P = torch.full((rows, Tp), 7.0, dtype=torch.bfloat16, device="cuda")
    S_d = S.cuda()
    check(lib.mt_attn_softmax_clamped(ptr(S_d), Tp, ptr(P), Tp, T, rows, 0.25, 10.0, stream_ptr()))
    ref = torch.softmax(torch.clamp(S[:, :T] * 0.25, -10, 10), -1)
    assert (P[:, :T].float().cpu() - ref).abs().max().item() < 4e-3 and float(P[:, T:].abs().max()) == 0.0
    # layernorm(residual + proj)
    n, ld = 96, 128
    a, b = torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g)
    gam, bet = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y = torch.zeros(rows, ld, dtype=torch.bfloat16, device="cuda")
    a_d, b_d, g_d, be_d = a.cuda(), b.cuda(), gam.cuda(), bet.cuda()      # keep the device buffers alive across the async launch
    check(lib.mt_layernorm_residual(ptr(a_d), n, ptr(b_d), n, ptr(g_d), ptr(be_d), ptr(y), ld, rows, n, 1e-6, stream_ptr()))
    torch.cuda.synchronize()
    ref = TF.layer_norm(a + b, (n,), gam, bet, 1e-6)
    assert (y[:, :n].float().cpu() - ref).abs().max().item() < 3e-2 and float(y[:, n:].abs().max()) == 0.0


@pytest.mark.parametrize("B,T,heads,dp,dt", [(2, 938, 8, 192, "f16"), (3, 100, 2, 64, "bf16"), (1, 65, 1, 128, "f16"), (2, 937, 3, 192, "f16")])
def test_attention_fused_matches_torch(mta, B, T, heads, dp, dt):
    """csrc/attn_fused.hip against the module's own arithmetic (cnn_rnn_model.py:118-139) in fp32 on the same 16-bit q, k, v:
    scale, clamp +-10 BEFORE the softmax (a third of the scores here are at the clamp), softmax over all T keys (no mask), P V.
    Rows whose query index is past T are not written; every other output column of the row is.
    (Per-element bounds, every sub-block mask and query-block edge, wide rows, NaN pads: tests/test_gpu_attn.py.)"""
    from music_transcription_amd._lib import lib, check, ptr, stream_ptr, DT_F16, DT_BF16
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    g = torch.Generator().manual_seed(B * 1000 + T)
    Ca, ld3, ldo = heads * dp, 3 * heads * dp, heads * dp
    scale = float(dp) ** -0.5
    qkv = (torch.randn(T * B, ld3, generator=g) * 1.5).to(tdt)
    qkv[:, :Ca] *= 3.0                                                    # |q k| * scale reaches +-10 and beyond (14 % of the scores)
    Tp = (T + 63) // 64 * 64
    dpr = (dp + 127) // 128 * 128
    qd = qkv.cuda()
    VT = torch.zeros(B * heads * dpr * Tp, dtype=tdt, device="cuda")
    ao = torch.full((T * B, ldo), 7.0, dtype=tdt, device="cuda")
    st = stream_ptr()
    code = DT_F16 if dt == "f16" else DT_BF16
    check(lib.mt_attn_transpose_v(ptr(qd), ld3, 2 * Ca, ptr(VT), B, T, Tp, heads, dp, st))
    check(lib.mt_attn_fused_clamped(ptr(qd), ld3, Ca, ptr(VT), Tp, B, T, heads, dp, scale, 10.0, ptr(ao), ldo, code, st))
    torch.cuda.synchronize()
    x = qkv.float().view(T, B, 3, heads, dp)
    q, k, v = (x[:, :, i].permute(1, 2, 0, 3) for i in range(3))          # (B, heads, T, dp)
    sc = torch.clamp(q @ k.transpose(-1, -2) * scale, -10.0, 10.0)
    assert float((sc.abs() >= 10.0).float().mean()) > 0.05
    ref = (torch.softmax(sc, -1) @ v).permute(2, 0, 1, 3).reshape(T * B, ldo)
    got = ao.float().cpu()
    tol = (4e-3 if dt == "f16" else 3e-2) * float(ref.abs().max())
    assert float((got - ref).abs().max()) < tol, (float((got - ref).abs().max()), tol)


@pytest.mark.parametrize("tag", ["large_a", "large_b"])
def test_large_small_configs_vs_reference_golden(mta, golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "small_models.npz"))
    nm, hs, nl, B, T, wseed, xseed = [int(v) for v in z[f"{tag}_cfg"]]
    sd = R.set_bn_flat(R.make_state_dict("cnn_rnn_large", nm, hs, nl, wseed), z[f"{tag}_bn"])
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=nm, hidden_size=hs, num_layers=nl, device="cuda")
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = _mel_in(B, nm, T, xseed)
    with torch.no_grad():
        got = model(x.cuda(), return_all_heads=True)
        model.model.raise_on_handoff_timeout(B, T)
        emu = R.cnnrnn_large_forward(sd, x, return_all_heads=True, o=R.Opts(gemm_f16=True))
        frame_only = model(x.cuda())
    assert torch.equal(frame_only, got["frame"])
    for k in ("frame", "onset", "offset"):
        gk = got[k].cpu()
        assert gk.shape == (B, 88, T)
        assert (gk - emu[k]).abs().max().item() < 1e-2, k        # same bf16 rounding points; accumulation order differs
        assert (gk - torch.from_numpy(z[f"{tag}_{k}"])).abs().max().item() < 3e-2, k   # vs the fp32 reference (bf16 operands)


@pytest.mark.parametrize("hidden,B", [(32, 40), (64, 70)])
def test_large_with_interleaved_batch_groups(mta, hidden, B):
    """CNNRNNModelLarge over 2 - 3 batch groups with a ragged last one (both recurrences interleave them inside one persistent
    launch each): against the oracle with the same rounding points, all three heads, and chunk for chunk against a forward over a
    slice of the batch."""
    nm, L, T = 32, 2, 24
    sd = R.make_state_dict("cnn_rnn_large", nm, hidden, L, seed=hidden + 1)
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=nm, hidden_size=hidden, num_layers=L, device="cuda").eval()
    model.load_state_dict(sd, strict=True)
    x = _mel_in(B, nm, T, B)
    with torch.no_grad():
        got = model(x.cuda(), return_all_heads=True)
        model.model.raise_on_handoff_timeout(B, T)
        emu = R.cnnrnn_large_forward(sd, x, return_all_heads=True, o=R.Opts(gemm_f16=True))
        part = model(x[33:38].contiguous().cuda(), return_all_heads=True)
        model.model.raise_on_handoff_timeout(5, T)
    for k in ("frame", "onset", "offset"):
        gk = got[k].cpu()
        assert gk.shape == (B, 88, T) and torch.isfinite(gk).all()
        assert (gk - emu[k]).abs().max().item() < 1e-2, k
        assert (part[k].cpu() - gk[33:38]).abs().max().item() < 5e-3, k


def test_large_variants_vs_reference_golden(mta, golden_dir):
    z = np.load(os.path.join(golden_dir, "small_models.npz"))
    x = _mel_in(2, 32, 30, 6)
    for seed, att, heads, key in ((12, False, True, "large_noattn_logits"), (13, True, False, "large_noheads_logits")):
        sd = R.set_bn_flat(R.make_state_dict("large", 32, 16, 2, seed, use_attention=att, use_heads=heads), z[key.replace("_logits", "_bn")])
        model = mta.TranscriptionModel("large", n_mels=32, hidden_size=16, num_layers=2, device="cuda",
                                       use_attention=att, use_onset_offset_heads=heads).eval()
        model.load_state_dict(sd, strict=True)
        with torch.no_grad():
            got = model(x.cuda()).cpu()
        ref = torch.from_numpy(z[key])
        # tiny config (48 features under the LayerNorm): relative bound, the no-heads fc sees |logit| up to ~2
        assert (got - ref).abs().max().item() < 5e-2 * max(1.0, ref.abs().max().item()), key


def test_large_canonical_b2_t938_vs_reference_golden(mta, golden_dir):
    """canonical 320/512/3 at B = 2, T = 938 (what main.py's chunks produce): strided frame logits + summary statistics."""
    c = np.load(os.path.join(golden_dir, "canonical_models.npz"))
    tag = "large_938"
    nm, hs, nl, B, T, wseed, xseed = [int(v) for v in c[f"{tag}_cfg"]]
    sd = R.set_bn_flat(R.make_state_dict("cnn_rnn_large", nm, hs, nl, wseed), c[f"{tag}_bn"])
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=nm, hidden_size=hs, num_layers=nl, device="cuda").eval()
    model.load_state_dict(sd, strict=True)
    x = _mel_in(B, nm, T, xseed)
    with torch.no_grad():
        got = model(x.cuda()).cpu().numpy()
        model.model.raise_on_handoff_timeout(B, T)
    assert got.shape == (B, 88, T)
    err = np.abs(got[:, ::5, ::7] - c[f"{tag}_sample"]).max()
    assert err < 1e-2, err                                             # f16 operands (observed ~1e-3)
    st = c[f"{tag}_stats"]
    assert abs(got.mean() - st[0]) < 2e-3 and abs(got.std() - st[1]) < 2e-3


def test_large_full_size_b16_independence_determinism_and_fused_projection(mta):
    """BASELINE configs[2] shape (CNNRNNModelLarge, batch 16 x 30 s): chunks are independent (no padding arises), the
    forward is run-to-run deterministic, and the fused-input-projection path (main layers 1.. project inside the
    recurrence, mt_cnnrnn_large_weights.main_w_ihx) gives the same logits as the GEMM path."""
    from oracle import frontend_ref as FR
    sd = R.make_state_dict("cnn_rnn_large", 320, 512, 3, seed=3)
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=320, hidden_size=512, num_layers=3, device="cuda").eval()
    model.load_state_dict(sd, strict=True)
    wave = torch.from_numpy(FR.synth_audio(4, 480000, seed=8)).cuda()
    wave = torch.cat([wave * s for s in (1.0, 0.5, 0.25, 0.8)], 0)                               # 16 distinct chunks
    mel, cmax = mta.MelFrontend(16000, 320, 512, "cuda")(wave, clamp=True)
    with torch.no_grad():
        full = model(mel, return_all_heads=True)
        full = {k: v.clone() for k, v in full.items()}
        again = model(mel, return_all_heads=True)
        assert all(torch.equal(full[k], again[k]) for k in full)                                 # deterministic
        perm = torch.tensor([5, 0, 11, 3])
        sub = model(mel[perm].contiguous(), return_all_heads=True)                               # other batch size, other positions
        for k in full:
            assert (sub[k] - full[k][perm]).abs().max().item() < 2e-3, k                         # GEMM tile order may differ with M
        model.model.fuse_input_projection = True
        fused = model(mel, return_all_heads=True)
        model.model.raise_on_handoff_timeout(16, 938)
        for k in full:
            assert torch.isfinite(fused[k]).all() and (fused[k] - full[k]).abs().max().item() < 3e-3, k
    assert float(full["frame"].std()) > 1e-3


def test_large_canonical_vs_reference_golden(mta, golden_dir):
    c = np.load(os.path.join(golden_dir, "canonical_models.npz"))
    tag = "large_937"
    nm, hs, nl, B, T, wseed, xseed = [int(v) for v in c[f"{tag}_cfg"]]
    sd = R.set_bn_flat(R.make_state_dict("cnn_rnn_large", nm, hs, nl, wseed), c[f"{tag}_bn"])
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=nm, hidden_size=hs, num_layers=nl, device="cuda").eval()
    model.load_state_dict(sd, strict=True)
    x = _mel_in(B, nm, T, xseed)
    with torch.no_grad():
        d = model(x.cuda(), return_all_heads=True)
        model.model.raise_on_handoff_timeout(B, T)
    for k, key in (("frame", f"{tag}_sample"), ("onset", f"{tag}_onset_sample"), ("offset", f"{tag}_offset_sample")):
        err = np.abs(d[k].cpu().numpy()[:, ::5, ::7] - c[key]).max()
        assert err < 3e-2, (k, err)


# ------------------------------------------------------------------ BASELINE configs[4] at the model's full size
CORPUS_LOGIT_TOL = 0.06        # full chunks vs fp32: 3 x the largest |dlogit| the f16 path shows at this size and weight scale (0.020 of 15)
CORPUS_LOGIT_TOL_TAIL = 0.15   # zero-padded tail chunks vs fp32: the clamp floor (max - 80 dB, one constant over the silent part) rounds to f16 as ONE
                               # systematic offset, not as noise: the oracle with the same f16 rounding points is itself 0.09 - 0.12 from fp32 there
                               # (0.013 on full chunks), worst flipped cell 0.043 from the threshold
CORPUS_LOGIT_TOL_EMU = 0.01    # every chunk vs the oracle with the HIP path's f16 rounding points (the mel differs by <= 5e-2 dB between the two)


def test_corpus_shard_full_size_large_matches_oracle_pipeline(mta):
    """corpus.transcribe_shard -- slab assembly ACROSS recordings, three slabs on two streams, logits held per slab, notes and F1 on
    the device -- with CNNRNNModelLarge 320/512/3 (main.py:16-20's model) on two recordings / five 30 s chunks, against the oracle
    pipeline of main.py:60-100 (chunking), :103-130 (mel per chunk), the model, :153-159 (threshold), :164-186 (concatenation),
    :189-226 (notes): the rolls are equal except cells whose oracle logit is within the stated tolerance of the threshold -- against
    the fp32 oracle and against the oracle with the f16 rounding points -- and the notes are the reference's run-length over that
    roll.  Weights: trained-scale logits (N(-5, 3), ~5 % active cells) with the recurrence gain left at 1: with W_hh x 3 the silent
    tail of a zero-padded chunk is a chaotic regime in which the f16-emulating ORACLE is 0.8 - 1.4 away from fp32 (measured), i.e. no
    statement about the kernels could be made there."""
    from oracle import frontend_ref as FR
    from music_transcription_amd import corpus
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    durs = [41.0, 65.0]                                                # 2 + 3 chunks; both last chunks zero-padded in the waveform domain
    waves = [FR.synth_audio(1, int(16000 * d), seed=70 + i)[0] for i, d in enumerate(durs)]
    chunks = []
    for w in waves:
        n = -(-len(w) // 480000)
        c = np.zeros(n * 480000, np.float32); c[:len(w)] = w
        chunks.append(c.reshape(n, 480000))
    mel_ref = torch.from_numpy(np.concatenate([FR.audio_to_mel(c, 16000, 320, 512)[None] for rec in chunks for c in rec]))   # batch-1 clamp per chunk
    mel_ref = mel_ref.reshape(5, 1, 320, 938)
    sd0 = R.make_state_dict("cnn_rnn_large", 320, 512, 3, seed=11)
    sd, _ = R.trained_scale_state_dict(sd0, "cnn_rnn_large", mel_ref[:1], w_hh_gain=1.0)
    with torch.no_grad():
        ref = R.forward(sd, mel_ref, "cnn_rnn_large", o=R.Opts(fast_lstm=True))     # fp32 (eval-mode BatchNorm: batch-independent)
        emu = R.forward(sd, mel_ref, "cnn_rnn_large", o=R.Opts(gemm_f16=True))      # the HIP path's rounding points
    model = mta.TranscriptionModel("cnn_rnn_large", n_mels=320, hidden_size=512, num_layers=3, device="cuda").eval()
    model.load_state_dict(sd, strict=True)
    dev_chunks = {i: torch.from_numpy(c).cuda() for i, c in enumerate(chunks)}
    g = torch.Generator().manual_seed(5)
    truth = {i: (torch.rand(88, len(c) * 938, generator=g) < 0.05).float() for i, c in enumerate(chunks)}
    res = corpus.transcribe_shard(model, [0, 1], lambda i: dev_chunks[i], n_mels=320, device="cuda", batch=2, streams=2, threshold=0.5,
                                  want_notes=True, reference_roll_of=lambda i, T_total: truth[i].cuda())
    assert res["chunks"] == 5 and res["slabs"] == 3 and res["finite"] and res["chunks_per_recording"] == {0: 2, 1: 3}
    fs, a, flips = 16000 / 512, 0, [0, 0]
    for i, rec in enumerate(chunks):
        n = len(rec)
        flat = lambda x: x[a:a + n].permute(1, 0, 2).reshape(88, n * 938).numpy()
        lg, lge = flat(ref), flat(emu)
        want = (lg > 0).astype(np.uint8)                                  # sigmoid(x) > 0.5
        got = np.zeros_like(want)
        for p, s, e in res["notes"][i]:
            got[p - 21, int(round(s * fs)):int(round(e * fs))] = 1
        tol = np.full(n * 938, CORPUS_LOGIT_TOL, np.float32)
        tol[(n - 1) * 938:] = CORPUS_LOGIT_TOL_TAIL                       # the recording's last chunk is the zero-padded one
        bad, bad_e = got != want, got != (lge > 0)
        flips[0] += int(bad.sum()); flips[1] += int(bad_e.sum())
        assert bad.mean() < 5e-3 and want.sum() > 1000, (i, bad.mean(), want.sum())
        assert not (bad & (np.abs(lg) >= tol[None, :])).any(), (i, float(np.abs(lg)[bad].max()))               # only cells at the threshold may differ
        assert not (bad_e & (np.abs(lge) >= CORPUS_LOGIT_TOL_EMU)).any(), (i, float(np.abs(lge)[bad_e].max()))
        assert res["notes"][i] == R.pianoroll_to_notes(got, fs) and len(res["notes"][i]) > 50                # the reference's run-length, note for note
        if not bad.any():
            assert res["notes"][i] == R.pianoroll_to_notes(want, fs)
        assert abs(res["f1"][i] - R.f1_binary(truth[i].numpy(), got)) < 1e-9
        a += n
    print(f"\n[corpus full size] cells flipped of {88 * 5 * 938}: {flips[0]} against the fp32 oracle, {flips[1]} against the f16-emulating oracle")
