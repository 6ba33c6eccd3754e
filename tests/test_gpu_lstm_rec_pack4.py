"""The plain inference recurrence after its register and address diet (csrc/lstm.hip).  The diet was made to fit FOUR workgroups on
a compute unit (96 registers); that packing is a measured loss and does not ship (profiles/lstm_pack4_*.txt), the leaner kernel does, at
three per CU.  It changed how the h gather is addressed (one buffer per (step, direction) image, k-steps in the immediate offset), where
the f16 gate pre-activations are read (behind the reduce barrier), where the cell states of interleaved batch groups live (LDS) and how
the poll loop leaves -- not one arithmetic operation.  So the outputs must be what they were: checked here against the float64 step model
of lstm_rec_ref.py with exactly the tolerances of test_gpu_lstm_rec.py (imported, not re-stated), at the smallest shapes that reach every
touched path:

  * H = 512 (NKSW = 8: two address registers per gather, the second 4 KB behind the first);
  * T = 5, as few steps as show every step-to-step path, and T = 8, where the six-slot gx ring wraps even with ONE batch group
    (with NG groups a step is NG slots: T = 5 wraps it for NG >= 2);
  * B = 32 (NG = 1), B = 128 (NG = 4), B = 40 (NG = 2 with a ragged second group of 8 rows); both directions are one launch;
  * gx as f16 (the instances of the default schedule) and as f32 (same code, other loader block size).

And the residency accounting (csrc/residency.hip) follows the occupancy query by itself: a launch of 128 workgroups at three per CU holds
43 CUs, and six plain recurrences in flight are admitted (6 x 128 / 3 = 256 CUs: the chip, not more)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_rec_ref as R  # noqa: E402
import test_gpu_lstm_rec as base  # noqa: E402  (helpers and tolerances: TOL_H_MAX / TOL_H_MEAN inside _check_h)

pytestmark = pytest.mark.gpu

CASES = [(512, 32, 5), (512, 128, 5), (512, 40, 5), (512, 32, 8), (512, 128, 8), (512, 40, 8)]     # (H, B, T)


@pytest.fixture(scope="module")
def mta():
    import __graft_entry__ as ge
    ge.build()
    import music_transcription_amd as m
    return m


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("entry", ["g16", "ex"])
def test_pack4_outputs_unchanged(mta, entry, case):
    """h of every step, both directions, against the kernel-rounded float64 model (base._check_h: TOL_H_MAX, TOL_H_MEAN and the exact-model
    bound of test_gpu_lstm_rec.py); two runs bit-equal"""
    base._inference(entry, case, entry == "g16")


def test_pack4_residency_follows_occupancy_and_six_in_flight(mta):
    """One plain H = 512 recurrence of one batch group (128 workgroups) is charged 128 / 3 = 43 CUs -- workgroups / the occupancy query's
    workgroups per CU, no constant -- and six of them on six streams are all admitted.  Read through mt_persistent_cus_in_flight, which reports what
    the launches pending on OTHER streams hold."""
    from music_transcription_amd._lib import lib, check
    H, B, T = 512, 32, 256                                                # (0.4 ms per launch: still pending when the host asks)
    dev = "cuda"
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    per = 43                                                              # round(128 workgroups / 3 per CU)
    assert 6 * 128 <= 3 * ncu
    gx = torch.zeros(lib.mt_lstm_gx_bytes(B, T, H) // 2, dtype=torch.uint8, device=dev)           # f16 gx: half of the f32 bytes
    whh = torch.zeros(2 * 4 * H * H, dtype=torch.float32, device=dev)
    streams = [torch.cuda.Stream() for _ in range(6)]
    hx = [torch.empty(lib.mt_lstm_hx_bytes(B, T, H), dtype=torch.uint8, device=dev) for _ in streams]
    sync = [torch.zeros(lib.mt_lstm_sync_bytes(B, H), dtype=torch.uint8, device=dev) for _ in streams]
    probe = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert lib.mt_persistent_cus_in_flight(probe.cuda_stream) == 0
    seen = []
    for s_, h_, y_ in zip(streams, hx, sync):
        # (check raises on a refused admission: all six must pass)
        check(lib.mt_lstm_bidir_fwd_ex(gx.data_ptr(), whh.data_ptr(), h_.data_ptr(), y_.data_ptr(), y_.numel(), B, T, H, base.GX_F16, s_.cuda_stream))
        seen.append(lib.mt_persistent_cus_in_flight(probe.cuda_stream))
    torch.cuda.synchronize()
    print("MEASURE CUs in flight after each of six launches:", seen)
    assert seen[0] == per, seen                                           # the first launch, alone and still pending
    assert all(0 <= v <= per * (i + 1) for i, v in enumerate(seen)), seen                         # (launches that have drained hold nothing)
    assert lib.mt_persistent_cus_in_flight(probe.cuda_stream) == 0
    for y_ in sync:
        assert int(y_[:4].view(torch.int32).item()) == 0, "hand-off timeout"
    for h_ in hx:                                                         # zero weights, zero gx: h = sigmoid(0) tanh(c) != poison, finite
        hv = h_.view(torch.float16)
        assert bool(torch.isfinite(hv).all().item())
