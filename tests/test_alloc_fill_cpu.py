"""tests/alloc_fill.py itself: the patched allocators fill every dtype the package uses, the originals come back, allocators that
promise contents are untouched, and the comparison rule reports a read of one unwritten element (and nothing else)."""
import pytest
import torch

from alloc_fill import BIG_FILL, NAN_FILL, alloc_fill, assert_fill_independent, mismatches, run_under_fills

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.uint8, torch.int32, torch.int64]
SHAPES = [(), (7,), (3, 5), (0,), (2, 0, 3)]


def _bytes(t):
    return torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage())


@pytest.mark.parametrize("byte", [0x00, NAN_FILL, BIG_FILL])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_every_allocator_fills_every_byte(dtype, byte):
    base = torch.zeros(4, 6, dtype=dtype)
    with alloc_fill(byte):
        made = [torch.empty(s, dtype=dtype) for s in SHAPES]
        made += [torch.empty(3, 5, dtype=dtype), torch.empty((3, 5), dtype=dtype), torch.empty(size=(3, 5), dtype=dtype)]
        made += [torch.empty_like(base), torch.empty_like(base.t()), torch.empty_like(base, dtype=dtype)]
        made += [torch.empty_strided((3, 4), (1, 5), dtype=dtype), torch.empty_strided((2, 3), (6, 2), dtype=dtype)]     # gaps in the storage
        made += [base.new_empty(5), base.new_empty((2, 3)), base.new_empty((), dtype=dtype)]
    for t in made:
        assert t.dtype == dtype
        b = _bytes(t)
        assert b.numel() == t.untyped_storage().nbytes()
        assert bool((b == byte).all()), (t.shape, t.stride())
    strided = made[-5]
    assert strided.shape == (3, 4) and strided.stride() == (1, 5) and not strided.is_contiguous()
    assert made[0].dim() == 0 and made[3].numel() == 0


def test_fill_values_are_what_the_tests_assume():
    with alloc_fill(NAN_FILL):
        for dt in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
            assert bool(torch.isnan(torch.empty(5, dtype=dt)).all())
        for dt in (torch.int32, torch.int64):
            assert torch.empty(5, dtype=dt).tolist() == [-1] * 5
        assert torch.empty(2, dtype=torch.uint8).tolist() == [255, 255]
    with alloc_fill(BIG_FILL):
        assert abs(float(torch.empty((), dtype=torch.float32)) - 51015.28) < 0.01
        assert float(torch.empty((), dtype=torch.bfloat16)) == 50944.0
        assert abs(float(torch.empty((), dtype=torch.float16)) - 7.28) < 0.01
        assert int(torch.empty((), dtype=torch.int32)) == 1195853639


def test_originals_are_restored_after_exit_and_after_an_exception():
    orig = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with alloc_fill(NAN_FILL):
        assert torch.empty is not orig[0] and torch.Tensor.new_empty is not orig[3]
        with alloc_fill(BIG_FILL):                                        # nesting restores the outer patch, then the originals
            assert int(torch.empty((), dtype=torch.uint8)) == BIG_FILL
        assert int(torch.empty((), dtype=torch.uint8)) == NAN_FILL
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig
    with pytest.raises(KeyError):
        with alloc_fill(NAN_FILL):
            raise KeyError("body raises")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig


def test_allocators_that_promise_contents_are_untouched():
    z, f = torch.zeros, torch.full
    with alloc_fill(NAN_FILL):
        assert torch.zeros is z and torch.full is f
        assert torch.zeros(3, 4).abs().sum() == 0 and bool((torch.full((5,), 2.5) == 2.5).all())
        assert torch.zeros_like(torch.ones(3)).tolist() == [0.0] * 3 and torch.ones(2, dtype=torch.int32).tolist() == [1, 1]
        assert torch.arange(4).tolist() == [0, 1, 2, 3]
        x = torch.ones(6)
        assert x.new_zeros(3).tolist() == [0.0] * 3 and x.clone().tolist() == [1.0] * 6
        assert torch.equal(torch.ones(3, 3) @ torch.ones(3, 3), torch.full((3, 3), 3.0))      # results of ops are not "empty"


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _toy(read_unwritten, dtype=torch.float32):
    """Sums 8 values through a 9-element scratch buffer; the buggy variant's loop bound is one too far."""
    def fn():
        x = torch.arange(1, 9, dtype=torch.float32) * 0.5              # (max 4.0: below 0x47 in every float type)
        buf = torch.empty(9, dtype=dtype)
        buf[:8] = x.to(dtype)
        n = 9 if read_unwritten else 8
        count = torch.empty(3, dtype=torch.int64)
        count[:2] = torch.tensor([4, 5])
        return {"sum": buf[:n].float().sum().reshape(1), "max": buf[:n].float().max().reshape(1), "count": count[: 3 if read_unwritten else 2]}
    return fn


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[-1])
def test_a_read_of_one_unwritten_element_is_reported_under_both_fills(dtype):
    res = run_under_fills(_toy(True, dtype))
    bad, spreads = mismatches(res)
    assert spreads == {"sum": 0.0, "max": 0.0, "count": 0.0}                  # the control runs agree: the bitwise rule applies
    for name in ("sum", "count"):
        assert f"{name} [0xFF]" in bad and f"{name} [0x47]" in bad, bad
    assert "max [0x47]" in bad, bad                                          # 0x47: what a NaN-swallowing fmax would hide under 0xFF
    with pytest.raises(AssertionError, match="depends on uninitialised memory"):
        assert_fill_independent(res, tag="toy")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[-1])
def test_the_same_function_without_the_read_passes(dtype):
    res = run_under_fills(_toy(False, dtype))
    assert mismatches(res)[0] == {}
    assert assert_fill_independent(res) == {"sum": 0.0, "max": 0.0, "count": 0.0}


def test_nan_swallowing_reader_is_caught_by_the_finite_fill_only():
    def fn():
        buf = torch.empty(4)
        buf[:3] = torch.tensor([1.0, -2.0, 3.0])
        return {"relu_max": torch.fmax(buf, torch.zeros(4)).max().reshape(1)}      # fmax drops the NaN of 0xFF
    bad, _ = mismatches(run_under_fills(fn))
    assert list(bad) == ["relu_max [0x47]"], bad


def test_spread_rule_where_the_control_runs_differ():
    calls = []

    def fn(extra):
        def run():
            i = len(calls)
            calls.append(i)
            jitter = (0.0, 1e-6, 1.5e-6, -1e-6)[i % 4]                         # what float atomics do to a sum
            return {"g": torch.tensor([1.0 + jitter + (extra if i % 4 >= 2 else 0.0), -0.5])}
        return run
    assert mismatches(run_under_fills(fn(0.0)))[0] == {}                     # inside 2 x spread
    calls.clear()
    bad, spreads = mismatches(run_under_fills(fn(1e-5)))                     # outside 2 x spread (and inside the 1e-3 cap)
    assert set(bad) == {"g [0xFF]", "g [0x47]"} and 0.5e-6 < spreads["g"] < 2e-6
    calls.clear()
    bad, _ = mismatches(run_under_fills(fn(float("nan"))))
    assert "NaN/Inf where the control has none" in bad["g [0xFF]"]


def test_masks_must_stay_below_one_half_and_hide_only_what_they_cover():
    def fn():
        out = torch.empty(2, 4, dtype=torch.int32)
        out[0] = torch.arange(4, dtype=torch.int32)
        out[1, :1] = 7                                                        # out[1, 1:] is unspecified by this toy's contract
        return {"out": out}
    res = run_under_fills(fn)
    assert set(mismatches(res)[0]) == {"out [0xFF]", "out [0x47]"}
    keep = torch.ones(2, 4, dtype=torch.bool)
    keep[1, 1:] = False
    assert mismatches(res, {"out": keep})[0] == {}
    keep[0, 3] = False                                                        # 4 of 8 masked: refused
    with pytest.raises(AssertionError, match="below one half"):
        mismatches(res, {"out": keep})
