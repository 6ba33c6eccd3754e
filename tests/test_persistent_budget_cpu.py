"""The admission arithmetic of persistent launches with two workgroup sets (csrc/residency.hip, mt_persistent_fits), without a device:
launches that hold need[i] CUs each and would take surplus[i] more when wide fit a device iff sum(need) + max(surplus) <= CUs, because at
most ONE launch is wide at a time.  H = 512: a set is 128 workgroups at three per CU (tests/test_kernel_budget_pack4_cpu.py pins three)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from music_transcription_amd import _lib
    return _lib.lib


def _fits(lib, need, surplus, ncu):
    n = len(need)
    return lib.mt_persistent_fits((C.c_double * n)(*need), (C.c_double * n)(*surplus) if surplus is not None else None, n, ncu)


def test_budget_of_launches_with_two_sets(lib):
    ncu, per = 256, 128 / 3                              # MI355X; CUs of one set at H = 512
    assert 86 + 3 * 43 == 215 <= ncu                     # the default schedule in whole CUs: one wide launch, three narrow
    for streams in range(1, 6):                          # 1 .. 5 streams of such launches: admitted (five: 6 x 42.67 = 256 exactly)
        assert _fits(lib, [per] * streams, [per] * streams, ncu) == 1, streams
    assert _fits(lib, [per] * 6, [per] * 6, ncu) == 0    # the sixth is refused
    assert _fits(lib, [per] * 6, [0.0] * 6, ncu) == 1    # six launches with ONE set (one batch group each) still fit, as before
    assert _fits(lib, [per] * 6, None, ncu) == 1
    assert _fits(lib, [per] * 7, None, ncu) == 0
    # one surplus counts, the largest: a small launch's surplus beside a large one's
    assert _fits(lib, [100.0, 100.0], [56.0, 10.0], ncu) == 1
    assert _fits(lib, [100.0, 100.0], [57.0, 10.0], ncu) == 0
    assert _fits(lib, [100.0, 100.0], [10.0, 57.0], ncu) == 0
    # forced wide (test hook): the surplus is part of the need, three such launches fill the device
    assert _fits(lib, [2 * per] * 3, [0.0] * 3, ncu) == 1
    assert _fits(lib, [2 * per] * 4, [0.0] * 4, ncu) == 0
    assert _fits(lib, [], None, ncu) == 1
