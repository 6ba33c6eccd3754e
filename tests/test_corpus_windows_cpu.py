"""corpus.plan_groups (host integers only): how transcribe_shard_windows groups the recordings of a shard."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def corpus():
    import __graft_entry__ as ge
    ge.build()
    from music_transcription_amd import corpus as c
    return c


def _bytes(group, frames, heads):
    return heads * len(group) * 88 * max(frames[k] for k in group) * 4


def _check(groups, windows, frames, gw, gb, heads):
    assert [k for g in groups for k in g] == list(range(len(windows)))          # every recording once, in order
    assert all(len(g) >= 1 for g in groups)
    for n, g in enumerate(groups):
        w = sum(windows[k] for k in g)
        if len(g) > 1:
            assert w - windows[g[-1]] < gw                  # it was still open before its last recording
            assert _bytes(g, frames, heads) <= gb
        if n + 1 < len(groups):                             # it closed for a reason: full, or the next recording did not fit
            assert w >= gw or _bytes(g + [groups[n + 1][0]], frames, heads) > gb


def test_hand_cases(corpus):
    pg = corpus.plan_groups
    assert pg([], [], 4) == []
    assert pg([3, 1, 2, 1, 4], [2300, 600, 1, 900, 3000], 4) == [[0, 1], [2, 3, 4]]
    assert pg([1, 1, 1, 1, 1], [5, 5, 5, 5, 5], 2) == [[0, 1], [2, 3], [4]]
    assert pg([9, 1, 1], [8000, 10, 10], 4) == [[0], [1, 2]]                     # one recording fills a group
    # bytes: two recordings of 1000 frames are 704 000 bytes; with 2 heads twice that
    assert pg([1, 1, 1], [1000, 1000, 1000], 100, 704000) == [[0, 1], [2]]
    assert pg([1, 1, 1], [1000, 1000, 1000], 100, 704000, heads=2) == [[0], [1], [2]]
    assert pg([1, 1, 1], [1000, 1000, 1000], 100, 703999) == [[0], [1], [2]]
    # padding counts: a short recording next to a long one costs the long one's frames
    assert pg([1, 4, 1], [10, 4000, 10], 100, 88 * 4 * 4000 * 2) == [[0, 1], [2]]
    # an oversize recording is a group of its own, wherever it stands
    assert pg([1, 40, 1, 1], [10, 40000, 10, 10], 100, 1 << 20) == [[0], [1], [2, 3]]
    assert pg([40], [40000], 100, 1) == [[0]]
    # zero-sample recordings: one window, one frame
    assert pg([1] * 5, [1] * 5, 3) == [[0, 1, 2], [3, 4]]
    assert pg([1, 3, 1], [1, 2000, 1], 128 * 3) == [[0, 1, 2]]
    with pytest.raises(ValueError):
        pg([1, 2], [1], 4)
    with pytest.raises(ValueError):
        pg([1], [1], 0)


def test_random_cases(corpus):
    rng = np.random.default_rng(0)
    closed_by_windows = closed_by_bytes = singles_over = 0
    for case in range(200):
        n = int(rng.integers(1, 40))
        frames = [1 if rng.random() < 0.1 else int(rng.integers(2, 60000)) for _ in range(n)]
        windows = [1 + max(0, t - 938) // 876 for t in frames]
        heads = int(rng.integers(1, 3))
        gw = int(rng.integers(1, 200))
        gb = int(rng.choice([1 << 30, 1 << 26, 1 << 24, 88 * 4 * 30000]))
        groups = corpus.plan_groups(windows, frames, gw, gb, heads)
        _check(groups, windows, frames, gw, gb, heads)
        assert groups == corpus.plan_groups(np.array(windows), np.array(frames), gw, gb, heads)
        for g in groups[:-1]:
            if sum(windows[k] for k in g) >= gw:
                closed_by_windows += 1
            else:
                closed_by_bytes += 1
        singles_over += sum(len(g) == 1 and _bytes(g, frames, heads) > gb for g in groups)
    assert closed_by_windows > 100 and closed_by_bytes > 100 and singles_over > 10
