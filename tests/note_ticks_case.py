"""The cases of the tick-matcher tests and a numpy restatement of the kernel's algorithm (helper module of test_note_ticks_cpu.py /
test_gpu_note_ticks.py; not collected; numpy only).

`row_counts` is mt_note_match_ticks' algorithm for one pitch row as csrc/note_ticks.hip builds it: lo / hi of every reference note by
binary search, the cuts where hi(i - 1) < lo(i), and per component the greedy pass for tp_onset and, for tp_onset_offset, per reference
note the greedy step (the first free compatible estimate) and otherwise a depth-first search with an explicit stack whose visit stamps
are the number of augmentations so far.  It also reports what the walk met (components, greedy matches, augmentations, failed searches,
the deepest stack), by which the CPU test knows that the cases exercise it.

`tables()` is one pair of note lists (estimates, reference) of 3 x 88 rows: the special rows of SPECIAL at fixed places, random rows
elsewhere."""
import numpy as np

TOL = 500
B, P = 3, 88
SEED = 3


def off_ok(r_on, r_off, e_off):
    return 5 * abs(int(r_off) - int(e_off)) <= max(2500, int(r_off) - int(r_on))


def row_counts(e_on, e_off, r_on, r_off, end=None):
    """-> dict: n_ref, n_est, tp_onset, tp_onset_offset and the walk's statistics.  end: 320 L of mt_note_match_list's length rule."""
    e_on, e_off, r_on, r_off = (np.asarray(v, dtype=np.int64) for v in (e_on, e_off, r_on, r_off))
    if end is not None:
        nr = int(np.searchsorted(r_on, end, side="left"))
        r_on, r_off = r_on[:nr], np.minimum(r_off[:nr], end)
    nr, ne = len(r_on), len(e_on)
    out = dict(n_ref=nr, n_est=ne, tp_onset=0, tp_onset_offset=0, components=[], greedy=0, augmentations=0, failed=0, max_depth=0)
    if not nr or not ne:
        return out
    lo = np.searchsorted(e_on, r_on - TOL, side="left")
    hi = np.searchsorted(e_on, r_on + TOL, side="right") - 1
    assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all() and (hi >= lo - 1).all()
    match, stamp = np.full(ne, -2, np.int64), np.full(ne, -2, np.int64)          # -2: never initialised; reading it is an error
    stk_i, stk_j = np.full(nr, -2, np.int64), np.full(nr, -2, np.int64)
    starts = [i for i in range(nr) if i == 0 or hi[i - 1] < lo[i]]

    def augment(a, root, epoch):
        d, i, j, h = 0, root, lo[root], hi[root]
        stk_i[a] = root
        while True:
            if j > h:
                d -= 1
                if d < 0:
                    return False
                i, j = stk_i[a + d], stk_j[a + d]
                assert i >= a and j >= 0
                h = hi[i]
                continue
            jj = j
            j += 1
            assert stamp[jj] >= -1, "stamp read before it was initialised"
            if stamp[jj] == epoch or not off_ok(r_on[i], r_off[i], e_off[jj]):
                continue
            stamp[jj] = epoch
            m = match[jj]
            assert m >= -1, "match read before it was initialised"
            assert a + d <= root, "the stack left the component's slice"
            stk_j[a + d] = j
            if m < 0:
                for k in range(d + 1):
                    match[stk_j[a + k] - 1] = stk_i[a + k]
                out["max_depth"] = max(out["max_depth"], d)
                return True
            d += 1
            out["max_depth"] = max(out["max_depth"], d)
            i, j, h = m, lo[m], hi[m]
            assert a + d <= root, "the stack left the component's slice"
            stk_i[a + d] = m

    for a in starts:
        l, h = lo[a], hi[a]
        p, init_to, epoch, i = l, l, 0, a
        while True:
            match[init_to:h + 1] = stamp[init_to:h + 1] = -1
            init_to = max(init_to, h + 1)
            p = max(p, l)
            if p <= h:
                out["tp_onset"] += 1
                p += 1
            if l <= h:
                found = False
                for j in range(l, h + 1):
                    assert match[j] >= -1
                    if match[j] < 0 and off_ok(r_on[i], r_off[i], e_off[j]):
                        match[j], found = i, True
                        out["greedy"] += 1
                        break
                if not found:
                    found = augment(a, i, epoch)
                    epoch += found
                    out["augmentations" if found else "failed"] += 1
                out["tp_onset_offset"] += found
            i += 1
            if i >= nr or h < lo[i]:
                break
            l, h = lo[i], hi[i]
        out["components"].append((a, i))
    assert out["tp_onset_offset"] == int((match >= 0).sum())
    return out


def rows_of(notes):
    """{"on", "off", "ptr"} arrays -> [(on, off)] per row."""
    pt = np.asarray(notes["ptr"])
    return [(np.asarray(notes["on"])[pt[r]:pt[r + 1]], np.asarray(notes["off"])[pt[r]:pt[r + 1]]) for r in range(len(pt) - 1)]


def model_counts(est, ref, lengths=None, pitches=P):
    """row_counts over two note lists -> ((B, 4) int64 counts, the per-row dicts)."""
    per = []
    for r, ((eo, ef), (ro, rf)) in enumerate(zip(rows_of(est), rows_of(ref))):
        per.append(row_counts(eo, ef, ro, rf, None if lengths is None else 320 * max(0, int(lengths[r // pitches]))))
    counts = np.zeros((len(per) // pitches, 4), np.int64)
    for r, c in enumerate(per):
        counts[r // pitches] += [c["n_ref"], c["n_est"], c["tp_onset"], c["tp_onset_offset"]]
    return counts, per


def scipy_row(e_on, e_off, r_on, r_off):
    """(tp_onset, tp_onset_offset) of one row by scipy's maximum bipartite matching."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    eo, ef, ro, rf = (np.asarray(v, dtype=np.int64) for v in (e_on, e_off, r_on, r_off))
    if not len(ro) or not len(eo):
        return 0, 0
    near = np.abs(ro[:, None] - eo[None, :]) <= TOL
    both = near & (5 * np.abs(rf[:, None] - ef[None, :]) <= np.maximum(2500, rf - ro)[:, None])
    return tuple(int((maximum_bipartite_matching(csr_matrix(g.astype(np.int8)), perm_type="column") >= 0).sum()) for g in (near, both))


# ------------------------------------------------------------------------------------------------ rows
def _estimates_near(rng, on, off, keep=0.85, extra=0.15, jitter=450, off_jitter=900):
    """Estimates scattered around reference notes: most notes get one, some two, with onset and offset jitter, plus strays."""
    est = []
    for a, b in zip(on, off):
        k = 1 if rng.random() < keep else 0
        k += rng.random() < extra
        for _ in range(k):
            s = max(0, int(a + rng.integers(-jitter, jitter + 1)))
            est.append((s, max(s + 1, int(b + rng.integers(-off_jitter, off_jitter + 1)))))
    for _ in range(int(rng.integers(0, 2))):
        s = int(rng.integers(0, max(1, int(on.max()) if len(on) else 12000)))
        est.append((s, s + int(rng.integers(1, 3000))))
    est.sort()
    return np.array([s for s, _ in est], np.int64), np.array([e for _, e in est], np.int64)


def random_row(rng):
    n = int(rng.integers(1, 9)) if rng.random() < 0.75 else 0
    on = np.sort(rng.integers(0, 6000, size=n))                                # close together: several notes share a window
    off = on + rng.integers(50, 4000, size=n)
    if n and rng.random() < 0.3:
        k = int(rng.integers(0, n))
        on[k:k + 2] = on[k]                                                     # (an onset may repeat)
    e_on, e_off = _estimates_near(rng, on, off) if rng.random() < 0.85 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    return e_on, e_off, on, off


def dense_row(rng, n):
    """n reference notes 100 to 900 ticks apart: components of every size, some across the 64-note tile boundaries."""
    on = np.cumsum(rng.integers(100, 900, size=n)) if n else np.zeros(0, np.int64)
    off = on + rng.integers(50, 4000, size=n)
    return (*_estimates_near(rng, on, off), on, off)


def one_sided(rng, refs):
    on = np.sort(rng.integers(0, 50000, size=40))
    off = on + rng.integers(50, 4000, size=40)
    none = np.zeros(0, np.int64)
    return (none, none, on, off) if refs else (on, off, none, none)


def equal_onsets(rng):
    """Runs of equal onsets on both sides, the offsets deciding who matches whom."""
    on = np.repeat(np.arange(5) * 300 + 1000, 3)
    off = on + np.tile([400, 1500, 3900], 5)
    e_on = np.repeat(np.arange(4) * 300 + 1100, 4)
    e_off = e_on + rng.integers(100, 4200, size=e_on.size)
    return e_on, e_off, on, off


def straddle(rng):
    """60 lone notes, then a chain of 12 notes 400 ticks apart: one component over reference notes 60 .. 71, across the tile boundary at 64."""
    on = np.concatenate([np.arange(60) * 3000, 60 * 3000 + np.arange(12) * 400])
    off = on + 300
    e_on = on + 150
    e_off = e_on + 150 + rng.integers(-700, 701, size=on.size)
    return e_on, np.maximum(e_off, e_on + 1), on, off


def chained(rng, n=1100):
    """n reference notes 400 ticks apart, every estimate within reach of three of them: one component.  The notes are 300, 1800 or
    3300 ticks long and the estimates' offsets off by up to 800 ticks where 500 to 660 are allowed, so the offset test prunes edges and
    some of the searches augment."""
    on = np.arange(n) * 400 + 200
    off = on + 300 + 1500 * rng.integers(0, 3, size=n)
    e_on = np.sort(on + 20 + rng.integers(-100, 101, size=n))
    e_off = off + rng.integers(-800, 801, size=n)
    return e_on, np.maximum(e_off, e_on + 1), on, off


def deep_search(n=300):
    """Reference note i reaches estimates i and i + 1; estimate 0 fails note 0's offset test, so the greedy step gives note i estimate
    i + 1, and the last note, which reaches estimate n - 1 alone, searches down the whole chain (n - 1 notes deep) and fails."""
    on = np.arange(n) * 400 + 200
    off = on + 300
    e_on = np.arange(n) * 400 + 50
    e_off = e_on + 450
    e_off[0] += 3000
    return e_on, e_off, on, off


def augmenting(_rng=None):
    """The smallest row that needs an augmentation: note 0 takes estimate 0, which is all note 1 can have; note 0 moves to estimate 1."""
    return np.array([1000, 1010]), np.array([2000, 2450]), np.array([1000, 1020]), np.array([2050, 1900])


SPECIAL = {                    # row -> (name, builder)
    0: ("refs_0", lambda g: dense_row(g, 0)), 1: ("refs_1", lambda g: dense_row(g, 1)), 2: ("refs_63", lambda g: dense_row(g, 63)),
    3: ("refs_64", lambda g: dense_row(g, 64)), 90: ("refs_65", lambda g: dense_row(g, 65)), 91: ("refs_129", lambda g: dense_row(g, 129)),
    5: ("refs_only", lambda g: one_sided(g, True)), 93: ("ests_only", lambda g: one_sided(g, False)),
    7: ("equal_onsets", equal_onsets), 95: ("straddle", straddle), 180: ("chained", chained), 181: ("deep_search", lambda g: deep_search()),
    182: ("augmenting", augmenting), 263: ("refs_129_last", lambda g: dense_row(g, 129)),
}
RANDOM_ROWS = [r for r in range(B * P) if r not in SPECIAL]


def tables(seed=SEED):
    """-> (est, ref): {"on", "off" int32, "ptr" int64} of B * P rows."""
    rng = np.random.default_rng(seed)
    est, ref = ([], [], [0]), ([], [], [0])
    for r in range(B * P):
        e_on, e_off, r_on, r_off = SPECIAL[r][1](rng) if r in SPECIAL else random_row(rng)
        for (on, off, pt), a, b in ((est, e_on, e_off), (ref, r_on, r_off)):
            assert len(a) == len(b) and (np.diff(a) >= 0).all() and (np.asarray(a) >= 0).all() and (np.asarray(b) > np.asarray(a)).all()
            on += [int(v) for v in a]
            off += [int(v) for v in b]
            pt.append(len(on))
    pack = lambda t: {"on": np.array(t[0], np.int32), "off": np.array(t[1], np.int32), "ptr": np.array(t[2], np.int64)}
    return pack(est), pack(ref)
