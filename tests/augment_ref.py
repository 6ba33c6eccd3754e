"""Float64 numpy reference of the training augmentation (csrc/augment.hip, rawdata.Augment): the interpolation table, the
fixed-point resampling rule with the kernel's integer arithmetic, the mean square, the hash and Box-Muller noise, and the
column rule that moves the labels with the audio.  Written from the rule, not from the package's code."""
import numpy as np

TAPS, PHASES, BETA = 32, 256, 10.0
ONE = 1 << 32
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def table(beta=BETA):
    """(PHASES + 1, TAPS) float64: sinc(t) * kaiser_beta(t / 16), t = j - 15 - ph / P; unit row sums; rows 0 and P impulses."""
    tab = np.zeros((PHASES + 1, TAPS))
    for ph in range(PHASES + 1):
        t = np.arange(TAPS) - 15.0 - ph / PHASES
        w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / 16.0) ** 2))) / np.i0(beta)
        row = np.sinc(t) * w
        tab[ph] = row / row.sum()
    tab[0] = np.eye(TAPS)[15]
    tab[PHASES] = np.eye(TAPS)[16]
    return tab


def table_f32(beta=BETA):
    """The table as the device holds it (float32 values), in float64."""
    return table(beta).astype(np.float32).astype(np.float64)


def positions(n, rate_q32):
    """(k, ph, mu) of outputs 0..n-1: pos = i * rate_q32 in 64-bit, k = pos >> 32, ph = frac >> 24, mu = (frac & 0xffffff) * 2^-24."""
    pos = np.arange(n, dtype=np.uint64) * np.uint64(rate_q32)
    frac = pos & np.uint64(0xFFFFFFFF)
    k = (pos >> np.uint64(32)).astype(np.int64)
    ph = (frac >> np.uint64(24)).astype(np.int64)
    mu = (frac & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return k, ph, mu


def resample(x_at, n, rate_q32, tab):
    """y_i = sum_j c_j * x[k - 15 + j], c_j = tab[ph][j] + mu * (tab[ph + 1][j] - tab[ph][j]).  x_at(idx) returns the float64
    samples at window-relative integer positions idx (any shape), zero where the window's recording has none."""
    k, ph, mu = positions(n, rate_q32)
    c = tab[ph] + mu[:, None] * (tab[ph + 1] - tab[ph])
    idx = k[:, None] - 15 + np.arange(TAPS)[None, :]
    return (c * x_at(idx)).sum(axis=1)


def window_reader(store, win_off, before, after):
    """x_at for a window of a store: store[win_off + idx] inside [-before, after), else 0."""
    store = np.asarray(store, dtype=np.float64)

    def x_at(idx):
        ok = (idx >= -before) & (idx < after)
        return np.where(ok, store[np.clip(win_off + idx, 0, len(store) - 1)], 0.0)
    return x_at


def mean_square(y):
    return float(np.sum(np.asarray(y, dtype=np.float64) ** 2) / len(y))


def gauss(seed, b, n):
    """g(seed, b, i) for i < n in float64: the 64-bit mixer on i + ((seed << 8) ^ b) * GOLD + GOLD, u1 = ((h >> 40) + 1) * 2^-24,
    u2 = ((h >> 16) & 0xFFFFFF) * 2^-24, g = sqrt(-2 ln u1) * cos(2 pi u2)."""
    base = ((((seed << 8) ^ b) * GOLD) + GOLD) & M64
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(base)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u1 = ((z >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def cols_aug(t0, t1, fs, rate_q32):
    """cols' = round((t0 + r * (times - t0)) * fs), times = linspace(t0, t1, int((t1 - t0) * fs)), r = rate_q32 / 2^32."""
    times = np.linspace(t0, t1, int((t1 - t0) * fs))
    r = rate_q32 / float(ONE)
    return np.round((t0 + r * (np.asarray(times, dtype=np.float64) - t0)) * fs).astype(np.int64)


def rate_of_cents(cents):
    return int(np.rint(2.0 ** (cents / 1200.0) * ONE))
