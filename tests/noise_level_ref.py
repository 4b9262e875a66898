"""Restatement of noisediff_amd.noise_level for the tests: the level grid and the integer table with Python integers, the per-level statistics
and the curve with numpy float64, and sklearn's spatial median (_spatial_median / _modified_weiszfeld_step of sklearn 1.7.2) on all pairs or
on a given pair table.  Needs neither sklearn nor the reference tree.  The seeded inputs of the goldens and of the GPU tests live here too, so
that the capture script and the tests build the same arrays."""
import numpy as np

N_LEVELS, SCALE = 15872, 15871.0
EPS = float(np.finfo(np.float64).eps)
OFF_GRID, BAD_NOISY = -1, -2


# --------------------------------------------------------------------------- the table

def classify(clean, noisy, n_levels=N_LEVELS, scale=SCALE):
    """Per element the level (>= 0), OFF_GRID or BAD_NOISY, and q = rint(noisy * 2^30) + 2^32 (int64; meaningless where the level is < 0)."""
    c, v, s = np.asarray(clean, np.float32).ravel(), np.asarray(noisy, np.float32).ravel(), np.float32(scale)
    with np.errstate(all="ignore"):
        lf = np.rint(c * s)                                                      # fp32
        on = (lf >= 0) & (lf < np.float32(n_levels))
        on &= np.abs(c - lf / s) < np.float32(1e-6)
        good = np.abs(v) < np.float32(4.0)                                       # NaN and inf fail
        q = np.where(good, np.rint(np.where(good, v, 0).astype(np.float64) * 2.0 ** 30), 0).astype(np.int64) + (1 << 32)
    level = np.where(on, np.where(on, lf, 0).astype(np.int64), OFF_GRID)
    level = np.where(on & ~good, BAD_NOISY, level)
    return level, q


def table(clean, noisy, n_levels=N_LEVELS, scale=SCALE):
    """({level: [n, sum q, sum q^2]} as Python integers, [off grid, bad noisy])."""
    level, q = classify(clean, noisy, n_levels, scale)
    t = {}
    for l, qq in zip(level.tolist(), q.tolist()):
        if l >= 0:
            e = t.setdefault(l, [0, 0, 0])
            e[0] += 1
            e[1] += qq
            e[2] += qq * qq
    return t, [int((level == OFF_GRID).sum()), int((level == BAD_NOISY).sum())]


def merge(a, b):
    t = {l: list(e) for l, e in a.items()}
    for l, e in b.items():
        o = t.setdefault(l, [0, 0, 0])
        for k in range(3):
            o[k] += e[k]
    return t


def words(t, n_levels=N_LEVELS):
    """The table as the library lays it out: uint64 [n_levels][4] = count, sum q, low and high word of sum q^2."""
    w = np.zeros((n_levels, 4), np.uint64)
    for l, (n, s1, s2) in t.items():
        assert n < (1 << 31) and s1 < (1 << 64) and s2 < (1 << 128)
        w[l] = [n, s1, s2 & ((1 << 64) - 1), s2 >> 64]
    return w


def stats(t, n_levels=N_LEVELS):
    """(count, mean, std) from the integer table, the library's formulas: the integer part exact, one conversion, IEEE divisions."""
    count, mean, std = np.zeros(n_levels, np.int64), np.full(n_levels, np.nan), np.full(n_levels, np.nan)
    for l, (n, s1, s2) in t.items():
        count[l] = n
        mean[l] = float(s1 - (n << 32)) / float(n) * 2.0 ** -30
        if n >= 2:
            std[l] = np.sqrt(float(n * s2 - s1 * s1) / float(n) / float(n - 1)) * 2.0 ** -30
    return count, mean, std


def stats_float64(clean, noisy, n_levels=N_LEVELS, scale=SCALE):
    """(count, mean, std) of the EXACT noisy values per level in numpy float64 (two passes): what the quantised table is measured against."""
    level, _ = classify(clean, noisy, n_levels, scale)
    v = np.asarray(noisy, np.float32).ravel().astype(np.float64)
    count, mean, std = np.zeros(n_levels, np.int64), np.full(n_levels, np.nan), np.full(n_levels, np.nan)
    for l in np.unique(level[level >= 0]):
        g = v[level == l]
        count[l], mean[l] = g.size, g.mean()
        if g.size >= 2:
            std[l] = g.std(ddof=1)
    return count, mean, std


def curve(count, std, scale=SCALE, below_median=True):
    """(levels, x, y): the levels with count >= 1 ascending, cut at the lower median of these levels on request, NaN stds dropped."""
    levels = np.nonzero(np.asarray(count) >= 1)[0]
    if below_median:
        levels = levels[:(levels.size - 1) // 2 + 1]
    levels = levels[~np.isnan(np.asarray(std)[levels])]
    x = (levels.astype(np.float32) / np.float32(scale)).astype(np.float64)
    return levels, x, np.asarray(std, np.float64)[levels]


# --------------------------------------------------------------------------- the fit

def all_pairs(m):
    i, j = np.triu_indices(m, 1)                                                 # itertools.combinations(range(m), 2)'s order
    return np.stack([i, j], 1).astype(np.int32)


def sklearn_pairs(m, n=10000, seed=0):
    """The subsets TheilSenRegressor(random_state=seed) draws above 141 samples (sklearn 1.7.2, _theil_sen.py, fit)."""
    rs = np.random.RandomState(seed)
    return np.array([rs.choice(m, size=2, replace=False) for _ in range(n)], np.int32)


def pair_points(x, y, pairs):
    """[P, 2] = (intercept, slope) of every pair, float64."""
    x, y, p = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(pairs)
    with np.errstate(all="ignore"):
        slope = (y[p[:, 1]] - y[p[:, 0]]) / (x[p[:, 1]] - x[p[:, 0]])
        return np.stack([y[p[:, 0]] - slope * x[p[:, 0]], slope], 1)


def weiszfeld_step(X, x_old):
    diff = X - x_old
    diff_norm = np.sqrt(np.sum(diff ** 2, axis=1))
    mask = diff_norm >= EPS
    in_x = int(mask.sum() < X.shape[0])
    diff, diff_norm = diff[mask], diff_norm[mask][:, np.newaxis]
    q = np.sum(diff / diff_norm, axis=0)
    quotient_norm = float(np.sqrt(q[0] * q[0] + q[1] * q[1])) if q.shape == (2,) else 0.0
    if quotient_norm > EPS:
        new_direction = np.sum(X[mask, :] / diff_norm, axis=0) / np.sum(1 / diff_norm, axis=0)
    else:
        new_direction, quotient_norm = 1.0, 1.0
    return max(0.0, 1.0 - in_x / quotient_norm) * new_direction + min(1.0, in_x / quotient_norm) * x_old


def spatial_median(X, max_iter=300, tol=1e-3, moves=None):
    """(steps taken, median).  ``moves``: a list that receives every step's squared move (the stopping test compares it with tol^2)."""
    tol2 = tol * tol
    old = np.mean(X, axis=0)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            new = weiszfeld_step(X, old)
            move = np.sum((old - new) ** 2)
            if moves is not None:
                moves.append(float(move))
            if move < tol2:
                break
            old = new
    return it + 1, new


def theil_sen(x, y, pairs=None, max_iter=300, tol=1e-3, reverse=False, moves=None):
    """(slope, intercept, steps).  ``reverse``: the points in reversed order, to measure what the order of the sums is worth."""
    m = len(x)
    if m == 0:
        return 0.0, 0.0, 0
    if pairs is None:
        if m == 1:
            return float("nan"), float("nan"), 0
        pairs = all_pairs(m)
    X = pair_points(x, y, pairs)
    steps, med = spatial_median(X[::-1].copy() if reverse else X, max_iter, tol, moves)
    return float(med[1]), float(med[0]), steps


def order_gap(x, y, pairs=None, max_iter=300, tol=1e-3):
    """|forward - reversed| of (slope, intercept): the conditioning of the long sums on this input."""
    a, b = theil_sen(x, y, pairs, max_iter, tol), theil_sen(x, y, pairs, max_iter, tol, reverse=True)
    assert a[2] == b[2], (a, b)
    return abs(a[0] - b[0]), abs(a[1] - b[1])


def get_poisson_lambda(clean, noisy, n_levels=N_LEVELS, scale=SCALE, below_median=True, moves=None):
    """(lambda, sigma, steps, levels fitted) through the integer table, the curve and the all-pairs fit."""
    t, _ = table(clean, noisy, n_levels, scale)
    count, _, std = stats(t, n_levels)
    levels, x, y = curve(count, std, scale, below_median)
    slope, intercept, steps = theil_sen(x, y, moves=moves)
    return slope, intercept, steps, levels.size


# --------------------------------------------------------------------------- seeded inputs

def level_frame(seed, shape, n_pool, extra=(0, 15871), singleton=True, lam=2e-4, var0=1e-6, scale=SCALE):
    """(clean, noisy) fp32 of ``shape``: levels drawn from ``n_pool`` of 1 .. 2999, five elements on each of ``extra`` and, on request, one
    element alone on a low level; noise variance lam * clean + var0."""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    pool = np.sort(rs.choice(np.arange(1, 3000), n_pool, replace=False))
    lv = rs.choice(pool, n)
    pos = rs.permutation(n)
    k = 0
    for e in extra:
        lv[pos[k:k + 5]] = e
        k += 5
    if singleton:
        lv[pos[k]] = next(i for i in range(1, 3000) if i not in set(pool.tolist()))
    clean = (lv.astype(np.float32) / np.float32(scale)).reshape(shape)
    noisy = (clean + np.sqrt(lam * clean.astype(np.float64) + var0) * rs.standard_normal(shape)).astype(np.float32)
    return clean, noisy


def synthetic_curve(m, seed, lam=2e-4, var0=1e-6, scale=SCALE):
    """(x, y) float64: m levels of 0 .. 15871 ascending as fp32 clean values, y = sqrt(lam x + var0) with 5 % scatter and a few outliers."""
    rs = np.random.RandomState(seed)
    lv = np.sort(rs.choice(int(scale) + 1, m, replace=False))
    x = (lv.astype(np.float32) / np.float32(scale)).astype(np.float64)
    y = np.sqrt(lam * x + var0) * (1.0 + 0.05 * rs.standard_normal(m))
    y[rs.choice(m, m // 10, replace=False)] *= 3.0
    return x, y


FIT_CASES = {                    # name: (m, seed, pairs, max_iter, tol); pairs: None = all, "sk" = sklearn_pairs(m)
    "m2": (2, 11, None, 300, 1e-3), "m3": (3, 12, None, 300, 1e-3), "m8": (8, 13, None, 300, 1e-3), "m141": (141, 14, None, 300, 1e-3),
    "m300.pairs": (300, 15, "sk", 300, 1e-3), "m700": (700, 16, None, 300, 1e-3), "m100.exhausted": (100, 17, None, 3, 0.0),
    "m141.tight": (141, 14, None, 300, 1e-7),
}
SKLEARN_CASES = {"m2": (2, 11, None), "m8": (8, 13, None), "m100": (100, 17, None), "m141": (141, 14, None), "m300": (300, 15, "sk"),
                 "m1000": (1000, 18, "sk")}


def fit_case(name):
    m, seed, pairs, max_iter, tol = FIT_CASES[name]
    x, y = synthetic_curve(m, seed)
    return x, y, (sklearn_pairs(m) if pairs == "sk" else None), max_iter, tol
