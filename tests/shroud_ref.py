"""The float64 restatement of the projection-derived breathing signal (the rule in the header of
csrc/shroud.hip), and the fixtures of its tests.

Stage A: t(u) = fl32(P[n][min(v + 1, nv - 1)][u] - P[n][max(v - 1, 0)][u]) (one float32 subtraction, the neighbour rows clamped to the
image), D[n][r] = 0.5 * sum over the ROI columns of double(t), A = fl32(D - (1 / w) * sum_{k = -h .. h} D[clamp(n + k)][r]) with k
ascending (w = 0: A = fl32(D)).  Stage B: c_i(s) = mean over the valid r of (A[i][r + s] - A[i - 1][r])^2 in float64 from the float32
A.  Stage C: argmin (lowest s on a tie), parabolic refinement where the minimum is interior and den > 0, cumulative sum from x_0 = 0."""
import numpy as np


def row_sums(projections, rows=None, columns=None) -> np.ndarray:
    """D [n, m] float64."""
    p = np.asarray(projections, dtype=np.float32)
    n, nv, nu = p.shape
    v_first, v_count = (0, nv) if rows is None else rows
    u_first, u_count = (0, nu) if columns is None else columns
    v = np.arange(v_first, v_first + v_count)
    cols = slice(u_first, u_first + u_count)
    t = p[:, np.minimum(v + 1, nv - 1), cols] - p[:, np.maximum(v - 1, 0), cols]
    assert t.dtype == np.float32
    return 0.5 * t.astype(np.float64).sum(axis=2)


def unsharp_mask(D, w: int) -> np.ndarray:
    """A [n, m] float32 from D."""
    D = np.asarray(D, dtype=np.float64)
    if w == 0:
        return D.astype(np.float32)
    assert w % 2 == 1 and w > 0
    n, h = D.shape[0], (w - 1) // 2
    s = np.zeros_like(D)
    for k in range(-h, h + 1):
        s = s + D[np.clip(np.arange(n) + k, 0, n - 1)]
    return (D - (1.0 / w) * s).astype(np.float32)


def shroud(projections, unsharp: int = 17, rows=None, columns=None) -> np.ndarray:
    return unsharp_mask(row_sums(projections, rows, columns), unsharp)


def costs(A, max_shift: int) -> np.ndarray:
    """[n - 1, 2 S + 1] float64."""
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    n, m = A.shape
    S = int(max_shift)
    assert 0 <= 2 * S < m
    c = np.zeros((max(n - 1, 0), 2 * S + 1))
    for j, s in enumerate(range(-S, S + 1)):
        lo, hi = max(0, -s), min(m, m - s)
        d = A[1:, lo + s:hi + s] - A[:-1, lo:hi]
        c[:, j] = (d * d).mean(axis=1)
    return c


def shifts(c):
    """-> (k* [pairs] int, shift [pairs] float64, den [pairs] float64 (nan where k* is on the border))."""
    c = np.asarray(c, dtype=np.float64)
    pairs, width = c.shape
    S = (width - 1) // 2
    k = np.argmin(c, axis=1) if pairs else np.zeros(0, dtype=int)  # the first of equal minima: the lowest s
    shift, den = (k - S).astype(np.float64), np.full(pairs, np.nan)
    for i in range(pairs):
        if 0 < k[i] < width - 1:
            den[i] = c[i, k[i] - 1] - 2.0 * c[i, k[i]] + c[i, k[i] + 1]
            if den[i] > 0:
                shift[i] = (k[i] - S) + 0.5 * (c[i, k[i] - 1] - c[i, k[i] + 1]) / den[i]
    return k - S, shift, den


def signal_from_costs(c) -> np.ndarray:
    """x [pairs + 1]: x_0 = 0, x_i = x_{i - 1} + shift_i, added one by one as the host does."""
    _, shift, _ = shifts(c)
    x = np.zeros(shift.size + 1)
    for i, s in enumerate(shift):
        x[i + 1] = x[i] + s
    return x


def signal(projections, unsharp: int = 17, max_shift: int = 16, rows=None, columns=None) -> np.ndarray:
    """The cumulative shifts, not detrended."""
    return signal_from_costs(costs(shroud(projections, unsharp, rows, columns), max_shift))


def detrend_linear(x) -> np.ndarray:
    y = np.asarray(x, dtype=np.float64)
    t = np.arange(y.size, dtype=np.float64)
    return y - np.polyval(np.polyfit(t, y, 1), t) if y.size > 1 else y - y


def local_maxima(x):
    x = np.asarray(x)
    return [i for i in range(1, x.size - 1) if x[i] > x[i - 1] and x[i] >= x[i + 1]]


# ---------------------------------------------------------------------------------------------------------------- fixtures
BREATHING_N, BREATHING_NV, BREATHING_NU = 120, 48, 40
BREATHING_TRUTH_MAXIMA = [8, 38, 67, 98]


def breathing_truth() -> np.ndarray:
    return 3.0 * np.sin(2 * np.pi * np.arange(BREATHING_N) / 30)


def breathing() -> np.ndarray:
    """P [120, 48, 40] float32: a static profile that drifts across the detector plus a logistic edge that follows truth_i."""
    i = np.arange(BREATHING_N, dtype=np.float64)[:, None, None]
    v = np.arange(BREATHING_NV, dtype=np.float64)[None, :, None]
    u = np.arange(BREATHING_NU, dtype=np.float64)[None, None, :]
    truth = breathing_truth()[:, None, None]
    static = 2 * np.exp(-(u - 20 - 6 * np.cos(2 * np.pi * i / 120)) ** 2 / 120) * (1 + 0.2 * np.sin(v / 5))
    edge = 1.5 / (1 + np.exp(-(v - 24 - truth - 0.01 * (u - 20) ** 2) / 1.2))
    return (static + edge).astype(np.float32)


def displaced_staircase(m: int = 34, shift: int = 3):
    """Two columns (before, after) of m = 34 integer-valued rows with after[r + 3] = before[r]: c(3) = 0 exactly, and the unit steps are
    placed so that c(2) = Q2 / 32 and c(4) = Q4 / 30 are the same rational (Q2 = 16, Q4 = 15): the refined shift is exactly 3 with
    den = c(2) + c(4) > 0."""
    assert m == 34 and shift == 3
    steps = np.zeros(m - 1)          # steps[j] = after[j + 1] - after[j]
    steps[2] = 1
    steps[3:33:2] = 1                # 15 unit steps among j = 3 .. 32
    after = np.concatenate([[0.0], np.cumsum(steps)])
    before = np.concatenate([after[3:], np.full(3, after[-1])])
    return before.astype(np.float32), after.astype(np.float32)
