"""TEST INFRASTRUCTURE: the moment planes and THE NOISE RULE of the ray-traced primary (header of
4d-cbct-mc_amd/csrc/primary_project.hip) restated in numpy float64, on top of tests/primary_ref.py (imported, not changed).

  MomentPrimary(ctx)           primary_ref.Primary whose spectrum weights are W_q = P_b g_j f(E_q): .weight = f (default E -> E: the
                               plane M_1); moment(k) sets f = E^k.  Traversals are kept, so the planes of several f cost one traversal.
  .moment_planes(p, ...)       {(k, Qn, "f64" | "f32"): M_k} for the moments asked for
  .weighted_plane(p, f, ...)   the plane of an arbitrary weight, float64 (the fourth moment; the truncated squares of the tally)
  draws(seed, n, ny, nx, ...)  u, z of draw k at every pixel: Philox4x32-10, key = seed, counter (x, y, first_projection + p, k)
  compound_poisson(...)        the rule on given planes: value (float64, not yet rounded), count n, `ambiguous` pixels
  gaussian(...)                max(0, mean + sqrt(max(variance, 0)) z2)
  rule_moments(...)            mean, variance, fourth central moment and zero fraction the rule has on constant planes
  w2_statement(...)            "M_2 is what the engine tallies" as an interval test per 8 x 8 block and a global pull"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
from scipy.stats import norm, poisson

import primary_ref as pr

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import fast_rng  # noqa: E402

AMBIGUOUS = 1e-9       # u within this of a step of F, or the argument of floor within this of an integer
LAMBDA_SWITCH = 64.0
N_MAX = 1024


class MomentPrimary(pr.Primary):
    def __init__(self, ctx):
        super().__init__(ctx)
        self.weight = None                       # None: the plane M_1 exactly as primary_ref forms it
        self._kept = {}
        self.pixel_area = 1.0 / (float(self.detector[0]["inv_pixel_size_X"]) * float(self.detector[0]["inv_pixel_size_Z"]))

    def spectrum(self, qn):
        E, W, K = super().spectrum(qn)
        if self.weight is None:
            return E, W, K
        gx, gw = np.polynomial.legendre.leggauss(qn)
        bins = np.nonzero(self.prob > 0.0)[0]
        base = (self.prob[bins][:, None] * 0.5 * gw[None, :]).reshape(-1)          # P_b g_j
        return E, base * self.weight(E), K

    def thickness_both(self, src, d):
        key = (np.asarray(src).tobytes(), np.asarray(d).shape, hash(np.ascontiguousarray(d).tobytes()))
        if key not in self._kept:
            self._kept[key] = super().thickness_both(src, d)
        return self._kept[key]

    def moment_planes(self, p, subsamples=(1, 1), energy_points=(2,), moments=(0, 1, 2), flip=True):
        out = {}
        try:
            for k in moments:
                self.weight = None if k == 1 else (lambda E, k=k: E ** k)
                for (qn, tag), plane in self.planes(p, subsamples, tuple(energy_points), flip=flip).items():
                    out[(k, qn, tag)] = plane
        finally:
            self.weight = None
        return out

    def weighted_plane(self, p, weight, subsamples=(1, 1), energy_points=2, flip=True):
        try:
            self.weight = weight
            return self.planes(p, subsamples, (energy_points,), flip=flip)[(energy_points, "f64")]
        finally:
            self.weight = None


# ---- the draws -----------------------------------------------------------------------------------------------------------------
def draws(seed: int, n: int, ny: int, nx: int, k: int, first_projection: int = 0):
    """(u, z) [n, ny, nx] of draw k: u = ((w0 >> 8) + 1) 2^-24, z = sqrt(-2 ln u) cos(2 pi (w1 >> 8) 2^-24)."""
    p, y, x = np.meshgrid(np.arange(n, dtype=np.uint64) + np.uint64(first_projection), np.arange(ny, dtype=np.uint64), np.arange(nx, dtype=np.uint64),
                          indexing="ij")
    w = fast_rng.philox4x32([x, y, p, np.full_like(x, k)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], rounds=10)
    u = ((w[0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u, np.sqrt(-2.0 * np.log(u)) * np.cos(2.0 * np.pi * u2)


def _planes(*a):
    a = [np.asarray(v, dtype=np.float32).astype(np.float64) for v in a]
    a = [v.reshape((-1,) + v.shape[-2:]) for v in a]
    return a


def compound_poisson(m0, m1, m2, histories, pixel_area, seed, first_projection=0):
    """THE NOISE RULE on float32 planes [n, ny, nx]: (value float64 before the one rounding to float32, count n, ambiguous)."""
    M0, M1, M2 = _planes(m0, m1, m2)
    shape = M0.shape
    na = float(histories) * float(pixel_area)
    lit = M0 > 0.0
    safe = np.where(lit, M0, 1.0)
    lam, mu = na * safe, M1 / safe
    s2 = np.maximum(M2 / safe - mu * mu, 0.0)
    u, z0 = draws(seed, *shape, 0, first_projection)
    _, z1 = draws(seed, *shape, 1, first_projection)
    count = np.zeros(shape)
    ambiguous = np.zeros(shape, dtype=bool)
    # lambda < 64: inversion by sequential search
    small = lit & (lam < LAMBDA_SWITCH)
    idx = np.nonzero(small)
    l, uu = lam[idx], u[idx]
    p = np.exp(-l)
    F = p.copy()
    n = np.zeros(l.shape)
    amb = np.abs(uu - F) < AMBIGUOUS
    active = np.nonzero(uu > F)[0]
    for step in range(1, N_MAX + 1):
        if active.size == 0:
            break
        n[active] += 1.0
        p[active] *= l[active] / n[active]
        F[active] += p[active]
        amb[active] |= np.abs(uu[active] - F[active]) < AMBIGUOUS
        active = active[uu[active] > F[active]]
    count[idx], ambiguous[idx] = n, amb
    # lambda >= 64: the normal with its first skewness correction
    large = lit & ~small
    arg = lam + np.sqrt(lam) * z0 + (z0 * z0 - 1.0) / 6.0 + 0.5
    count = np.where(large, np.maximum(0.0, np.floor(arg)), count)
    ambiguous |= large & (np.abs(arg - np.rint(arg)) < AMBIGUOUS)
    value = np.where(lit & (count > 0), np.maximum(0.0, count * mu + np.sqrt(count * s2) * z1) / na, 0.0)
    return value, np.where(lit, count, 0.0), ambiguous & lit


def value_at_count(m0, m1, m2, histories, pixel_area, seed, count, first_projection=0):
    """The value of the rule at a given count n (the comparison "at equal count"), and the size of its terms for the tolerance."""
    M0, M1, M2 = _planes(m0, m1, m2)
    na = float(histories) * float(pixel_area)
    lit = M0 > 0.0
    safe = np.where(lit, M0, 1.0)
    mu = M1 / safe
    s2 = np.maximum(M2 / safe - mu * mu, 0.0)
    _, z1 = draws(seed, *M0.shape, 1, first_projection)
    count = np.asarray(count, dtype=np.float64).reshape(M0.shape)
    ok = lit & (count > 0)
    terms = np.where(ok, (count * np.abs(mu) + np.sqrt(count * s2) * np.abs(z1)) / na, 0.0)
    return np.where(ok, np.maximum(0.0, count * mu + np.sqrt(count * s2) * z1) / na, 0.0), terms


def gaussian(mean, variance, seed, first_projection=0):
    """(value float64 before rounding, size of its terms)."""
    m, v = _planes(mean, variance)
    _, z2 = draws(seed, *m.shape, 2, first_projection)
    sd = np.sqrt(np.maximum(v, 0.0))
    return np.maximum(0.0, m + sd * z2), np.abs(m) + sd * np.abs(z2)


# ---- what the rule's moments are -------------------------------------------------------------------------------------------------
def rule_moments(m0, m1, m2, histories, pixel_area):
    """For constant moments: (mean = M_1, variance = M_2 / (N a), fourth central moment, probability of an exact zero).
    S = N a x value is a compound Poisson sum of Gaussian jumps N(mu, s2): cumulants kappa_r = lambda E[Y^r], so kappa_2 = lambda
    (mu^2 + s2), kappa_4 = lambda (mu^4 + 6 mu^2 s2 + 3 s2^2) and mu_4 = kappa_4 + 3 kappa_2^2.  Zero: n = 0, or the clamp at n >= 1."""
    na = float(histories) * float(pixel_area)
    lam, mu = na * m0, m1 / m0
    s2 = max(m2 / m0 - mu * mu, 0.0)
    k2 = lam * (mu * mu + s2)
    k4 = lam * (mu ** 4 + 6.0 * mu * mu * s2 + 3.0 * s2 * s2)
    n = np.arange(1, int(lam + 40.0 * np.sqrt(lam) + 60.0))
    clamp = float(np.sum(poisson.pmf(n, lam) * norm.cdf(-np.sqrt(n) * mu / np.sqrt(s2)))) if s2 > 0 else 0.0
    return m1, k2 / na ** 2, (k4 + 3.0 * k2 * k2) / na ** 4, float(np.exp(-lam)) + clamp


def sampler_statement(values, m0, m1, m2, histories, pixel_area, label):
    """The statistical statement of the issue on one constant-plane sample: mean, variance and (lambda < 64) the fraction of zeros
    within 5 standard errors of the rule's values; the standard error of the variance from the rule's fourth central moment."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    n = v.size
    mean, var, mu4, p0 = rule_moments(m0, m1, m2, histories, pixel_area)
    lam = histories * pixel_area * m0
    se_mean = np.sqrt(var / n)
    se_var = np.sqrt((mu4 - var * var * (n - 3.0) / (n - 1.0)) / n)
    got_mean, got_var, got_p0 = float(v.mean()), float(v.var(ddof=1)), float(np.mean(v == 0.0))
    se_p0 = np.sqrt(p0 * (1.0 - p0) / n)
    print(f"{label}: lambda {lam:g}: mean {got_mean:.6g} (rule {mean:.6g}, {abs(got_mean - mean) / se_mean:.2f} se), variance {got_var:.6g} "
          f"(rule {var:.6g}, {abs(got_var - var) / se_var:.2f} se), zeros {got_p0:.6g} (rule {p0:.6g}, se {se_p0:.3g})")
    assert abs(got_mean - mean) <= 5.0 * se_mean, label
    assert abs(got_var - var) <= 5.0 * se_var, label
    if lam < LAMBDA_SWITCH:
        assert abs(got_p0 - p0) <= 5.0 * se_p0, label
    return got_mean, got_var, got_p0


# constant planes of the statistical cases: a pixel of 0.01 cm^2, photons of 60 keV +- 18 keV, lambda set through the histories
STAT_LAMBDAS = (0.5, 8.0, 63.0, 64.0, 1000.0)
STAT_SHAPE = (256, 256)
STAT_AREA = 0.01
STAT_M0 = 2.5e-4
STAT_MU, STAT_SD = 6.0e4, 1.8e4


def stat_case(lam):
    """(m0, m1, m2 as float32 values, histories) of the constant planes with N a M_0 = lam."""
    m0 = np.float32(STAT_M0)
    m1 = np.float32(STAT_M0 * STAT_MU)
    m2 = np.float32(STAT_M0 * (STAT_MU ** 2 + STAT_SD ** 2))
    return float(m0), float(m1), float(m2), lam / (STAT_AREA * float(m0))


# ---- M_2 is what the engine tallies ----------------------------------------------------------------------------------------------
def w2_expectations(P, p, n, subsamples, fine=(8, 8)):
    """Tally-unit planes (not flipped) of the restatement for N = n histories: upper = N a 1e4 M_2, lower (the tally squares w >> 10,
    w = 100 E: at least (100 E - 1023)^2), variance = N a 1e8 M_4, and upper at the fine sub-sampling for the edge mask."""
    na = n * P.pixel_area
    upper = P.weighted_plane(p, lambda E: (100.0 * E) ** 2, subsamples, flip=False) * na
    lower = P.weighted_plane(p, lambda E: np.maximum(100.0 * E - 1023.0, 0.0) ** 2, subsamples, flip=False) * na
    var = P.weighted_plane(p, lambda E: (100.0 * E) ** 4, subsamples, flip=False) * na
    fine_upper = P.weighted_plane(p, lambda E: (100.0 * E) ** 2, fine, flip=False) * na
    return upper, lower, var, fine_upper


def w2_blocks(upper, lower, var, fine_upper):
    """Block sums and the masks: lit, edge (the rule of primary_ref.expectation_statement), used."""
    ub, lb, vb, fb = (pr.block_sums(a) for a in (upper, lower, var, fine_upper))
    lit = (vb > 0) & (ub > 0)
    edge = lit & (np.abs(fb - ub) > 0.2 * np.sqrt(np.where(vb > 0, vb, 1.0)))
    return ub, lb, vb, lit, edge, lit & ~edge


def w2_statement(mc, tested, upper, lower, var, fine_upper, label):
    """mc = w2[0] 2^20 of the engine; tested = N a 1e4 M_2 of the kernel; the rest from the restatement.  A block passes between
    lower - 4 sd and upper + 4 sd, where the kernel's plane stands for `upper` and lower is shifted by the same difference."""
    ub, lb, vb, lit, edge, used = w2_blocks(upper, lower, var, fine_upper)
    tb, mb = pr.block_sums(tested), pr.block_sums(mc)
    hi, lo = tb, tb - (ub - lb)
    sd = np.sqrt(np.where(vb > 0, vb, 1.0))
    over, under = (mb - hi) / sd, (lo - mb) / sd
    worst = float(np.max(np.maximum(over, under)[used]))
    total_sd = np.sqrt(var.sum())
    pull = max(0.0, float(mc.sum() - tested.sum()), float((tested.sum() - (upper.sum() - lower.sum())) - mc.sum())) / total_sd
    print(f"{label}: blocks lit {int(lit.sum())}, left out {int(edge.sum())}, worst excess over [lower - 4 sd, upper + 4 sd] in sd "
          f"{worst - 4.0:.2f} (<= 0 passes), relative width of the interval {float((upper.sum() - lower.sum()) / upper.sum()):.2e}, "
          f"mc / upper {float(mc.sum() / tested.sum()):.6f}, global pull {pull:.2f}")
    assert edge.sum() <= 0.2 * lit.sum(), label
    assert worst <= 4.0, label
    assert pull <= 5.0, label
    return worst, pull


# ---- the inputs of the sampler comparison (GPU test c; held to the ambiguity cap on the CPU) -------------------------------------
SAMPLER_SHAPES = ((5, 7), (16, 16), (33, 17))          # [ny, nx] of the 7 x 5, 16 x 16 and 17 x 33 detectors
SAMPLER_HISTORIES, SAMPLER_AREA = 1048576.0, 0.0078125   # N a = 8192 exactly, so that lambda = 64 is met exactly
SAMPLER_LAMBDAS = (0.0, 1e-3, 1.0, 63.9, 64.0, 1e4)
SAMPLER_PLANES = 3


def sampler_inputs(shape):
    """Moment planes [3 planes, ny, nx] (float32) whose lambda takes every value of SAMPLER_LAMBDAS (0: a pixel with M_0 = 0) in
    turn, with photon energies of 30 .. 90 keV and spreads of 0 .. 30 keV; every seventh pixel has M_2 = M_0 mu^2 (s2 = 0 up to rounding)."""
    ny, nx = shape
    rng = np.random.default_rng(ny * 1000 + nx)
    n = SAMPLER_PLANES * ny * nx
    lam = np.array(SAMPLER_LAMBDAS)[(np.arange(n) + rng.integers(0, 6)) % 6]
    mu = rng.uniform(3.0e4, 9.0e4, n)
    sd = np.where(np.arange(n) % 7 == 0, 0.0, rng.uniform(0.0, 3.0e4, n))
    m0 = lam / (SAMPLER_HISTORIES * SAMPLER_AREA)
    planes = [a.astype(np.float32).reshape(SAMPLER_PLANES, ny, nx) for a in (m0, m0 * mu, m0 * (mu * mu + sd * sd))]
    return planes


def float32_tolerance(value, terms):
    """Rounding a float64 value once to float32 (half an ulp: 2^-24 relative, or the smallest subnormal), plus 1e-12 of the terms for
    the last bits of exp, log, cos and sqrt on either side."""
    return 2.0 ** -24 * np.abs(value) + 1e-12 * terms + 2.0 ** -149
