"""TEST INFRASTRUCTURE: plain float64 restatements of the scattering samplers, numpy only.  Inputs: the host tables a context hands out
(`tables`, reference layouts: Rayleigh [point + material * 128], Compton [material + shell * 25], material = material number - 1)
and the per-history streams of oracle/fast_rng.py.

  rotate                 the textbook rotation of a direction by a polar and an azimuthal angle (MC-GPU_kernel_v1.3.cu:1103-1148)
  rayleigh_replay        GRAa's rejection loop (:1181-1246) fed the deviates the device draws, with the margin of every decision
  compton_angular_law    probability of each cos(theta) bin under GCOa's law (:1316-1372): envelope(tau) T(tau) S(E, tau)
  compton_first_tau      tau of a Compton event's first trial (:1318-1327) from its first two deviates
  azimuth_about          the azimuth of a rotated direction about the original one, in rotate's convention

tests/test_scatter_law.py pins these to the CPU oracle (and through tests/test_oracle_golden.py to the reference build) before any
GPU is involved; tests/test_scatter_gpu.py holds the HIP samplers to them."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT / "oracle") not in sys.path:
    sys.path.insert(0, str(ROOT / "oracle"))
import fast_rng  # noqa: E402

NPRAY, MAXMAT = 128, 25
MC2 = 510998.918            # electron rest energy [eV] as the reference writes it
INV_MC2 = 1.956951306108245e-6
WAVE = 8.065535669099010e-5  # E [eV] -> momentum transfer scale of GRAa
TABLE_NAMES = {"xco": "<f4", "pco": "<f4", "aco": "<f4", "bco": "<f4", "pmax": "<f4", "itlco": "u1", "ituco": "u1",
               "fco": "<f4", "uico": "<f4", "fj0": "<f4", "noscco": "<i4"}


def tables(ctx) -> dict:
    """The host tables of a context (engine.Context.host_table) plus the energy grid."""
    t = {k: ctx.host_table(k, dt) for k, dt in TABLE_NAMES.items()}
    t["e0"], t["ide"] = np.float32(ctx.getf("e0")), np.float32(ctx.getf("ide"))
    return t


def energy_index(t: dict, energy) -> int:
    """Bin of the energy grid (float32 arithmetic, as every build of the kernels computes it; callers stay off bin borders)."""
    return int(np.floor((np.float32(energy) - t["e0"]) * t["ide"]))


# ----------------------------------------------------------------------------------------------------------------------------------
# rotation
# ----------------------------------------------------------------------------------------------------------------------------------
def _frame(d):
    """Unit vector along d and the two transverse axes the reference's rotation measures the azimuth from."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    u, v, w = d[:, 0], d[:, 1], d[:, 2]
    dxy = u * u + v * v
    tilted = dxy > 1.0e-28
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 1.0 / np.sqrt(dxy)
        e1 = np.stack([u * w * s, v * w * s, -dxy * s], axis=1)
        e2 = np.stack([-v * s, u * s, np.zeros_like(u)], axis=1)
    sign = np.where(w > 0, 1.0, -1.0)
    e1 = np.where(tilted[:, None], e1, np.stack([sign, np.zeros_like(u), np.zeros_like(u)], axis=1))
    e2 = np.where(tilted[:, None], e2, np.stack([np.zeros_like(u), np.ones_like(u), np.zeros_like(u)], axis=1))
    return d, e1, e2


def rotate(d, costh, phi, sinth=None):
    """d (any length > 0) turned by the polar angle theta and the azimuth phi: d cos + sin (e1 cos(phi) + e2 sin(phi)).
    `sinth`: sin(theta) where the caller knows it better than sqrt(1 - cos^2) does (angles near 0 and pi)."""
    d, e1, e2 = _frame(d)
    costh = np.asarray(costh, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    st = np.sqrt(np.maximum(1.0 - costh * costh, 0.0)) if sinth is None else np.asarray(sinth, dtype=np.float64)
    return d * costh[:, None] + st[:, None] * (e1 * np.cos(phi)[:, None] + e2 * np.sin(phi)[:, None])


def azimuth_about(d_in, d_out):
    """phi in [0, 2 pi) with d_out = rotate(d_in, ., phi); meaningless where d_out is (anti)parallel to d_in."""
    _, e1, e2 = _frame(d_in)
    o = np.asarray(d_out, dtype=np.float64).reshape(-1, 3)
    return np.mod(np.arctan2(np.sum(o * e2, axis=1), np.sum(o * e1, axis=1)), 2.0 * np.pi)


# ----------------------------------------------------------------------------------------------------------------------------------
# deviates
# ----------------------------------------------------------------------------------------------------------------------------------
class MwcDeviates:
    """The per-history streams of the FAST kernels (oracle/fast_rng.py), advanced only for the items that draw.
    mapping "f32": rng_f, the float32 nearest to (u >> 8) 2^-24 + 2^-26;  "f64": rng_d, (u + 1/2) 2^-32."""

    def __init__(self, ids, seed: int, stream_key: int, mapping: str):
        self.x, self.c = fast_rng.seed_streams(np.asarray(ids, dtype=np.uint64), seed, stream_key)
        self.x, self.c = self.x.copy(), self.c.copy()
        self.mapping = mapping
        self.drawn = np.zeros(self.x.size, dtype=np.int64)

    def u32(self, idx):
        self.x[idx], self.c[idx] = fast_rng.mwc_step(self.x[idx], self.c[idx])
        self.drawn[idx] += 1
        return self.x[idx]

    def value(self, u):
        if self.mapping == "f32":  # one fused multiply-add ROUNDED to float32: from k = 2^22 on, k 2^-24 + 2^-26 is no float32
            return ((u >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 + 2.0 ** -26).astype(np.float32).astype(np.float64)
        return (u.astype(np.float64) + 0.5) * 2.0 ** -32

    def next(self, idx, wide: bool = False):
        """`wide`: the deviate of GRAa's table look-up, for which both builds take the whole word, (u + 1/2) 2^-32."""
        u = self.u32(idx)
        return (u.astype(np.float64) + 0.5) * 2.0 ** -32 if wide else self.value(u)


class ArrayDeviates:
    """Deviates from a table [item, draw] (the CPU tests feed RANECU doubles this way)."""

    def __init__(self, table):
        self.table = np.asarray(table, dtype=np.float64)
        self.drawn = np.zeros(self.table.shape[0], dtype=np.int64)

    def next(self, idx, wide: bool = False):
        v = self.table[idx, self.drawn[idx]]
        self.drawn[idx] += 1
        return v


# ----------------------------------------------------------------------------------------------------------------------------------
# Rayleigh
# ----------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1.0e-300)


def _rita_interval(t, mat, ru, itn):
    """GRAa's bracketing search from the table's bracket of cell `itn`: (i, smallest relative margin of its comparisons)."""
    i = t["itlco"][itn + mat * NPRAY].astype(np.int64)
    j = t["ituco"][itn + mat * NPRAY].astype(np.int64)
    margin = np.full(ru.shape, np.inf)
    pco = t["pco"].astype(np.float64)
    while True:
        open_ = (j - i) > 1
        if not open_.any():
            return i, margin
        k = (i + j) >> 1
        p = pco[np.where(open_, k - 1, 0) + mat * NPRAY]
        up = ru > p
        margin = np.where(open_, np.minimum(margin, _rel(ru, p)), margin)
        i = np.where(open_ & up, k, i)
        j = np.where(open_ & ~up, k, j)


def rayleigh_replay(t: dict, mat: int, energy, index: int, deviates, n: int | None = None) -> dict:
    """GRAa's loop in float64 (float32 table entries widened where the reference widens them) for n events at one energy, each fed
    its own deviates.  Returns per event: `costh`, `trials`, `margin` = the smallest relative margin of any decision it took (the
    bracket comparisons ru > pco[k - 1], the cut xx < x2max, the acceptance test), and `drawn` = deviates consumed.  The branch of
    xmax < 0.01 needs E < 124 eV, below every table, and is not restated."""
    n = deviates.drawn.size if n is None else n
    e = np.float64(np.float32(energy))
    xmax = e * WAVE
    assert xmax >= 0.01
    xl = np.float64(t["xco"][(mat + 1) * NPRAY - 1])
    x2max = min(xmax * xmax, xl)
    pmax = np.float64(t["pmax"][(index + 1) * MAXMAT + mat])
    pco, xco, aco, bco = (t[k][mat * NPRAY:(mat + 1) * NPRAY] for k in ("pco", "xco", "aco", "bco"))
    dp = np.append(pco[1:] - pco[:-1], np.float32(0)).astype(np.float64)      # float32 differences, widened
    dx = np.append(xco[1:] - xco[:-1], np.float32(0)).astype(np.float64)
    ab1 = (aco + np.float32(1.0) + bco).astype(np.float64)
    pco64, xco64, aco64, bco64 = (v.astype(np.float64) for v in (pco, xco, aco, bco))
    costh = np.zeros(n)
    trials = np.zeros(n, dtype=np.int64)
    margin = np.full(n, np.inf)
    active = np.arange(n)
    while active.size:
        ru = deviates.next(active, wide=True) * pmax
        cell = ru * (NPRAY - 1)
        itn = cell.astype(np.int64)
        i, m = _rita_interval(t, mat, ru, itn)
        # the cell itself is a rounded product: where it lies within 1e-5 of a border, the neighbour's bracket must lead to the same interval
        near = np.abs(cell - np.rint(cell)) <= 1.0e-5 * np.maximum(cell, 1.0)
        if near.any():
            other = np.clip(np.where(cell - np.floor(cell) < 0.5, itn - 1, itn + 1), 0, NPRAY - 2)[near]
            i2, m2 = _rita_interval(t, mat, ru[near], other)
            m[near] = np.where(i2 == i[near], np.minimum(m[near], m2), 0.0)
        q = i - 1
        rr = ru - pco64[q]
        d = dp[q]
        with np.errstate(divide="ignore", invalid="ignore"):
            xx = np.where(rr > 1e-16, xco64[q] + ab1[q] * d * rr / (d * d + (aco64[q] * d + bco64[q] * rr) * rr) * dx[q], xco64[q])
        m = np.minimum(m, _rel(xx, x2max))
        inside = xx < x2max
        c = 1.0 - 2.0 * xx / x2max
        g = (c * c + 1.0) * 0.5
        xi = np.ones(active.size)
        xi[inside] = deviates.next(active[inside])
        m = np.where(inside, np.minimum(m, _rel(xi, g)), m)
        ok = inside & (xi < g)
        trials[active] += 1
        margin[active] = np.minimum(margin[active], m)
        costh[active[ok]] = c[ok]
        active = active[~ok]
    return {"costh": costh, "trials": trials, "margin": margin, "drawn": deviates.drawn.copy()}


# ----------------------------------------------------------------------------------------------------------------------------------
# Compton
# ----------------------------------------------------------------------------------------------------------------------------------
def compton_profiles(t: dict, mat: int, energy, cdt):
    """f_i and n_i(E, cdt) (K.cu:1340-1366) of every shell of the material in float64: arrays [shell], [shell, len(cdt)]."""
    e = np.float64(np.float32(energy))
    cdt = np.atleast_1d(np.asarray(cdt, dtype=np.float64))
    nosc = int(t["noscco"][mat])
    sh = mat + MAXMAT * np.arange(nosc)
    f, ui, fj0 = (t[k][sh].astype(np.float64)[:, None] for k in ("fco", "uico", "fj0"))
    aux = e * (e - ui) * cdt[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        pz = np.where((aux > 1.0e-12) | (ui > 1.0e-12), fj0 * (aux - ui * MC2) / (np.sqrt(aux + aux + ui * ui) * MC2), 0.002)
    r2, h2 = np.sqrt(2.0), np.sqrt(0.5)
    prof = np.where(pz > 0, 1.0 - 0.5 * np.exp(0.5 - (r2 * pz + h2) ** 2), 0.5 * np.exp(0.5 - (h2 - r2 * pz) ** 2))
    return f[:, 0], np.where(ui < e, prof, 0.0)


def compton_s(t: dict, mat: int, energy, cdt):
    """S(E, theta) = sum_i f_i n_i(E, cdt), cdt = 1 - cos(theta)."""
    f, prof = compton_profiles(t, mat, energy, cdt)
    return f @ prof


def _law_density(t, mat, energy, tau):
    """envelope(tau) T(tau) S(E, tau), up to a constant: what GCOa's angle loop accepts (K.cu:1316-1372)."""
    ek = np.float64(np.float32(energy)) * INV_MC2
    ek2, ek3 = 2.0 * ek + 1.0, ek * ek
    cdt = np.minimum((1.0 - tau) / (tau * ek), 2.0)
    envelope = 1.0 / tau + tau            # the mixture of 1 / tau and tau on [taumin, 1] with the reference's weights a1 : a2
    T = (1.0 + tau * ((ek3 - ek2 - 1.0) + tau * (ek2 + tau * ek3))) / (ek3 * tau * (tau * tau + 1.0))
    return envelope * T * compton_s(t, mat, energy, cdt)


def compton_angular_law(energy, mat: int, edges, t: dict, order: int = 48):
    """Probability of each bin [edges[k], edges[k + 1]) of cos(theta) under the reference's Compton law: the density above integrated in
    float64 with a Gauss-Legendre rule of `order` points per bin in tau (the density is smooth in tau), normalised over [-1, 1]."""
    ek = np.float64(np.float32(energy)) * INV_MC2
    x, w = np.polynomial.legendre.leggauss(order)

    def integral(c_lo, c_hi):
        # cos = 1 - (1 - tau) / (tau ek)  <=>  tau = 1 / (1 + ek (1 - cos))
        a, b = 1.0 / (1.0 + ek * (1.0 - c_lo)), 1.0 / (1.0 + ek * (1.0 - c_hi))
        tau = 0.5 * (a + b) + 0.5 * (b - a) * x
        return 0.5 * (b - a) * float(np.sum(w * _law_density(t, mat, energy, tau)))

    edges = np.asarray(edges, dtype=np.float64)
    fine = np.linspace(-1.0, 1.0, 257)
    total = sum(integral(fine[k], fine[k + 1]) for k in range(256))
    out = np.empty(edges.size - 1)
    for k in range(edges.size - 1):
        lo, hi = max(edges[k], -1.0), min(edges[k + 1], 1.0)
        cuts = np.linspace(lo, hi, 5)     # four panels per bin: the quantile bins of the forward peak are wide in tau
        out[k] = sum(integral(cuts[m], cuts[m + 1]) for m in range(4)) / total
    return out


def compton_first_tau(energy, xi0, xi1):
    """tau of the first trial of an event (K.cu:1318-1327) from its first two deviates, and the relative margin of the choice of the
    branch.  cos(theta) of that trial is 1 - (1 - tau) / (tau ek)."""
    ek = np.float64(np.float32(energy)) * INV_MC2
    ek2 = 2.0 * ek + 1.0
    taumin = 1.0 / ek2
    a1 = np.log(ek2)
    lhs = xi0 * (a1 + 2.0 * ek * (ek + 1.0) * taumin * taumin)
    tau = np.where(lhs < a1, taumin ** xi1, np.sqrt(1.0 + xi1 * (taumin * taumin - 1.0)))
    return tau, _rel(lhs, a1)
