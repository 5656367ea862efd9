"""The water pre-correction fit (csrc/wpc_fit.hip, water_precorrection.py) restated in float64 on top of the FDK
oracle (oracle/fdk_oracle.py), and the problems the tests of the fit share.  TEST INFRASTRUCTURE.

The rule: f_n = FDK(q with wpc = e_n), n = 0..N; fbar_n = mean of f_n over the slab's y slices; B[i][j] = sum weight fbar_i fbar_j,
a[i] = sum weight fbar_i template; c = inv(B) a."""
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

import cases

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import fdk_oracle as fo  # noqa: E402

recon = cases.pkg.reconstruction

TOL_REL = 2e-4   # x max|oracle|: float32 kernels against the float64 oracle, the project's FDK tolerance (tests/test_fdk_configs.py)
EDGE = 1e-3      # pixel: margin of fdk_oracle.ambiguous_voxels


# ---------------------------------------------------------------------------------------------------------------- the rule
def unit(n):
    e = np.zeros(n + 1)
    e[n] = 1.0
    return e


def basis_means(proj, du, dv, u0, v0, sid, sdd, gantry_deg, off_x, off_y, dim, spacing, origin, hann, hann_y, pad, slab, order, ramp="fft"):
    """fbar [order + 1][nz][nx] in float64: the oracle's reconstruction of q^n on the slab's slices, averaged over them."""
    iy = np.arange(slab[0], slab[0] + slab[1])
    return np.stack([fo.reconstruct(proj, du, dv, u0, v0, sid, sdd, gantry_deg, off_x, off_y, dim, spacing, origin, hann=hann, hann_y=hann_y,
                                    wpc=unit(n), pad=pad, ramp=ramp, iy=iy).mean(1) for n in range(order + 1)])


def normal_equations(fbar, weight, template):
    fbar, weight, template = (np.asarray(v, dtype=np.float64) for v in (fbar, weight, template))
    B = np.einsum("zx,izx,jzx->ij", weight, fbar, fbar)
    a = np.einsum("zx,izx,zx->i", weight, fbar, template)
    return B, a


def solve(B, a):
    return np.linalg.inv(B).dot(a)


def residual(c, fbar, weight, template):
    image = np.tensordot(np.asarray(c, dtype=np.float64), np.asarray(fbar, dtype=np.float64)[: len(c)], axes=1)
    return float(np.sum(weight * (image - template) ** 2))


# ---------------------------------------------------------------------------------------------------------------- the problems
class Problem:
    """One fit problem: geometry, float32 projections, volume grid, filter settings; weight and template [nz][nx]."""

    def __init__(self, name, geo, nu, nv, du, dim, spacing, proj, origin=None, pad=0.0, hann=1.0, hann_y=1.0, weight=None, template=None):
        self.name, self.geo, self.nu, self.nv, self.du, self.dv = name, geo, nu, nv, du, du
        self.dim, self.spacing, self.origin, self.pad, self.hann, self.hann_y = tuple(dim), tuple(spacing), origin, pad, hann, hann_y
        self.u0, self.v0 = -(nu - 1) / 2 * du, -(nv - 1) / 2 * du
        self.proj = proj(self) if callable(proj) else proj
        X, _, Z = fo.volume_axes(self.dim, self.spacing, origin)
        self.r = np.hypot(X[None, :], Z[:, None])          # [nz][nx]: distance of a pixel from the rotation axis
        rng = np.random.default_rng(11)
        self.weight = weight(self) if weight else rng.uniform(0.0, 1.0, self.r.shape).astype(np.float32)
        self.template = template(self) if template else rng.uniform(0.0, 0.03, self.r.shape).astype(np.float32)

    @property
    def n(self):
        return len(self.geo.gantry_angles)

    def geometry_args(self):
        g = self.geo
        return (self.du, self.dv, self.u0, self.v0, g.source_to_isocenter, g.source_to_detector, np.asarray(g.gantry_angles),
                np.asarray(g.projection_offsets_x), np.asarray(g.projection_offsets_y))

    def oracle(self, slab, order):
        return basis_means(self.proj, *self.geometry_args(), self.dim, self.spacing, self.origin, self.hann, self.hann_y, self.pad, slab, order)

    def left_out(self, slab):
        """[nz][nx]: pixels with a voxel of their slab column within EDGE pixel of a detector edge in some projection."""
        iy = np.arange(slab[0], slab[0] + slab[1])
        return fo.ambiguous_voxels(self.nu, self.nv, *self.geometry_args(), self.dim, self.spacing, self.origin, iy=iy, delta=EDGE).any(1)

    def fdk_args(self):
        """(projections, geometry, pixel_spacing, pixel_origin, dimension, spacing) as reconstruction.fdk and fit_wpc take them."""
        return self.proj, self.geo, (self.du, self.dv), (self.u0, self.v0), self.dim, self.spacing


def _geometry(angles, off_x=0.0, off_y=0.0):
    g = recon.CircularGeometry(1000.0, 1500.0)
    off_x, off_y = np.broadcast_to(off_x, (len(angles),)), np.broadcast_to(off_y, (len(angles),))
    for ang, ox, oy in zip(angles, off_x, off_y):
        g.add_projection(ang, ox, oy)
    return g


def cylinder_chords(p, radius, length):
    """Exact chord lengths [nv][nu] of the rays source -> pixel centre through a cylinder about the y axis (any gantry angle sees the
    same: centred detector, no offsets)."""
    sid, sdd = p.geo.source_to_isocenter, p.geo.source_to_detector
    u = p.u0 + p.du * np.arange(p.nu)
    v = p.v0 + p.dv * np.arange(p.nv)
    dx, dy = np.meshgrid(u, v)
    dz = -sdd
    # source (0, 0, sid) + t (dx, dy, dz): (t dx)^2 + (sid + t dz)^2 = R^2
    qa = dx * dx + dz * dz
    qb = 2.0 * sid * dz
    qc = sid * sid - radius * radius
    disc = qb * qb - 4.0 * qa * qc
    root = np.sqrt(np.maximum(disc, 0.0))
    t1, t2 = (-qb - root) / (2.0 * qa), (-qb + root) / (2.0 * qa)
    with np.errstate(divide="ignore"):
        ty = np.where(dy != 0.0, (length / 2.0) / np.abs(dy), np.inf)  # |y| <= length / 2
    t1, t2 = np.maximum(t1, -ty), np.minimum(t2, ty)
    return np.where((disc > 0.0) & (t2 > t1), (t2 - t1) * np.sqrt(dx * dx + dy * dy + dz * dz), 0.0)


def _two_energy_cylinder(p):
    L = cylinder_chords(p, 60.0, 400.0)
    q = -np.log(0.5 * np.exp(-0.03 * L) + 0.5 * np.exp(-0.015 * L))
    return np.broadcast_to(q.astype(np.float32), (p.n,) + q.shape).copy()


def _noisy_sphere(p):
    du, dv, u0, v0, sid, sdd, ang, ox, oy = p.geometry_args()
    q = fo.sphere_projections(0.02, 60.0, (20.0, 5.0, -10.0), p.n, p.nu, p.nv, du, dv, u0, v0, sid, sdd, ang, ox, oy).astype(np.float32)
    return q + 0.05 * np.random.default_rng(5).standard_normal(size=q.shape, dtype=np.float32)


CENTRED_SLAB = (3, 5)  # y = 3..7


@lru_cache(maxsize=None)
def problem(name):
    if name == "centred":  # a beam-hardened water cylinder: the fit has something to correct
        return Problem(name, _geometry(90.0 + 9.0 * np.arange(40)), 64, 32, 5.0, (40, 12, 40), (4.0, 4.0, 4.0), _two_energy_cylinder,
                       weight=lambda p: ((p.r < 50.0) | ((p.r > 70.0) & (p.r < 78.0))).astype(np.float32),
                       template=lambda p: np.where(p.r < 60.0, 0.02, 0.0).astype(np.float32))
    if name == "half_fan":  # n = 41: chunks 32 + 9, a last batch of one projection
        return Problem(name, recon.create_geometry(41, start_angle=90.0, detector_offset_x=-80.0), 96, 64, 4.0, (48, 30, 40), (5.0, 5.0, 6.0), _noisy_sphere, pad=0.5)
    if name == "wide":      # test_fdk_configs' explicit_origin: a partial second x-block, one slice, off-centre origin
        return Problem(name, recon.create_geometry(90, start_angle=90.0, detector_offset_x=-80.0), 96, 64, 4.0, (300, 1, 40), (0.8, 2.0, 5.0), _noisy_sphere,
                       origin=(-100.0, 12.5, -90.0), pad=0.5)
    if name == "varying_offsets":
        k = np.arange(90)
        return Problem(name, _geometry(90.0 + 4.0 * k, -80.0 + 5.0 * np.sin(0.61 * k), 3.0 + 2.0 * np.cos(0.37 * k)), 96, 64, 4.0, (48, 30, 40), (5.0, 5.0, 6.0),
                       _noisy_sphere, pad=0.5)
    raise KeyError(name)


# (problem, slab, highest order): every basis the GPU tests compare; a lower order's basis is the first rows of a higher one's
GPU_CASES = [("centred", CENTRED_SLAB, 5), ("half_fan", (0, 1), 7), ("half_fan", (0, 30), 7), ("half_fan", (27, 3), 7), ("wide", (0, 1), 2),
             ("varying_offsets", (11, 8), 3)]


@lru_cache(maxsize=None)
def oracle_basis(name, slab, order):
    """(fbar [order + 1][nz][nx] float64, left-out pixels [nz][nx]); computed once, shared, never written to."""
    fbar, out = problem(name).oracle(slab, order), problem(name).left_out(slab)
    fbar.setflags(write=False)
    out.setflags(write=False)
    return fbar, out
