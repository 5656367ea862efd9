"""FDK (csrc/fdk.hip) at the launch shapes the reference's `rtkfdk` call takes, against the float64 oracle (oracle/fdk_oracle.py).
test_fdk.py pins every stage on small detectors (96 columns, at most 120 projections, volumes of 64 voxels or fewer per axis); the
configurations here reach what those do not:
  ref_shape        the reference's detector (1024 x 768 pixels of 0.388 mm, offset -159.856 mm, pixel origin -n d / 2 of the stacks
                   written here), pad 1, hann 1, hannY 1, 464 x 250 x 464 voxels of 1 mm, 70 projections: two back-projection
                   x-blocks, the hipFFT ramp at L = 7500, the direct LDS ramp at nu_e = 5545 (over 64 KiB of LDS), chunks 32 + 32 + 6
                   and 64 + 6, a ragged back-projection batch, voxels off the detector in u and in v
  ref_angles       the reference's 894 angles on full 1024-column rows (24 of them) and a thin volume inside those rows: every
                   chunk and hipFFT plan boundary of both routes (27 x 32 + 30, 13 x 64 + 62)
  pad_flip         offsets for which -2 off / du is an integer, so that the float32 offset pads one column more than the double one
  left_pad_fft     a positive offset (zero columns on the left) with pad > 0
  varying_offsets  per-projection offset_x and offset_y
  explicit_origin  an off-centre origin, nx = 300 (a partial second x-block), ny = 1
  thin_detector    nv = 2 and 3 under the 3- and 17-tap hannY kernels (edge replication), odd nu (row tails of ramp_rows_kernel)
  few_views        n = 1, 2, 3
and the C ABI of a caller built against the header before `pad`, and run-to-run determinism.  Each GPU result is held to the oracle at
2e-4 x max|oracle| on its (sub-)grid, outside the voxels where a sample sits within 1e-3 pixel of a detector edge
(fdk_oracle.ambiguous_voxels): there float32 and float64 may take or drop a whole contribution."""
import ctypes as C
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import cases

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import fdk_oracle as fo  # noqa: E402

recon = cases.pkg.reconstruction

TOL = 2e-4        # x max|oracle|: float32 kernels against the float64 oracle (test_fdk.py)
EDGE = 1e-3       # pixel: margin of the ambiguity mask
REF_NU, REF_NV, REF_PIX, REF_OFF = 1024, 768, 0.388, -159.856  # the reference's detector (create_geometry's default offset)
WPC = (0.0, 1.05, 0.01)


class Case:
    """One FDK problem: geometry, a noisy sphere's line integrals (float32), volume grid, filter settings and the voxel sub-grid
    (ix, iy, iz; None = all) on which the kernels are compared with the oracle."""

    def __init__(self, name, geo, nu, nv, du, dim, spacing, pixel_origin=None, origin=None, hann=1.0, hann_y=1.0, pad=0.0, sub=(None, None, None),
                 sphere=(0.02, 60.0, (20.0, 5.0, -10.0)), noise=0.05, seed=5):
        self.name, self.geo, self.nu, self.nv, self.du, self.dv = name, geo, nu, nv, du, du
        self.dim, self.spacing, self.origin, self.hann, self.hann_y, self.pad, self.sub = tuple(dim), tuple(spacing), origin, hann, hann_y, pad, sub
        self.u0, self.v0 = pixel_origin if pixel_origin is not None else (-(nu - 1) / 2 * du, -(nv - 1) / 2 * du)
        self.sphere, self.noise, self.seed = sphere, noise, seed

    @property
    def n(self):
        return len(self.geo.gantry_angles)

    def geometry_args(self):
        g = self.geo
        return (self.du, self.dv, self.u0, self.v0, g.source_to_isocenter, g.source_to_detector, np.asarray(g.gantry_angles),
                np.asarray(g.projection_offsets_x), np.asarray(g.projection_offsets_y))

    def projections(self):
        mu, radius, centre = self.sphere
        du, dv, u0, v0, sid, sdd, ang, ox, oy = self.geometry_args()
        p = fo.sphere_projections(mu, radius, centre, self.n, self.nu, self.nv, du, dv, u0, v0, sid, sdd, ang, ox, oy).astype(np.float32)
        p += (self.noise * np.random.default_rng(self.seed).standard_normal(size=p.shape, dtype=np.float32))
        return p

    def oracle(self, proj, wpc=None, pad=None):
        du, dv, u0, v0, sid, sdd, ang, ox, oy = self.geometry_args()
        return fo.reconstruct(proj, du, dv, u0, v0, sid, sdd, ang, ox, oy, self.dim, self.spacing, self.origin, hann=self.hann, hann_y=self.hann_y,
                              wpc=wpc, pad=self.pad if pad is None else pad, ramp="fft", ix=self.sub[0], iy=self.sub[1], iz=self.sub[2])

    def ambiguous(self):
        du, dv, u0, v0, sid, sdd, ang, ox, oy = self.geometry_args()
        return fo.ambiguous_voxels(self.nu, self.nv, du, dv, u0, v0, sid, sdd, ang, ox, oy, self.dim, self.spacing, self.origin,
                                   ix=self.sub[0], iy=self.sub[1], iz=self.sub[2], delta=EDGE)

    def hip(self, proj, wpc=None, pad=None):
        vol, _ = recon.fdk(proj, self.geo, (self.du, self.dv), (self.u0, self.v0), self.dim, self.spacing, self.origin, self.hann, self.hann_y,
                           wpc, pad=self.pad if pad is None else pad)
        return self.pick(vol)

    def pick(self, vol):
        ix, iy, iz = (np.arange(n) if i is None else np.asarray(i) for n, i in zip(self.dim, self.sub))
        return vol[np.ix_(iz, iy, ix)]


def _geometry(angles, off_x, off_y=0.0):
    g = recon.CircularGeometry(1000.0, 1500.0)
    off_x, off_y = np.broadcast_to(off_x, (len(angles),)), np.broadcast_to(off_y, (len(angles),))
    for a, ox, oy in zip(angles, off_x, off_y):
        g.add_projection(a, ox, oy)
    return g


def _ref_xz():
    """x / z indices of the reference-size sub-grid: both faces, both sides of the x-block boundary at 256, the centre, a coarse
    sweep, and the indices where the field-of-view circle (232.8 mm) meets the outer rows and columns."""
    return np.unique(np.r_[0, 1, 2, 205, 206, 207, 208, 230, 231, 232, 233, 254, 255, 256, 257, 258, 461, 462, 463, np.arange(12, 460, 23)])


@lru_cache(maxsize=None)
def case(name):
    if name == "ref_shape":
        iy = [0, 1, 62, 124, 125, 187, 248, 249]
        return Case(name, recon.create_geometry(70, start_angle=90.0), REF_NU, REF_NV, REF_PIX, (464, 250, 464), (1.0, 1.0, 1.0),
                    pixel_origin=(-REF_NU * REF_PIX / 2, -REF_NV * REF_PIX / 2), pad=1.0, sub=(_ref_xz(), iy, _ref_xz()),
                    sphere=(0.02, 250.0, (6.0, 4.0, -9.0)))
    if name == "ref_angles":
        xz = np.unique(np.r_[0, 255, 256, 463, np.arange(9, 460, 29)])
        return Case(name, recon.create_geometry(894, start_angle=90.0), REF_NU, 24, REF_PIX, (464, 6, 464), (1.0, 0.7, 1.0),
                    pixel_origin=(-REF_NU * REF_PIX / 2, -24 * REF_PIX / 2), pad=1.0, sub=(xz, None, xz), sphere=(0.02, 250.0, (6.0, 1.0, -9.0)))
    if name.startswith("pad_flip"):  # pad_flip_<offset>_<pad>
        off, pad = (float(v) for v in name.split("_")[2:])
        return Case(name, recon.create_geometry(90, start_angle=90.0, detector_offset_x=off), 96, 64, 3.88, (48, 30, 40), (5.0, 5.0, 6.0), pad=pad)
    if name == "left_pad_fft":
        return Case(name, recon.create_geometry(90, start_angle=90.0, detector_offset_x=80.0), 96, 64, 4.0, (48, 30, 40), (5.0, 5.0, 6.0), pad=0.5)
    if name == "varying_offsets":
        k = np.arange(90)
        geo = _geometry(90.0 + 4.0 * k, -80.0 + 5.0 * np.sin(0.61 * k), 3.0 + 2.0 * np.cos(0.37 * k))
        return Case(name, geo, 96, 64, 4.0, (48, 30, 40), (5.0, 5.0, 6.0), pad=0.5)
    if name == "explicit_origin":
        return Case(name, recon.create_geometry(90, start_angle=90.0, detector_offset_x=-80.0), 96, 64, 4.0, (300, 1, 40), (0.8, 2.0, 5.0),
                    origin=(-100.0, 12.5, -90.0), pad=0.5)
    if name.startswith("thin"):  # thin_<nv>_<hann_y>
        nv, hann_y = int(name.split("_")[1]), float(name.split("_")[2])
        return Case(name, recon.create_geometry(60, start_angle=90.0, detector_offset_x=0.0), 97, nv, 4.0, (40, 3, 40), (5.0, 0.5, 5.0),
                    hann_y=hann_y)
    if name.startswith("views"):  # views_<n>
        angles = {1: [90.0], 2: [90.0, 270.0], 3: [90.0, 160.0, 300.0]}[int(name.split("_")[1])]
        return Case(name, _geometry(angles, -80.0), 96, 64, 4.0, (48, 30, 40), (5.0, 5.0, 6.0), pad=0.5)
    raise KeyError(name)


PAD_FLIP = ["pad_flip_-11.64_0", "pad_flip_-11.64_1", "pad_flip_-79.54_1"]
SMALL = PAD_FLIP + ["left_pad_fft", "varying_offsets", "explicit_origin", "thin_2_1", "thin_2_0.5", "thin_3_1", "thin_3_0.5", "views_1",
                    "views_2", "views_3"]


def launch(c, direct=False):
    """fdk.hip's host rules for a case: symmetric padding (from the double offsets), rtkfdk --pad extension, the hipFFT row length L,
    the LDS image of the direct ramp, the chunks of projections and the back-projection x-blocks."""
    ox = np.asarray(c.geo.projection_offsets_x, dtype=np.float64)
    pad_l, pad_r = fo.symmetric_padding(c.nu, c.du, c.u0, float(ox.min()), float(ox.max()))
    nu_p = c.nu + pad_l + pad_r
    nxt = min(int(np.ceil(c.pad * nu_p)), nu_p - 1) if c.pad > 0 else 0
    nu_e = nu_p + 2 * nxt
    L = max(2 * (nu_p + nxt - 1) + 1, nu_e)
    while L % 2 or fo.fast_length(L) != L:
        L += 1
    chunk = min(c.n, 64 if direct else 32)
    chunks = [min(chunk, c.n - f) for f in range(0, c.n, chunk)]
    return dict(pad=(pad_l, pad_r), nu_p=nu_p, next=nxt, nu_e=nu_e, L=L, lds=(3 * nu_e + 2) * 4, chunks=chunks,
                batches=[min(8, m - b) for m in chunks for b in range(0, m, 8)], x_blocks=(c.dim[0] + 255) // 256)


def _compare(c, got, want, amb, label=""):
    scale = np.abs(want).max()
    err = float(np.abs(np.where(amb, 0.0, got.astype(np.float64) - want)).max() / scale)
    print(f"{c.name}{label}: max |hip - oracle| / max |oracle| = {err:.3e} outside {int(amb.sum())} of {amb.size} voxels within {EDGE} pixel of an edge")
    assert got.shape == want.shape and scale > 0
    assert amb.mean() < 0.01
    assert err < TOL, err
    return err


# ---------------------------------------------------------------------------------------------------------------- CPU: the oracle
def _small_half_fan(n=24, off_x=-80.0):
    c = Case("pin", recon.create_geometry(n, start_angle=90.0, detector_offset_x=off_x), 96, 40, 4.0, (24, 10, 20), (5.0, 5.0, 6.0))
    return c, c.projections()


def test_fft_ramp_equals_the_direct_ramp():
    """ramp_rows 'fft' against np.convolve: rows directly (rel 1e-13 of the largest output), and whole reconstructions (half-fan
    on both sides, pad > 0, Hann on and off) at 1e-12 of max |volume|."""
    rng = np.random.default_rng(3)
    for nu_e, first, count in ((97, 0, 97), (200, 50, 100), (1001, 333, 335)):
        rows = rng.normal(size=(3, nu_e))
        for hann in (0.0, 1.0, 0.6):
            h = fo.ramp_kernel(nu_e - 1, hann)
            a, b = fo.ramp_rows(rows, h, first, count, "direct"), fo.ramp_rows(rows, h, first, count, "fft")
            assert a.shape == b.shape == (3, count)
            assert np.abs(a - b).max() < 1e-13 * np.abs(a).max()
    for off_x, pad, hann, hann_y in ((-80.0, 1.0, 1.0, 1.0), (80.0, 0.5, 0.0, 0.0), (-150.0, 0.3, 0.7, 0.5)):
        c, proj = _small_half_fan(off_x=off_x)
        du, dv, u0, v0, sid, sdd, ang, ox, oy = c.geometry_args()
        kw = dict(hann=hann, hann_y=hann_y, pad=pad, wpc=WPC)
        a = fo.reconstruct(proj, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, ramp="direct", **kw)
        b = fo.reconstruct(proj, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, ramp="fft", **kw)
        assert np.abs(a - b).max() < 1e-12 * np.abs(a).max(), (off_x, float(np.abs(a - b).max() / np.abs(a).max()))
    assert fo.fast_length(7393) == 7500 and fo.fast_length(11089) == 11250 and fo.fast_length(1) == 1


def test_sub_grid_equals_the_full_volume():
    """The oracle on an index sub-grid (unsorted, repeated indices, explicit origin) returns exactly those voxels of the full
    volume: the same arithmetic, bit for bit."""
    c, proj = _small_half_fan()
    du, dv, u0, v0, sid, sdd, ang, ox, oy = c.geometry_args()
    ix, iy, iz = [23, 0, 11, 11, 5], [9, 0, 4], [0, 19, 7]
    for origin in (None, (-40.0, -3.0, -70.0)):
        kw = dict(hann=1.0, hann_y=1.0, pad=0.5, origin=origin)
        full = fo.reconstruct(proj, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, **kw)
        sub = fo.reconstruct(proj, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, ix=ix, iy=iy, iz=iz, **kw)
        np.testing.assert_array_equal(sub, full[np.ix_(iz, iy, ix)])
        amb_full = fo.ambiguous_voxels(c.nu, c.nv, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, origin, delta=0.05)
        amb_sub = fo.ambiguous_voxels(c.nu, c.nv, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, origin, ix=ix, iy=iy, iz=iz, delta=0.05)
        np.testing.assert_array_equal(amb_sub, amb_full[np.ix_(iz, iy, ix)])


def test_ambiguity_mask():
    """ambiguous_voxels against an independent evaluation through the projection matrices of the geometry file
    (CircularGeometry.matrix) on a half-fan case with varying offsets; a voxel put exactly on the padded detector's first column,
    and one exactly on the last row, are marked, and each stops being marked half a pixel away."""
    k = np.arange(12)
    geo = _geometry(30.0 * k + 7.0, -80.0 + 3.0 * np.sin(k), 1.5 * np.cos(k))
    c = Case("mask", geo, 96, 40, 4.0, (20, 8, 18), (20.0, 15.0, 20.0))  # corners off the detector in u and in v
    du, dv, u0, v0, sid, sdd, ang, ox, oy = c.geometry_args()
    delta = 0.2  # wide, so that the mask is not empty on this grid
    got = fo.ambiguous_voxels(c.nu, c.nv, du, dv, u0, v0, sid, sdd, ang, ox, oy, c.dim, c.spacing, delta=delta)
    pad_l, pad_r = fo.symmetric_padding(c.nu, du, u0, ox.min(), ox.max())
    nu_p, u0_p = c.nu + pad_l + pad_r, u0 - pad_l * du
    X, Y, Z = fo.volume_axes(c.dim, c.spacing)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    pts = np.stack([xx.ravel(), yy.ravel(), zz.ravel(), np.ones(xx.size)])
    want = np.zeros(xx.size, dtype=bool)
    for i in range(len(ang)):
        uvw = geo.matrix(i) @ pts
        fu, fv = (uvw[0] / uvw[2] - u0_p) / du, (uvw[1] / uvw[2] - v0) / dv
        u_in, v_in = (fu > -delta) & (fu < nu_p - 1 + delta), (fv > -delta) & (fv < c.nv - 1 + delta)
        u_edge = (np.abs(fu) < delta) | (np.abs(fu - (nu_p - 1)) < delta)
        v_edge = (np.abs(fv) < delta) | (np.abs(fv - (c.nv - 1)) < delta)
        want |= (u_edge & v_in) | (v_edge & u_in)
    np.testing.assert_array_equal(got.ravel(), want)
    assert 0 < got.sum() < 0.2 * got.size
    # one projection at angle 0, offset 0: x' = X, z' = Z; a voxel at X with sdd X / sid = u0_p projects onto column 0
    u0c = -(96 - 1) / 2 * 4.0
    for x, marked in ((u0c * 1000.0 / 1500.0, True), ((u0c + 2.0) * 1000.0 / 1500.0, False)):
        m = fo.ambiguous_voxels(96, 40, 4.0, 4.0, u0c, -78.0, 1000.0, 1500.0, [0.0], [0.0], [0.0], (1, 1, 1), (1.0, 1.0, 1.0), (x, 0.0, 0.0))
        assert bool(m[0, 0, 0]) == marked, x
    for y, marked in ((78.0 * 1000.0 / 1500.0, True), (76.0 * 1000.0 / 1500.0, False)):  # last row: v = v0 + 39 dv = 78
        m = fo.ambiguous_voxels(96, 40, 4.0, 4.0, u0c, -78.0, 1000.0, 1500.0, [0.0], [0.0], [0.0], (1, 1, 1), (1.0, 1.0, 1.0), (0.0, y, 0.0))
        assert bool(m[0, 0, 0]) == marked, y


# ---------------------------------------------------------------------------------------------------------------- CPU: what each case reaches
def test_configurations_reach_the_launch_shapes():
    ref = case("ref_shape")
    f, d = launch(ref), launch(ref, direct=True)
    assert f["pad"] == (0, 825) and f["nu_e"] == 5545 and f["L"] == 7500
    assert d["lds"] > 64 * 1024                                   # the direct ramp needs the hipFuncSetAttribute branch
    assert f["chunks"] == [32, 32, 6] and d["chunks"] == [64, 6] and f["batches"][-1] == 6 and f["x_blocks"] == 2
    ix, iy, iz = ref.sub
    assert {0, 463} <= set(ix) and {0, 249} <= set(iy) and {0, 463} <= set(iz) and {124, 125} <= set(iy)
    assert {255, 256} <= set(ix)                                  # both sides of the x-block boundary
    # the field-of-view circle: the ray through the outer pixel passes the isocentre at sid |u| / sqrt(sdd^2 + u^2)
    u_out = abs(ref.u0 + REF_OFF)
    r_fov = 1000.0 * u_out / np.hypot(1500.0, u_out)
    X, _, Z = fo.volume_axes(ref.dim, ref.spacing, None, ix, None, iz)
    r = np.hypot(X[None, :], Z[:, None])
    assert ((r > r_fov - 1.5) & (r < r_fov)).any() and ((r > r_fov) & (r < r_fov + 1.5)).any() and (r > r_fov + 50).any()
    # rows near the source project past the 768 detector rows
    assert 2.0 * 124.5 > REF_NV * REF_PIX / 2
    ang = case("ref_angles")
    assert launch(ang)["chunks"] == [32] * 27 + [30] and launch(ang, direct=True)["chunks"] == [64] * 13 + [62]
    assert launch(case("left_pad_fft"))["pad"][0] > 0 and launch(case("left_pad_fft"))["next"] > 0
    vo = case("varying_offsets")
    assert np.ptp(vo.geo.projection_offsets_x) > 5.0 and min(np.abs(vo.geo.projection_offsets_y)) > 0.5 and np.ptp(vo.geo.projection_offsets_y) > 2.0
    eo = case("explicit_origin")
    assert eo.dim[0] % 256 != 0 and launch(eo)["x_blocks"] == 2 and eo.dim[1] == 1
    assert tuple(eo.origin) != tuple(fo.volume_axes(eo.dim, eo.spacing)[i][0] for i in range(3))
    for name in ("thin_2_1", "thin_3_0.5"):
        assert launch(case(name))["nu_e"] % 4 != 0 and case(name).nv < fo.hann_y_kernel(0.5).size
    assert [case(f"views_{n}").n for n in (1, 2, 3)] == [1, 2, 3]
    for name in ["ref_shape", "ref_angles"] + SMALL:  # the comparisons leave out less than 1 % of their voxels
        assert case(name).ambiguous().mean() < 0.01, name


@pytest.mark.parametrize("name", PAD_FLIP)
def test_pad_flip_offsets_flip_the_padding_under_float32(name):
    """The offsets of pad_flip make -2 off / du an integer: in double the padding is k columns, with the offset rounded to float32
    k + 1 (what fdk.hip computed before it took the double offsets) -- the same flip as at the reference's own geometry."""
    c = case(name)
    off = c.geo.projection_offsets_x[0]
    exact = fo.symmetric_padding(c.nu, c.du, c.u0, off, off)
    rounded = float(np.float32(off))
    assert fo.symmetric_padding(c.nu, c.du, c.u0, rounded, rounded) == (exact[0], exact[1] + 1)
    assert launch(c)["pad"] == exact
    ref = case("ref_shape")
    r32 = float(np.float32(REF_OFF))
    assert fo.symmetric_padding(REF_NU, REF_PIX, ref.u0, REF_OFF, REF_OFF) == (0, 825)
    assert fo.symmetric_padding(REF_NU, REF_PIX, ref.u0, r32, r32) == (0, 826)


# ---------------------------------------------------------------------------------------------------------------- GPU
@lru_cache(maxsize=None)
def _inputs(name):
    c = case(name)
    return c.projections()


@lru_cache(maxsize=None)
def _oracle(name, wpc=None, pad=None):
    c = case(name)
    return c.oracle(_inputs(name), wpc, pad), c.ambiguous()


def _route(monkeypatch, direct):
    if direct:
        monkeypatch.setenv("MCGPU_FDK_DIRECT_RAMP", "1")
    else:
        monkeypatch.delenv("MCGPU_FDK_DIRECT_RAMP", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
def test_ref_shape(engine, direct, monkeypatch):
    """The reference's launch shape on both ramp routes."""
    _route(monkeypatch, direct)
    want, amb = _oracle("ref_shape")
    _compare(case("ref_shape"), case("ref_shape").hip(_inputs("ref_shape")), want, amb, " direct" if direct else " fft")


@pytest.mark.gpu
def test_ref_shape_with_water_precorrection(engine, monkeypatch):
    _route(monkeypatch, False)
    want, amb = _oracle("ref_shape", WPC)
    _compare(case("ref_shape"), case("ref_shape").hip(_inputs("ref_shape"), WPC), want, amb, " wpc")


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
def test_ref_shape_is_deterministic(engine, direct, monkeypatch):
    """No atomics anywhere: two runs give the same volume bit for bit."""
    _route(monkeypatch, direct)
    c, proj = case("ref_shape"), _inputs("ref_shape")
    a, _ = recon.fdk(proj, c.geo, (c.du, c.dv), (c.u0, c.v0), c.dim, c.spacing, None, c.hann, c.hann_y, pad=c.pad)
    b, _ = recon.fdk(proj, c.geo, (c.du, c.dv), (c.u0, c.v0), c.dim, c.spacing, None, c.hann, c.hann_y, pad=c.pad)
    assert a.tobytes() == b.tobytes()
    assert np.isfinite(a).all() and np.abs(a).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
def test_ref_angles(engine, direct, monkeypatch):
    _route(monkeypatch, direct)
    want, amb = _oracle("ref_angles")
    _compare(case("ref_angles"), case("ref_angles").hip(_inputs("ref_angles")), want, amb, " direct" if direct else " fft")


@pytest.mark.gpu
@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
@pytest.mark.parametrize("name", SMALL)
def test_small_configuration(engine, name, direct, monkeypatch):
    _route(monkeypatch, direct)
    want, amb = _oracle(name)
    _compare(case(name), case(name).hip(_inputs(name)), want, amb, " direct" if direct else " fft")


def _fdk_with_struct_size(c, proj, struct_size, pad):
    """mcgpu_fdk_reconstruct through ctypes as a caller compiled against a header whose struct ends at `struct_size` bytes would call
    it; the options memory holds `pad` whatever the size says."""
    lib = cases.pkg.engine.load_library()
    lib.mcgpu_fdk_reconstruct.argtypes = [C.POINTER(recon._FdkOptions), C.c_void_p, C.c_void_p, C.POINTER(recon._FdkReport)]
    lib.mcgpu_fdk_reconstruct.restype = C.c_int
    p = np.ascontiguousarray(proj, dtype=np.float32)
    keep = [np.ascontiguousarray(v, dtype=np.float64) for v in (c.geo.gantry_angles, c.geo.projection_offsets_x, c.geo.projection_offsets_y)]
    dp = C.POINTER(C.c_double)
    o = recon._FdkOptions(struct_size, c.n, c.nu, c.nv, c.du, c.dv, c.u0, c.v0, c.geo.source_to_isocenter, c.geo.source_to_detector,
                          *(a.ctypes.data_as(dp) for a in keep), *c.dim, *c.spacing, *(float("nan"),) * 3, c.hann, c.hann_y, None, 0, 0, pad)
    vol = np.zeros(c.dim[::-1], dtype=np.float32)
    cases.pkg.engine._check(lib.mcgpu_fdk_reconstruct(C.byref(o), p.ctypes.data, vol.ctypes.data, C.byref(recon._FdkReport())))
    return vol


@pytest.mark.gpu
def test_old_header_reads_pad_as_zero(engine, monkeypatch):
    """A caller built against the header before `pad` passes a struct that ends where `pad` begins: whatever lies beyond reads as 0,
    so the result is bit for bit the one of pad = 0 -- and pad = 1 with the full struct really is different."""
    _route(monkeypatch, False)
    c, proj = case("left_pad_fft"), _inputs("left_pad_fft")
    full = C.sizeof(recon._FdkOptions)
    old = recon._FdkOptions.pad.offset
    assert old + 8 == full
    zero = _fdk_with_struct_size(c, proj, full, 0.0)
    assert _fdk_with_struct_size(c, proj, old, 1.0).tobytes() == zero.tobytes()
    one = _fdk_with_struct_size(c, proj, full, 1.0)
    assert np.abs(one - zero).max() > 1e-3 * np.abs(zero).max()
    vol, _ = recon.fdk(proj, c.geo, (c.du, c.dv), (c.u0, c.v0), c.dim, c.spacing, None, c.hann, c.hann_y, pad=0.0)
    assert vol.tobytes() == zero.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the C ABI's refusals
class _Tiny:
    """mcgpu_fdk_reconstruct through ctypes on the smallest valid problem (one projection, 2 x 2 pixels, one voxel); keyword
    arguments replace fields of mcgpu_fdk_options."""

    def __init__(self):
        self.lib = cases.pkg.engine.load_library()
        self.lib.mcgpu_fdk_reconstruct.argtypes = [C.POINTER(recon._FdkOptions), C.c_void_p, C.c_void_p, C.POINTER(recon._FdkReport)]
        self.lib.mcgpu_fdk_reconstruct.restype = C.c_int
        self.angle = np.array([30.0])
        self.proj = np.array([[[1.0, 2.0], [3.0, 4.0]]], np.float32)

    def options(self, **fields):
        o = recon._FdkOptions(C.sizeof(recon._FdkOptions), 1, 2, 2, 4.0, 4.0, -2.0, -2.0, 1000.0, 1500.0, self.angle.ctypes.data_as(C.POINTER(C.c_double)),
                              None, None, 1, 1, 1, 1.0, 1.0, 1.0, *(float("nan"),) * 3, 0.0, 0.0, None, 0, 0, 0.0)
        for k, v in fields.items():
            setattr(o, k, v)
        return o

    def __call__(self, o, projections=True, volume=True):
        vol = np.full((1, 1, 1), -1.0, np.float32)
        rc = self.lib.mcgpu_fdk_reconstruct(C.byref(o) if o is not None else None, self.proj.ctypes.data if projections else None,
                                            vol.ctypes.data if volume else None, None)
        return rc, vol, self.lib.mcgpu_last_error().decode(errors="replace")


_SET_SIZE = "!!ERROR!! mcgpu_fdk_reconstruct: set mcgpu_fdk_options.struct_size = sizeof(mcgpu_fdk_options)"
_BAD = "!!ERROR!! mcgpu_fdk_reconstruct: bad argument"


@pytest.mark.parametrize("what, message", [("options", _SET_SIZE), ("struct_size", _SET_SIZE), ("projections", _BAD), ("volume", _BAD), ("n_proj", _BAD),
                                           ("nu", _BAD), ("du", _BAD), ("gantry_deg", _BAD)])
def test_abi_refuses_before_any_hip_call(engine, what, message):
    """-1 and the message, with the volume untouched; runs without a device, so nothing of HIP was asked."""
    call = _Tiny()
    over = {"struct_size": dict(struct_size=0), "n_proj": dict(n_proj=0), "nu": dict(nu=1), "du": dict(du=0.0),
            "gantry_deg": dict(gantry_deg=C.POINTER(C.c_double)())}.get(what, {})
    rc, vol, msg = call(None if what == "options" else call.options(**over), projections=what != "projections", volume=what != "volume")
    assert rc == -1 and msg == message and np.all(vol == -1.0)


def test_abi_a_device_that_does_not_exist_is_an_error_return(engine):
    """Device 9999: the runtime's refusal comes back as -1 with the failing call in the message (no GPU is needed to be refused)."""
    call = _Tiny()
    rc, vol, msg = call(call.options(device=9999))
    assert rc == -1 and "!!HIP ERROR!! hipSetDevice" in msg and np.all(vol == -1.0)


@pytest.mark.gpu
def test_abi_a_valid_call_follows_a_refused_device(engine):
    call = _Tiny()
    assert call(call.options(device=9999))[0] == -1
    rc, vol, msg = call(call.options())
    assert rc == 0, msg
    assert np.isfinite(vol).all() and vol[0, 0, 0] > 0
