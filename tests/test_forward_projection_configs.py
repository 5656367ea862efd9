"""The Joseph forward projector (csrc/forward_project.hip, csrc/joseph_ray.inc) at the launch shapes the reference's
`project_forward` call takes and at the edges of its host rules and ray branches, against the float64 restatement (joseph_ref.py).
test_forward_projection.py compares the kernel with the restatement on volumes of 30 voxels a side, 77 x 45 pixels and 21
projections with constant offsets; the configurations here reach what those do not:
  ref_shape          random 512^3 voxels of 1 mm, the reference's detector (1024 x 768 pixels of 0.388 mm, offset -159.856 mm), 894
                     angles from 90 degrees: 14 chunks of 64 projections (the last of 62: batches 16 + 16 + 16 + 14), tap positions
                     near 512 in float32, 500 float32 products per ray; compared on sampled rays (joseph_ref.project_rays) of the
                     projections on both sides of the batch and chunk boundaries, tile and detector edges included; twice, same bytes
  ref_shape_phantom  the same on the Catphan604 densities (the sharp edges of real input)
  chunks_<n>         n = 64, 65, 130 projections, each with its own angle, offset_x and offset_y (not monotone), 37 x 29 pixels
  central_plane_in   rays with D_y == 0 exactly (row nv / 2) and D_x == 0 exactly (column nu / 2 at 0 degrees) inside the slab
  central_plane_out  the same with the plane a quarter voxel outside the volume box but within reach of the bilinear taps
  source_inside      source and detector inside the volume: t0 and t1 stay at 0 and 1
  thin_<shape>       one or two planes along an axis, a single voxel: ns == fs
  deg45              exact 45, 135, 225, 315 degrees on isotropic voxels and an even detector (the central column ties the two
                     largest direction components), in a stack with other angles
  aniso_large_<fan>  300 x 97 x 260 voxels of (0.9, 2.5, 1.3) mm, off-centre origin, full-fan and half-fan, on sampled rays
the context's volume sources (u16 with the palette beyond the LDS stage, palette sizes 8192 and 8193, u8 at 512^3), and the refusals
of the C ABI.  Tolerance: test_forward_projection.py's, |got - ref| <= 1e-5 |ref| + 1e-5 max(spacing) outside the rays whose main
axis float32 and float64 may choose differently (joseph_ref.ambiguous_main_axis); rays the restatement gives 0 are exactly 0.
Parity against RTK itself is unpinned (RTK is absent here).

Measured on an MI355X, max err / tol: ref_shape 0.007, ref_shape_phantom 0.007, aniso_large 0.006 / 0.007, chunks 0.011,
central_plane 0.008 - 0.010, source_inside 0.008, thin 0.006 - 0.014, deg45 0.009 (0.33 % of its rays ambiguous, none elsewhere), u16
palette in global memory 0.010.  With tap positions and sums in float32, as joseph_ray.inc had them before these tests,
ref_shape_phantom stood at 4.138 (96 of 15,144 rays over the tolerance) and aniso_large_half at 0.764.  The table of what each
mutation of the kernel trips is in DESIGN.md, section 3."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import cases
import joseph_ref as jr
from test_forward_projection import _main_axis_face_rays

pkg = cases.pkg
fp = pkg.forward_projection
recon = pkg.reconstruction

SID, SDD = 1000.0, 1500.0
REF_DET, REF_PIX = (1024, 768), (0.388, 0.388)
REF_PROJECTIONS = (0, 15, 16, 63, 64, 65, 127, 128, 447, 700, 879, 880, 893)
PHANTOM_PROJECTIONS = (0, 16, 64, 333, 880, 893)
TILE_IU, TILE_IV = (0, 7, 8, 15, 16, 1023), (0, 15, 16, 767)
THIN_SHAPES = [(1, 9, 11), (9, 1, 11), (9, 11, 1), (2, 2, 2), (1, 1, 1)]  # [z][y][x]


def _geometry(angles, off_x=0.0, off_y=0.0):
    g = recon.CircularGeometry(SID, SDD)
    off_x, off_y = np.broadcast_to(off_x, (len(angles),)), np.broadcast_to(off_y, (len(angles),))
    for a, ox, oy in zip(angles, off_x, off_y):
        g.add_projection(float(a), float(ox), float(oy))
    return g


class Case:
    """One forward projection: volume [z][y][x] (float32), spacing and origin (x, y, z), geometry, detector, and the rays
    (p, iu, iv) on which the kernel is compared with the restatement (None = every ray)."""

    def __init__(self, name, vol, sp, org, geo, det, pix, rays=None):
        self.name, self.vol, self.sp, self.org, self.geo, self.det, self.pix, self.rays = name, vol, tuple(sp), tuple(org), geo, det, pix, rays

    def geometry_args(self):
        g = self.geo
        u0, v0 = fp.detector_origin(self.det, self.pix)
        return (np.asarray(g.gantry_angles), np.asarray(g.projection_offsets_x), np.asarray(g.projection_offsets_y), g.source_to_isocenter,
                g.source_to_detector), (self.pix[0], self.pix[1], u0, v0)

    def oracle(self):
        """(ref, ambiguous) on the compared rays: 1-D for a sample, [n][nv][nu] in full."""
        a, d = self.geometry_args()
        if self.rays is None:
            return (jr.project(self.vol, self.sp, self.org, *a, *self.det, *d),
                    jr.ambiguous_main_axis(*a, *self.det, *d, spacing=self.sp))
        return (jr.project_rays(self.vol, self.sp, self.org, *a, *d, *self.rays),
                jr.ambiguous_main_axis_rays(*a, *d, *self.rays, spacing=self.sp))

    def hip(self):
        return fp.project_forward(fp.RTKImage(self.vol, self.sp, self.org), self.geo, detector_size=self.det, detector_pixel_spacing=self.pix).array

    def pick(self, stack):
        return stack if self.rays is None else stack[self.rays[0], self.rays[2], self.rays[1]]


def _centred(shape_zyx, sp, shift=(0.0, 0.0, 0.0)):
    return tuple(-(n - 1) / 2 * s + d for n, s, d in zip(shape_zyx[::-1], sp, shift))


def _sample(projections, det, per_projection, seed, iu_edges=(), iv_edges=()):
    """(p, iu, iv): `per_projection` random pixels of each listed projection plus the grid iu_edges x iv_edges."""
    rng = np.random.default_rng(seed)
    eu, ev = (a.ravel() for a in np.meshgrid(np.asarray(iu_edges, int), np.asarray(iv_edges, int)))
    p, iu, iv = [], [], []
    for q in projections:
        iu.append(np.r_[rng.integers(0, det[0], per_projection), eu])
        iv.append(np.r_[rng.integers(0, det[1], per_projection), ev])
        p.append(np.full(iu[-1].size, q))
    return np.concatenate(p), np.concatenate(iu), np.concatenate(iv)


def _random(shape_zyx, seed):
    return np.random.default_rng(seed).random(shape_zyx, dtype=np.float32)


def _catphan512():
    g = pkg.workloads.workload_geometry("catphan", 512)
    return g, fp.prepare_image_for_rtk(g.densities, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)


def _chunk_geometry(n):
    """Every projection its own angle and offsets; none of the three sequences is monotone, and neighbours differ by millimetres."""
    k = np.arange(n)
    return _geometry((137.508 * k) % 360.0, 6.0 * np.sin(1.7 * k) - 3.0, 5.0 * np.cos(2.3 * k) + 1.0)


CENTRAL_ANGLES = (0.0, 90.0, 180.0, 270.0, 33.0, 141.5, 200.0, 307.0)


def _central_plane(name, index_y):
    """nv even, dv = 2, offset_y = 0: row nv / 2 has v = 0 exactly, so D_y == 0; nu even, du = 2, offset_x = 0: column nu / 2 has
    u = 0, so D_x == 0 at 0 degrees.  The plane y = 0 lies at index `index_y` of the volume."""
    shape, sp = (15, 10, 17), (2.5, 3.0, 2.0)
    org = list(_centred(shape, sp, (0.8, 0.0, -1.1)))
    org[1] = -index_y * sp[1]
    return Case(name, _random(shape, 11), sp, org, _geometry(CENTRAL_ANGLES), (36, 28), (2.0, 2.0))


def build_case(name):
    if name == "ref_shape":
        rays = _sample(REF_PROJECTIONS, REF_DET, 2500, 1, TILE_IU, TILE_IV)
        return Case(name, _random((512, 512, 512), 21), (1.0, 1.0, 1.0), _centred((512,) * 3, (1.0,) * 3), fp.create_geometry(894, start_angle=90.0),
                    REF_DET, REF_PIX, rays)
    if name == "ref_shape_phantom":
        img = _catphan512()[1]
        rays = _sample(PHANTOM_PROJECTIONS, REF_DET, 2500, 2, TILE_IU, TILE_IV)
        return Case(name, img.array, img.spacing, img.origin, fp.create_geometry(894, start_angle=90.0), REF_DET, REF_PIX, rays)
    if name.startswith("chunks_"):
        shape, sp = (13, 16, 19), (2.5, 2.0, 3.0)
        return Case(name, _random(shape, 3), sp, _centred(shape, sp, (1.0, -0.6, 0.4)), _chunk_geometry(int(name.split("_")[1])), (37, 29), (2.1, 2.3))
    if name == "central_plane_in":
        return _central_plane(name, 4.3)
    if name == "central_plane_out":   # a quarter voxel below the box: the taps of row 0 are in reach, the box is not
        return _central_plane(name, -0.75)
    if name == "central_plane_above":  # a quarter voxel above the box (ny = 10: the box ends at 9.5)
        return _central_plane(name, 9.75)
    if name == "source_inside":
        shape, sp = (30, 12, 30), (120.0, 20.0, 120.0)
        return Case(name, _random(shape, 5), sp, _centred(shape, sp, (17.0, 3.0, -29.0)), _geometry((0.0, 90.0, 180.0, 270.0, 45.0, 77.7, 213.0), -4.0, 2.0),
                    (36, 28), (1.5, 1.5))
    if name.startswith("thin_"):
        shape = tuple(int(v) for v in name.split("_")[1:])
        sp = (20.0, 16.0, 24.0)
        return Case(name, _random(shape, 6) + np.float32(0.5), sp, _centred(shape, sp, (1.5, -1.0, 2.0)),
                    _geometry((0.0, 90.0, 180.0, 270.0, 30.0, 45.0, 123.4, 237.0)), (36, 28), (1.5, 1.5))
    if name == "deg45":
        shape, sp = (20, 9, 20), (2.0, 2.0, 2.0)
        angles = (45.0, 135.0, 225.0, 315.0, 0.0, 90.0, 180.0, 270.0, 44.9, 45.1, 20.0, 70.0, 110.0, 160.0, 250.0, 340.0)
        return Case(name, _random(shape, 8), sp, _centred(shape, sp, (0.7, 0.3, -0.9)), _geometry(angles), (76, 44), (1.3, 1.7))
    if name.startswith("aniso_large_"):
        shape, sp = (260, 97, 300), (0.9, 2.5, 1.3)
        off = {"full": 0.0, "half": -159.856}[name.split("_")[2]]
        geo = _geometry(90.0 + 360.0 / 24 * np.arange(24) + 0.37, off, 1.25)
        rays = _sample(range(24), (256, 192), 1500, 9, (0, 15, 16, 255), (0, 15, 16, 191))
        return Case(name, _random(shape, 10), sp, (-120.5, -131.0, -190.25), geo, (256, 192), (1.552, 1.552), rays)
    raise KeyError(name)


@lru_cache(maxsize=None)
def case(name):
    """The small cases are kept for the session; the 512^3 ones are built by their test alone and let go with it."""
    assert not name.startswith("ref_shape")
    return build_case(name)


SMALL = ["chunks_64", "chunks_65", "chunks_130", "central_plane_in", "central_plane_out", "central_plane_above", "source_inside"] \
    + ["thin_%d_%d_%d" % s for s in THIN_SHAPES] + ["deg45"]
SAMPLED = ["aniso_large_full", "aniso_large_half"]


@lru_cache(maxsize=None)
def _oracle(name):
    return case(name).oracle()


def _check_conditions(name, ref, amb):
    """What a case must offer whatever the kernel gives: few ambiguous rays, enough rays through the volume."""
    assert amb.mean() < 0.01, (name, float(amb.mean()))
    assert (ref > 0).mean() > 0.1, (name, float((ref > 0).mean()))
    assert np.isfinite(ref).all()


def _compare(c, got_stack, ref, amb):
    name = c.name
    _check_conditions(name, ref, amb)
    got = c.pick(got_stack).astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    tol = 1e-5 * np.abs(ref) + 1e-5 * max(c.sp)
    ratio = float((err / tol)[~amb].max())
    print(f"{name}: max err / tol = {ratio:.3f} on {int((~amb).sum())} rays, ambiguous share {amb.mean():.5f}, hit share {(ref > 0).mean():.3f}")
    assert ratio <= 1.0, (name, ratio, int(((err > tol) & ~amb).sum()))
    assert np.all(got[ref == 0] == 0.0), name  # rays that miss give exactly 0
    return ratio


# ---------------------------------------------------------------------------------------------------------------- CPU: the oracle
def test_project_rays_equals_the_entries_of_project():
    """A small anisotropic, offset case with misses: the listed rays of the stack bit for bit (unsorted, repeated), and the subset
    form of the ambiguity mask likewise (rel widened until the mask is not empty)."""
    rng = np.random.default_rng(4)
    shape, sp = (11, 15, 9), (4.0, 3.0, 2.0)
    vol = rng.random(shape)
    org = _centred(shape, sp, (2.0, -1.0, 0.5))
    k = np.arange(9)
    geo = _geometry(12.5 + 40.0 * k, 35.0 + 4.0 * np.sin(k), -20.0 + 3.0 * np.cos(k))
    c = Case("pin", vol, sp, org, geo, (61, 39), (2.9, 2.3))
    a, d = c.geometry_args()
    full = jr.project(vol, sp, org, *a, *c.det, *d)
    assert (full == 0).mean() > 0.05 and (full > 0).mean() > 0.1
    p, iu, iv = rng.integers(0, 9, 4000), rng.integers(0, 61, 4000), rng.integers(0, 39, 4000)
    p[:3], iu[:3], iv[:3] = p[3:6], iu[3:6], iv[3:6]
    sub = jr.project_rays(vol, sp, org, *a, *d, p, iu, iv)
    np.testing.assert_array_equal(sub, full[p, iv, iu])
    assert (sub == 0).any()
    np.testing.assert_array_equal(jr.project_rays(vol.astype(np.float32), sp, org, *a, *d, p, iu, iv),
                                  jr.project(vol.astype(np.float32), sp, org, *a, *c.det, *d)[p, iv, iu])  # a float32 volume, converted in the gather
    amb = jr.ambiguous_main_axis(*a, *c.det, *d, spacing=sp, rel=0.3)
    assert 0 < amb.sum() < amb.size
    np.testing.assert_array_equal(jr.ambiguous_main_axis_rays(*a, *d, p, iu, iv, spacing=sp, rel=0.3), amb[p, iv, iu])


def _constant(c, value):
    return Case(c.name, np.full(c.vol.shape, value), c.sp, c.org, c.geo, c.det, c.pix)


def _rays_of(c, i):
    """Source, pixel positions and index-space direction of projection i of a case, detector order."""
    a, (du, dv, u0, v0) = c.geometry_args()
    uu, vv = np.meshgrid(u0 + du * np.arange(c.det[0]), v0 + dv * np.arange(c.det[1]))
    S, P = jr.ray_endpoints(a[0][i], a[1][i], a[2][i], a[3], a[4], uu.ravel(), vv.ravel())
    return S, P


def test_oracle_central_plane_rays():
    """Row nv / 2 has D_y == 0 exactly (and column nu / 2 at 0 degrees D_x == 0): inside the slab value x chord of a constant box
    to 1e-12 on the rays through the two main-axis faces, with the plane outside the box exactly 0, never NaN."""
    value = 0.37
    for name in ("central_plane_in", "central_plane_out", "central_plane_above"):
        c = _constant(case(name), value)
        ref, _ = c.oracle()
        assert np.isfinite(ref).all()
        nu, nv = c.det
        N, sp, org = np.array(c.vol.shape[::-1]), np.array(c.sp), np.array(c.org)
        seen = 0
        for i, angle in enumerate(CENTRAL_ANGLES):
            S, P = _rays_of(c, i)
            D = (P - S).reshape(nv, nu, 3)
            assert np.all(D[nv // 2, :, 1] == 0.0) and np.all(D[nv // 2 - 1, :, 1] != 0.0)
            if angle == 0.0:
                assert np.all(D[:, nu // 2, 0] == 0.0)
            row = ref[i, nv // 2]
            if name == "central_plane_in":
                chord, ok = _main_axis_face_rays(N, sp, org, S, P)
                chord, ok = chord.reshape(nv, nu)[nv // 2], ok.reshape(nv, nu)[nv // 2]
                seen += int(ok.sum())
                np.testing.assert_allclose(row[ok], value * chord[ok], rtol=1e-12)
            else:
                assert np.all(row == 0.0)
                assert (ref[i] > 0).any()  # other rows of the same projection do cross the box
        assert name != "central_plane_in" or seen > 100


def test_oracle_source_and_detector_inside_a_constant_volume():
    """Nothing is clipped: every ray gives value x |pixel - source| to 1e-12."""
    value = 0.61
    c = _constant(case("source_inside"), value)
    ref, _ = c.oracle()
    N, sp, org = np.array(c.vol.shape[::-1]), np.array(c.sp), np.array(c.org)
    for i in range(len(c.geo.gantry_angles)):
        S, P = _rays_of(c, i)
        for X in (S[None, :], P):  # both ends a voxel or more inside the outer voxel centres
            idx = (X - org) / sp
            assert np.all(idx >= 1.0) and np.all(idx <= N - 2.0)
        np.testing.assert_allclose(ref[i].ravel(), value * np.linalg.norm(P - S, axis=1), rtol=1e-12)


@pytest.mark.parametrize("shape", THIN_SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_oracle_thin_volumes(shape):
    """One or two planes along an axis and a single voxel, constant: finite, no NaN, and on rays through the two main-axis faces
      - a voxel or more from the side faces (_main_axis_face_rays; needs side axes of three voxels or more): value x chord;
      - with one plane along the main axis (ns == fs, one sample of weight hi - lo = 1): value x chord x w(A) w(B), where A, B are
        the side coordinates of the sample and w the share of the two bilinear taps that lie inside, min(A + 1, N - A) cut to 0..1
        (taps beside the volume read 0, so a single voxel gives the whole chord only on its centre line);
    every ray gives at most value x one step per plane, and 0 where the segment misses the box."""
    value = 0.83
    c = _constant(case("thin_%d_%d_%d" % shape), value)
    ref, _ = c.oracle()
    assert np.isfinite(ref).all() and (ref >= 0).all() and (ref > 0).mean() > 0.1
    N, sp, org = np.array(shape[::-1]), np.array(c.sp), np.array(c.org)
    exact = single = 0
    for i in range(len(c.geo.gantry_angles)):
        S, P = _rays_of(c, i)
        got, dlen = ref[i].ravel(), np.linalg.norm(P - S, axis=1)
        chord, ok = _main_axis_face_rays(N, sp, org, S, P)
        exact += int(ok.sum())
        np.testing.assert_allclose(got[ok], value * chord[ok], rtol=1e-12)
        Si, Di = (S - org) / sp, (P - S) / sp
        r = np.arange(len(Di))
        m = np.argmax(np.abs(Di), axis=1)
        Dm = Di[r, m]
        assert np.all(got <= value * dlen / np.abs(Dm) * N[m] * (1 + 1e-12))
        ta, tb, tc = (-0.5 - Si[m]) / Dm, (N[m] - 0.5 - Si[m]) / Dm, -Si[m] / Dm
        one = (N[m] == 1) & (np.minimum(ta, tb) > 0) & (np.maximum(ta, tb) < 1)
        w = np.ones(len(Di))
        for a in range(3):
            for t in (ta, tb):  # both faces crossed inside the box
                x = Si[a] + t * Di[:, a]
                one &= (m == a) | ((x > -0.5) & (x < N[a] - 0.5))
            x = Si[a] + tc * Di[:, a]
            w *= np.where(m == a, 1.0, np.clip(np.minimum(x + 1, N[a] - x), 0, 1))
        single += int(one.sum())
        np.testing.assert_allclose(got[one], (value * np.abs(tb - ta) * dlen * w)[one], rtol=1e-12)
        with np.errstate(divide="ignore", invalid="ignore"):
            fa, fb = (-0.5 - Si) / Di, (N - 0.5 - Si) / Di
        t0 = np.clip(np.nanmax(np.minimum(fa, fb), axis=1), 0, 1)
        t1 = np.clip(np.nanmin(np.maximum(fa, fb), axis=1), 0, 1)
        assert np.all(got[t1 < t0] == 0.0)
    assert exact > 50 or shape[1] < 3  # ny < 3: y is a side axis of every ray of a circular orbit, so none is a voxel from its faces
    assert single > 50 or 1 not in (shape[0], shape[2])  # one plane along z or x: the main axis of some of the angles


@pytest.mark.parametrize("name", SMALL + SAMPLED)
def test_cases_meet_their_conditions(name):
    """Decided by the restatement alone: less than 1 % of the rays ambiguous, more than 10 % through the volume."""
    ref, amb = _oracle(name)
    _check_conditions(name, ref, amb)
    c = case(name)
    if name.startswith("chunks_"):
        g = c.geo
        for seq in (g.gantry_angles, g.projection_offsets_x, g.projection_offsets_y):
            d = np.diff(np.asarray(seq))
            assert (d > 0).any() and (d < 0).any() and np.abs(d[:16]).min() > 0.05
        assert c.det[0] % 16 and c.det[1] % 16
    if name == "central_plane_out":
        assert (ref[:, c.det[1] // 2] == 0).all()
    if name == "source_inside":
        assert (ref > 0).all()
    if name == "deg45":
        assert _oracle(name)[1][:4].mean() > 0.01 and {45.0, 135.0, 0.0, 90.0, 180.0, 270.0} <= set(c.geo.gantry_angles)


def test_reference_samples_reach_the_chunk_and_tile_edges():
    """ref_shape's sample by construction (no volume is built): the projections on both sides of the batch (16) and chunk (64)
    boundaries, the last chunk of 62 with its batch of 14, and the corners of tiles and of the detector."""
    for projections in (REF_PROJECTIONS, PHANTOM_PROJECTIONS):
        p, iu, iv = _sample(projections, REF_DET, 2500, 1, TILE_IU, TILE_IV)
        assert set(p) == set(projections) and p.size == len(projections) * (2500 + 24)
        for q in projections:
            pairs = set(zip(iu[p == q], iv[p == q]))
            assert {(a, b) for a in TILE_IU for b in TILE_IV} <= pairs
        assert iu.max() == 1023 and iv.max() == 767 and iu.min() == 0 and iv.min() == 0
    assert {0, 15, 16, 63, 64, 65, 127, 128, 879, 880, 893} <= set(REF_PROJECTIONS)
    assert 894 % 64 == 62 and 62 % 16 == 14 and 880 == 13 * 64 + 48 and 893 - 880 == 13
    geo = fp.create_geometry(894, start_angle=90.0)
    assert geo.gantry_angles[0] == 90.0 and set(geo.projection_offsets_x) == {-159.856}


# ---------------------------------------------------------------------------------------------------------------- GPU: kernel against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL + SAMPLED)
def test_configuration(engine, name):
    c = case(name)
    got = c.hip()
    assert got.shape == (len(c.geo.gantry_angles), c.det[1], c.det[0])
    _compare(c, got, *_oracle(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ref_shape", "ref_shape_phantom"])
def test_ref_shape(engine, name):
    """The full stack of the reference's shape (2.8 GB on the host), twice: the same bytes, and the sampled rays within tolerance."""
    c = build_case(name)
    got = c.hip()
    assert got.shape == (894, 768, 1024)
    _compare(c, got, *c.oracle())
    again = c.hip()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- GPU: the context's volume sources
def _context(engine, tmp_path, g):
    ctx = engine.create(cases.build_case("water", tmp_path / "ctx"), device=0)
    ctx.set_geometry(g)
    return ctx


def _levels(n_levels):
    """One material with exactly `n_levels` distinct float32 densities, every one of them present: that many palette entries."""
    shape = (48, 44, 42)
    g = cases.geometry.MCBoxGeometry(shape=shape, image_spacing=(6.0, 5.0, 4.0), material="h2o")
    levels = np.round(np.linspace(0.2, 1.9, n_levels), 6).astype(np.float32)
    assert np.unique(levels).size == n_levels
    g.densities[:] = levels[np.random.default_rng(n_levels).permutation(int(np.prod(shape))) % n_levels].reshape(shape)
    return g


CTX_ANGLES = [3.0, 47.0, 90.0, 181.5, 300.0, 359.0, 12.0]
CTX_DET, CTX_PIX = (96, 64), (3.1, 3.1)


def _context_and_host(engine, tmp_path, g, angles, det, pix):
    """(stack from the context's resident volume, stack of the host path on the same densities, image, geometry, volume kind,
    palette size)."""
    spacing, origin = fp.rtk_frame(g.image_shape, g.image_spacing)
    with _context(engine, tmp_path, g) as ctx:
        kind, n_pal = ctx.geti("volume_kind"), ctx.geti("palette_size")
        got, _ = ctx.project_forward(angles, detector_size=det, detector_pixel_spacing=pix, spacing_iec=spacing, origin_iec=origin)
    geo = recon.create_geometry(0)
    for a in angles:
        geo.add_projection(a, pkg.defaults.DEFAULTS.detector_lateral_displacement, 0.0)
    img = fp.prepare_image_for_rtk(g.densities, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
    want = fp.project_forward(img, geo, detector_size=det, detector_pixel_spacing=pix).array
    return got, want, img, geo, kind, n_pal


@pytest.mark.gpu
def test_u16_volume_with_the_palette_in_global_memory(engine, tmp_path):
    """About 20,000 (material, density) pairs: u16 indices whose palette does not fit the 8192-entry LDS stage (SrcU16<false>, the
    densities read from the float2 palette).  Against the restatement on the float32 densities, and the host path bit for bit."""
    g = cases._graded(20000)()
    g.image_spacing = (6.0, 5.0, 4.0)
    got, want, img, geo, kind, n_pal = _context_and_host(engine, tmp_path, g, CTX_ANGLES, CTX_DET, CTX_PIX)
    assert kind == 1 and n_pal > 8192
    c = Case("u16_global_palette", img.array, img.spacing, img.origin, geo, CTX_DET, CTX_PIX)
    ref, amb = c.oracle()
    _check_conditions(c.name, ref, amb)
    err, tol = np.abs(got - ref), 1e-5 * np.abs(ref) + 1e-5 * max(c.sp)
    ratio = float((err / tol)[~amb].max())
    print(f"{c.name}: palette {n_pal}, max err / tol = {ratio:.3f}, ambiguous share {amb.mean():.5f}")
    assert ratio <= 1.0, ratio
    assert np.all(got[ref == 0] == 0.0)
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n_levels", [8192, 8193])
def test_palette_at_the_lds_boundary(engine, tmp_path, n_levels):
    """The largest palette that is staged in LDS and the smallest that is not: both the host path bit for bit."""
    g = _levels(n_levels)
    got, want, _, _, kind, n_pal = _context_and_host(engine, tmp_path, g, CTX_ANGLES, CTX_DET, CTX_PIX)
    assert kind == 1 and n_pal == n_levels
    assert (want > 0).mean() > 0.2
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_u8_volume_at_full_size(engine, tmp_path):
    """The Catphan604 geometry of 512^3 voxels resident in a context (tiled u8), the reference's detector, 20 angles (a batch of 16
    and one of 4): the host path bit for bit."""
    g = pkg.workloads.workload_geometry("catphan", 512)
    angles = list(90.0 + 17.3 * np.arange(20))
    got, want, _, _, kind, _ = _context_and_host(engine, tmp_path, g, angles, REF_DET, REF_PIX)
    assert kind == 0 and got.shape == (20, 768, 1024)
    assert (want > 0).mean() > 0.2
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- the C ABI's refusals
class _Call:
    """mcgpu_forward_project / mcgpu_forward_project_context through ctypes on a small valid problem; keyword arguments replace
    fields of mcgpu_fp_options, `volume` / `output` the two buffers (None = a null pointer)."""
    KEEP = object()

    def __init__(self):
        self.lib = pkg.engine.load_library()
        self.lib.mcgpu_forward_project.argtypes = [C.POINTER(fp._FpOptions), C.c_void_p, C.c_void_p, C.POINTER(fp._FpReport)]
        self.lib.mcgpu_forward_project_context.argtypes = [C.c_void_p, C.POINTER(fp._FpOptions), C.c_void_p, C.POINTER(fp._FpReport)]
        self.lib.mcgpu_forward_project.restype = self.lib.mcgpu_forward_project_context.restype = C.c_int
        self.vol = _random((7, 6, 9), 12)
        self.angles = np.array([10.0, 100.0, 250.0])
        self.off = np.array([-5.0, 2.0, 0.0]), np.array([1.0, -1.0, 0.5])
        self.nu, self.nv = 21, 13

    def options(self, struct_size=None, **fields):
        dp = C.POINTER(C.c_double)
        u0, v0 = fp.detector_origin((self.nu, self.nv), (4.0, 4.0))
        o = fp._FpOptions(C.sizeof(fp._FpOptions) if struct_size is None else struct_size, 3, self.nu, self.nv, 4.0, 4.0, u0, v0, SID, SDD,
                          self.angles.ctypes.data_as(dp), self.off[0].ctypes.data_as(dp), self.off[1].ctypes.data_as(dp), 9, 6, 7, 5.0, 6.0, 7.0,
                          *(float("nan"),) * 3, 0)
        for k, v in fields.items():
            setattr(o, k, v)
        return o

    def host(self, o, volume=KEEP, output=KEEP):
        out = np.full((3, self.nv, self.nu), -1.0, np.float32)
        rc = self.lib.mcgpu_forward_project(C.byref(o), self.vol.ctypes.data if volume is self.KEEP else volume,
                                            out.ctypes.data if output is self.KEEP else output, C.byref(fp._FpReport()))
        return rc, out, self.lib.mcgpu_last_error().decode(errors="replace")

    def context(self, ctx, o, output=KEEP):
        n = max(o.n_proj, 1) * max(o.nv, 1) * max(o.nu, 1)
        out = np.full(n, -1.0, np.float32)
        rc = self.lib.mcgpu_forward_project_context(ctx.h if ctx is not None else None, C.byref(o), out.ctypes.data if output is self.KEEP else output,
                                                    C.byref(fp._FpReport()))
        return rc, out, self.lib.mcgpu_last_error().decode(errors="replace")


def test_abi_refuses_a_zero_struct_size(engine, case_dir):
    """struct_size = 0 (a caller that did not set it): -1 and a message that names the field, on both entry points, before
    anything is read or launched."""
    call = _Call()
    rc, out, msg = call.host(call.options(struct_size=0))
    assert rc == -1 and "struct_size" in msg and "mcgpu_forward_project:" in msg and np.all(out == -1.0)
    with engine.create(case_dir("water"), device=-1) as ctx:
        rc, out, msg = call.context(ctx, call.options(struct_size=0))
    assert rc == -1 and "struct_size" in msg and "mcgpu_forward_project_context" in msg and np.all(out == -1.0)


@pytest.mark.parametrize("field, value", [("n_proj", 0), ("nu", 0), ("nv", 0), ("du", 0.0), ("dv", -1.0), ("sid", 0.0), ("sdd", float("nan")),
                                          ("gantry_deg", None)])
def test_abi_refuses_bad_arguments(engine, case_dir, field, value):
    call = _Call()
    o = call.options()
    setattr(o, field, C.POINTER(C.c_double)() if value is None else value)
    rc, out, msg = call.host(o)
    assert rc == -1 and msg.endswith("mcgpu_forward_project: bad argument") and np.all(out == -1.0)
    with engine.create(case_dir("water"), device=-1) as ctx:
        rc, out, msg = call.context(ctx, o)
    assert rc == -1 and msg.endswith("mcgpu_forward_project_context: bad argument")


@pytest.mark.parametrize("what", ["nx", "ny", "nz", "sx", "sy", "sz", "volume", "output"])
def test_abi_refuses_bad_volume_arguments(engine, what):
    call = _Call()
    o = call.options()
    if what in ("volume", "output"):
        rc, out, msg = call.host(o, **{what: None})
    else:
        setattr(o, what, 0)
        rc, out, msg = call.host(o)
    assert rc == -1 and msg.endswith("mcgpu_forward_project: bad volume argument") and np.all(out == -1.0)


def test_abi_refuses_a_context_without_a_device(engine, case_dir):
    call = _Call()
    with engine.create(case_dir("water"), device=-1) as ctx:
        rc, out, msg = call.context(ctx, call.options(nx=0, ny=0, nz=0))
        assert rc == -1 and "the context needs a device" in msg and np.all(out == -1.0)
    rc, _, msg = call.context(None, call.options(nx=0, ny=0, nz=0))
    assert rc == -1 and "bad argument" in msg


@pytest.mark.gpu
def test_abi_old_header_reads_device_as_zero(engine):
    """A caller built against a header that ends before `device` passes a shorter struct: what lies beyond reads as 0, so the
    stack is bit for bit the one of the full struct with device = 0 -- whatever the memory behind the short struct holds."""
    call = _Call()
    full = C.sizeof(fp._FpOptions)
    cut = fp._FpOptions.device.offset
    assert cut < full <= cut + 8
    rc0, want, _ = call.host(call.options(device=0))
    assert rc0 == 0 and np.isfinite(want).all() and (want > 0).mean() > 0.1
    rc1, got, msg = call.host(call.options(struct_size=cut, device=12345))
    assert rc1 == 0, msg
    assert got.tobytes() == want.tobytes()
    img = fp.RTKImage(call.vol, (5.0, 6.0, 7.0), _centred(call.vol.shape, (5.0, 6.0, 7.0)))
    geo = _geometry(call.angles, *call.off)
    assert fp.project_forward(img, geo, detector_size=(call.nu, call.nv), detector_pixel_spacing=(4.0, 4.0)).array.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_abi_context_refuses_another_volume_size(engine, tmp_path):
    """A caller that states a volume size states the context's IEC size, or is told both."""
    call = _Call()
    g = cases.geometry.MCBoxGeometry(shape=(23, 18, 13), image_spacing=(7.0, 7.0, 7.0), material="h2o")  # IEC (X, Y, Z) = (23, 13, 18)
    with _context(engine, tmp_path, g) as ctx:
        rc, out, msg = call.context(ctx, call.options(nx=23, ny=18, nz=13))
        assert rc == -1 and "23x18x13" in msg and "23x13x18" in msg and np.all(out == -1.0)
        rc, out, msg = call.context(ctx, call.options(nx=23, ny=13, nz=18, sx=0.0, sy=0.0, sz=0.0))
        assert rc == 0, msg
        assert np.isfinite(out).all() and (out > 0).mean() > 0.1


def _tiny_call(device):
    """mcgpu_forward_project on the smallest valid problem: one projection of 2 x 2 pixels through one voxel of 5 mm."""
    call = _Call()
    angle, vol, out = np.array([30.0]), np.ones((1, 1, 1), np.float32), np.full((1, 2, 2), -1.0, np.float32)
    o = fp._FpOptions(C.sizeof(fp._FpOptions), 1, 2, 2, 4.0, 4.0, -2.0, -2.0, SID, SDD, angle.ctypes.data_as(C.POINTER(C.c_double)), None, None,
                      1, 1, 1, 5.0, 5.0, 5.0, *(float("nan"),) * 3, device)
    rc = call.lib.mcgpu_forward_project(C.byref(o), vol.ctypes.data, out.ctypes.data, None)
    return rc, out, call.lib.mcgpu_last_error().decode(errors="replace")


def test_abi_a_device_that_does_not_exist_is_an_error_return(engine):
    """Device 9999: the runtime's refusal comes back as -1 with the failing call in the message (no GPU is needed to be refused)."""
    rc, out, msg = _tiny_call(9999)
    assert rc == -1 and "!!HIP ERROR!! hipSetDevice" in msg and np.all(out == -1.0)


@pytest.mark.gpu
def test_abi_a_valid_call_follows_a_refused_device(engine):
    assert _tiny_call(9999)[0] == -1
    rc, out, msg = _tiny_call(0)
    assert rc == 0, msg
    assert np.isfinite(out).all() and (out > 0).all()  # every ray of the 2 x 2 detector passes through the voxel
