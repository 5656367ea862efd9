"""Joseph forward projection (csrc/forward_project.hip, 4d-cbct-mc_amd/forward_projection.py; the reference's
cbctmc/forward_projection.py on RTK's JosephForwardProjectionImageFilter).
CPU: the float64 restatement (joseph_ref.py) against analytic chords, the ray geometry against CircularGeometry.matrix, the IEC
transform and origin rule of prepare_image_for_rtk, the header of the stacks.
GPU: the HIP kernel against the restatement, the context's volume representations against the host path, FP -> FDK, the
alignment of Monte Carlo projections with the density FP, and density_fp_4d.mha of a 4-D scan.
Parity against RTK itself is unpinned (RTK is absent here)."""
import numpy as np
import pytest

import cases
import joseph_ref as jr
import warp_ref

pkg = cases.pkg
fp = pkg.forward_projection
recon = pkg.reconstruction


# ---------------------------------------------------------------------------------------------------------------- CPU
def _main_axis_face_rays(N, sp, org, S, P):
    """Per ray: (chord length in mm between the two faces of the main axis, True where the ray crosses both of those faces at
    least one voxel away from every side face)."""
    Si, Di = (S - org) / sp, (P - S) / sp
    m = np.argmax(np.abs(Di), axis=1)
    r = np.arange(len(m))
    ta, tb = (-0.5 - Si[m]) / Di[r, m], (N[m] - 0.5 - Si[m]) / Di[r, m]
    ok = np.ones(len(m), bool)
    for t in (ta, tb):
        X = Si + t[:, None] * Di
        for a in range(3):
            ok &= (m == a) | ((X[:, a] >= 0.5) & (X[:, a] <= N[a] - 1.5))
    ok &= (np.minimum(ta, tb) > 0) & (np.maximum(ta, tb) < 1)
    return np.abs(tb - ta) * np.linalg.norm(P - S, axis=1), ok


@pytest.mark.parametrize("angle, spacing", [(0.0, (2.0, 2.0, 2.0)), (90.0, (1.5, 2.5, 2.0)), (33.0, (2.0, 3.0, 1.0)), (240.0, (2.0, 2.0, 4.0))])
def test_oracle_constant_box_gives_value_times_chord(angle, spacing):
    """Rays that enter and leave through the faces of their main axis, a voxel or more from the side faces: value x chord to 1e-12.
    This pins the length of a step and the weights of the partial first and last steps."""
    shape_zyx, value = (14, 12, 18), 0.37
    vol = np.full(shape_zyx, value)
    N, sp = np.array(shape_zyx[::-1]), np.array(spacing)
    org = -(N - 1) / 2 * sp + np.array([1.3, -0.7, 2.1])
    sid, sdd, nu, nv, du, dv = 400.0, 700.0, 60, 50, 1.7, 1.9
    u0, v0 = -0.5 * nu * du + 0.3, -0.5 * nv * dv
    got = jr.project(vol, sp, org, [angle], [5.0], [-3.0], sid, sdd, nu, nv, du, dv, u0, v0)[0].ravel()
    uu, vv = np.meshgrid(u0 + du * np.arange(nu), v0 + dv * np.arange(nv))
    S, P = jr.ray_endpoints(angle, 5.0, -3.0, sid, sdd, uu.ravel(), vv.ravel())
    chord, ok = _main_axis_face_rays(N, sp, org, S, P)
    assert ok.sum() > 200
    np.testing.assert_allclose(got[ok], value * chord[ok], rtol=1e-12)


def test_oracle_voxelised_sphere_gives_its_chords_within_a_voxel():
    """Rays well inside the sphere (they would still hit it two voxels smaller) give its chord within one voxel diagonal; every ray
    lies between the chords of the spheres one voxel smaller and one voxel larger (to 0.05 voxel: the bilinear taps at the
    surface reach a little further)."""
    n, s, radius, c = 40, 1.0, 12.3, np.array([1.7, -2.2, 0.9])
    X = -(n - 1) / 2 * s + s * np.arange(n)
    zz, yy, xx = np.meshgrid(X, X, X, indexing="ij")
    vol = (((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) <= radius ** 2).astype(float)
    sid, sdd, nu, nv, du, dv = 300.0, 500.0, 48, 48, 1.1, 1.1
    u0, v0 = -0.5 * nu * du, -0.5 * nv * dv
    for angle in (0.0, 27.0, 45.5, 130.0):
        got = jr.project(vol, (s, s, s), (X[0],) * 3, [angle], [0.0], [0.0], sid, sdd, nu, nv, du, dv, u0, v0)[0].ravel()
        uu, vv = np.meshgrid(u0 + du * np.arange(nu), v0 + dv * np.arange(nv))
        S, P = jr.ray_endpoints(angle, 0.0, 0.0, sid, sdd, uu.ravel(), vv.ravel())
        d = (P - S) / np.linalg.norm(P - S, axis=1)[:, None]
        w = S - c
        b = (d * w).sum(axis=1)
        chord = lambda r: 2 * np.sqrt(np.clip(b ** 2 - ((w * w).sum() - r ** 2), 0, None))
        inner = chord(radius - 2 * s) > 0
        assert inner.sum() > 500
        assert np.abs(got - chord(radius))[inner].max() <= np.sqrt(3) * s, angle
        assert np.abs(got - chord(radius))[inner].mean() < 0.5 * s, angle
        assert (got >= chord(radius - s) - 0.05 * s).all() and (got <= chord(radius + s) + 0.05 * s).all(), angle


@pytest.mark.parametrize("start_angle, offset", [(90.0, 0.0), (270.0, 0.0), (90.0, -159.856), (270.0, -159.856)])
def test_pixel_positions_project_to_their_own_uv(start_angle, offset):
    geo = recon.create_geometry(7, start_angle=start_angle, detector_offset_x=offset, detector_offset_y=2.5)
    nu, nv, du, dv = 64, 48, 0.388 * 16, 0.388 * 16
    u0, v0 = fp.detector_origin((nu, nv), (du, dv))
    uu, vv = np.meshgrid(u0 + du * np.arange(nu), v0 + dv * np.arange(nv))
    for i, a in enumerate(geo.gantry_angles):
        S, P = jr.ray_endpoints(a, geo.projection_offsets_x[i], geo.projection_offsets_y[i], geo.source_to_isocenter, geo.source_to_detector,
                                uu.ravel(), vv.ravel())
        h = geo.matrix(i) @ np.vstack([P.T, np.ones(len(P))])
        np.testing.assert_allclose(h[0] / h[2], uu.ravel(), atol=1e-9)
        np.testing.assert_allclose(h[1] / h[2], vv.ravel(), atol=1e-9)
        hs = geo.matrix(i) @ np.append(S, 1.0)  # the source projects to infinity
        assert abs(hs[2]) < 1e-9


def test_prepare_image_for_rtk_iec_mapping_and_origin_rule():
    rng = np.random.default_rng(3)
    n0, n1, n2 = 5, 4, 3  # MC (x, y, z)
    img = rng.random((n0, n1, n2)).astype(np.float32)
    out = fp.prepare_image_for_rtk(img, image_spacing=(1.0, 2.0, 3.0), input_value_range=None, output_value_range=None)
    assert out.array.shape == (n1, n2, n0)  # ITK [Z][Y][X]: IEC X = MC x, Y = -MC z, Z = -MC y
    for iz in range(n1):
        for iy in range(n2):
            for ix in range(n0):
                assert out.array[iz, iy, ix] == img[ix, n1 - 1 - iz, n2 - 1 - iy]
    assert out.spacing == (1.0, 3.0, 2.0)
    # the reference's origin rule: (-NX SX/2 + SY/2, -NY SZ/2 + SZ/2, -NZ SY/2 + SX/2), ITK size (5, 3, 4), spacing (1, 3, 2)
    assert out.origin == pytest.approx((-2.5 + 1.5, -3.0 + 1.0, -6.0 + 0.5), abs=1e-12)
    iso = fp.prepare_image_for_rtk(img, image_spacing=(2.0, 2.0, 2.0), input_value_range=None, output_value_range=None)
    assert iso.origin == pytest.approx(tuple(-(n - 1) / 2 * 2.0 for n in (n0, n2, n1)), abs=1e-12)  # centred
    off = fp.prepare_image_for_rtk(img, image_spacing=(2.0, 2.0, 2.0), input_value_range=None, output_value_range=None,
                                   origin_offset=(1.0, -2.0, 0.5))
    assert off.origin == pytest.approx(tuple(o + d for o, d in zip(iso.origin, (1.0, -2.0, 0.5))), abs=1e-12)
    assert fp.rtk_frame((n0, n1, n2), (1.0, 2.0, 3.0)) == (out.spacing, out.origin)


def test_prepare_image_for_rtk_rescales_and_clips():
    img = np.array([-2000.0, -1024.0, 1023.5, 3071.0, 5000.0], np.float32).reshape(5, 1, 1)
    out = fp.prepare_image_for_rtk(img, image_spacing=(1.0, 1.0, 1.0))
    np.testing.assert_allclose(out.array.ravel(), [0.0, 0.0, 0.5, 1.0, 1.0], atol=1e-7)
    raw = fp.prepare_image_for_rtk(img, image_spacing=(1.0, 1.0, 1.0), input_value_range=None)
    np.testing.assert_array_equal(raw.array.ravel(), img.ravel())


def test_forward_projection_module_surface():
    assert fp.create_geometry is recon.create_geometry and fp.save_geometry is recon.save_geometry


def test_density_fp_stack_header(engine, tmp_path):
    """density_fp(_4d).mha carry the reference's stack metadata: spacing (du, dv, 1), origin (-nu du / 2, -nv dv / 2, 0)."""
    spacing, origin = fp.stack_metadata()
    assert spacing == (0.388, 0.388, 1.0) and origin == pytest.approx((-0.5 * 1024 * 0.388, -0.5 * 768 * 0.388, 0.0))
    w = engine.StackWriter(tmp_path / "density_fp.mha", 16, 8, 3, spacing[:2])
    for k in range(3):
        w.append(np.full((8, 16), k, np.float32))
    w.finish(replace_zeros=False)
    arr, sp, org = recon.read_mha(tmp_path / "density_fp.mha")
    assert arr.shape == (3, 8, 16) and arr[0].max() == 0.0
    assert sp == pytest.approx([0.388, 0.388, 1.0]) and org == pytest.approx([-0.5 * 16 * 0.388, -0.5 * 8 * 0.388, 0.0])
    assert fp.detector_origin((16, 8), (0.388, 0.388)) == pytest.approx(tuple(org[:2]))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _compare(vol_zyx, sp, org, geo, det, pix):
    """HIP kernel (host path) against the float64 restatement."""
    img = fp.RTKImage(np.ascontiguousarray(vol_zyx, np.float32), tuple(sp), tuple(org))
    got = fp.project_forward(img, geo, detector_size=det, detector_pixel_spacing=pix).array
    u0, v0 = fp.detector_origin(det, pix)
    args = (geo.gantry_angles, geo.projection_offsets_x, geo.projection_offsets_y, geo.source_to_isocenter, geo.source_to_detector,
            det[0], det[1], pix[0], pix[1], u0, v0)
    ref = jr.project(img.array.astype(np.float64), sp, org, *args)
    amb = jr.ambiguous_main_axis(*args, spacing=sp)
    return got, ref, amb


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["centred", "half_fan_anisotropic", "near_45", "offsets_and_misses"])
def test_hip_matches_the_oracle(engine, case):
    rng = np.random.default_rng(7)
    if case == "centred":
        shape, sp, n_proj, start, off = (17, 21, 19), (2.0, 2.0, 2.0), 5, 0.0, (0.0, 0.0)
    elif case == "half_fan_anisotropic":
        shape, sp, n_proj, start, off = (13, 23, 30), (3.0, 1.5, 2.5), 21, 90.0, (-40.0, 0.0)  # half-fan proportions of a small detector
    elif case == "near_45":
        shape, sp, n_proj, start, off = (20, 9, 20), (2.0, 2.0, 2.0), 3, 44.7, (0.0, 0.0)
    else:
        shape, sp, n_proj, start, off = (11, 15, 9), (4.0, 3.0, 2.0), 17, 12.5, (35.0, -20.0)
    vol = rng.random(shape)  # [z][y][x]
    N = np.array(shape[::-1])
    org = -(N - 1) / 2 * np.array(sp) + rng.uniform(-3, 3, 3)
    geo = recon.create_geometry(n_proj, start_angle=start, detector_offset_x=off[0], detector_offset_y=off[1], arc=360.0 if n_proj > 3 else 0.6)
    det, pix = ((77, 45), (1.3, 1.7)) if case != "offsets_and_misses" else ((61, 39), (2.9, 2.3))
    got, ref, amb = _compare(vol, sp, org, geo, det, pix)
    assert got.shape == (n_proj, det[1], det[0])
    err = np.abs(got - ref)
    tol = 1e-5 * np.abs(ref) + 1e-5 * max(sp)
    bad = (err > tol) & ~amb
    assert not bad.any(), (case, int(bad.sum()), float(err[~amb].max()), int(amb.sum()))
    assert amb.mean() < 0.01
    assert (ref > 0).mean() > 0.1
    if case == "offsets_and_misses":
        assert (ref == 0).any() and np.all(got[ref == 0] == 0.0)  # rays that miss give exactly 0
    if case == "near_45":  # the main axis changes across the detector
        uu = fp.detector_origin(det, pix)[0] + pix[0] * np.arange(det[0])
        S, P = jr.ray_endpoints(geo.gantry_angles[0], 0.0, 0.0, geo.source_to_isocenter, geo.source_to_detector, uu, np.zeros_like(uu))
        axes = set(np.argmax(np.abs(P - S), axis=1))
        assert axes == {0, 2}


@pytest.mark.gpu
def test_off_centre_cube_lands_where_the_matrix_says(engine):
    n, s = 41, 2.0
    vol = np.zeros((n, n, n), np.float32)
    iX, iY, iZ = 30, 12, 8
    vol[iZ - 1:iZ + 2, iY - 1:iY + 2, iX - 1:iX + 2] = 1.0
    org = (-(n - 1) / 2 * s,) * 3
    centre = np.array([org[0] + iX * s, org[1] + iY * s, org[2] + iZ * s, 1.0])
    geo = recon.create_geometry(12, start_angle=90.0)  # half-fan: offset -159.856
    det, pix = (256, 192), (1.552, 1.552)
    out = fp.project_forward(fp.RTKImage(vol, (s, s, s), org), geo, detector_size=det, detector_pixel_spacing=pix).array
    u0, v0 = fp.detector_origin(det, pix)
    seen = 0
    for i in range(12):
        h = geo.matrix(i) @ centre
        pu, pv = (h[0] / h[2] - u0) / pix[0], (h[1] / h[2] - v0) / pix[1]
        if not (8 <= pu < det[0] - 8 and 8 <= pv < det[1] - 8):
            continue
        seen += 1
        w = out[i]
        vv, uu = np.meshgrid(np.arange(det[1]), np.arange(det[0]), indexing="ij")
        cu, cv = (w * uu).sum() / w.sum(), (w * vv).sum() / w.sum()
        assert abs(cu - pu) < 0.5 and abs(cv - pv) < 0.5, (i, cu, pu, cv, pv)
    assert seen >= 4


def _context(engine, tmp_path, g):
    inp = cases.build_case("water", tmp_path / "ctx")
    ctx = engine.create(inp, device=0)
    ctx.set_geometry(g)
    return ctx


def _u8_geometry():
    """A few (material, density) pairs on a grid that is no multiple of the 4^3 tiles of the u8 volume."""
    M = cases.materials
    g = cases.geometry.MCBoxGeometry(shape=(23, 18, 13), image_spacing=(7.0, 7.0, 7.0), material="h2o")
    g.densities[:] = np.float32(1.0)
    g.densities[3:11, 2:15, 1:9] = np.float32(1.25)
    g.materials[12:20, 5:9, 4:12], g.densities[12:20, 5:9, 4:12] = M.material_number("bone_050"), np.float32(1.6)
    g.materials[:, :, 11:], g.densities[:, :, 11:] = M.material_number("air"), np.float32(0.0013)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("kind, factory", [(0, _u8_geometry), (1, cases._graded(3000)), (2, cases._graded(80000))])
def test_context_volumes_equal_the_host_path(engine, tmp_path, kind, factory):
    """The context's u8 (tiled), u16 and raw float2 volumes, read in the .vox frame, give bit-for-bit the stack of the host path
    on the MCGeometry densities: the same traversal and arithmetic, only the voxel fetch differs, and the palette holds the same
    float32 densities."""
    g = factory()
    g.image_spacing = (6.0, 5.0, 4.0) if kind == 1 else g.image_spacing  # anisotropic: pins the spacing permutation too
    with _context(engine, tmp_path, g) as ctx:
        assert ctx.geti("volume_kind") == kind
        angles = [3.0, 47.0, 90.0, 181.5, 300.0, 359.0, 12.0]
        spacing, origin = fp.rtk_frame(g.image_shape, g.image_spacing)
        det, pix = (96, 64), (3.1, 3.1)
        got, rep = ctx.project_forward(angles, detector_size=det, detector_pixel_spacing=pix, spacing_iec=spacing, origin_iec=origin)
    geo = recon.create_geometry(0)
    for a in angles:
        geo.add_projection(a, pkg.defaults.DEFAULTS.detector_lateral_displacement, 0.0)
    img = fp.prepare_image_for_rtk(g.densities, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
    want = fp.project_forward(img, geo, detector_size=det, detector_pixel_spacing=pix).array
    assert (want > 0).mean() > 0.2
    np.testing.assert_array_equal(got, want)
    assert rep["ms_kernel"] > 0 and rep["ms_upload"] == 0


class _ShiftModel:  # the toy correspondence model of tests/test_4d.py: rigid SI shift proportional to the signal
    def __init__(self, shape, amplitude_voxels=3.4):
        self.shape, self.amp = shape, amplitude_voxels

    def predict(self, x):
        u = np.zeros((3,) + tuple(self.shape), dtype=np.float32)
        u[2] = self.amp * float(x[0])
        u[0] = 0.5 * float(x[1])
        return u


def _slab():
    g = cases.geometry.MCBoxGeometry(shape=(24, 20, 16), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[6:14, 5:15, 4:12] = cases.materials.material_number("bone_050")
    g.densities[6:14, 5:15, 4:12] = 1.4
    return g


@pytest.mark.gpu
def test_context_path_after_a_device_warp_equals_the_host_path(engine, tmp_path):
    g = _slab()
    field = _ShiftModel(g.image_shape).predict(np.array([0.8, -1.0]))
    with _context(engine, tmp_path, g) as ctx:
        ctx.warp_geometry(field, frame="geometry")
        spacing, origin = fp.rtk_frame(g.image_shape, g.image_spacing)
        got, _ = ctx.project_forward([0.0, 90.0, 200.0], detector_size=(80, 40), detector_pixel_spacing=(4.0, 4.0), spacing_iec=spacing,
                                     origin_iec=origin)
    wm, wd = warp_ref.warp_nearest(g.materials, g.densities, field, cases.materials.material_number("air"), cases.materials.MATERIALS_125KEV["air"])
    assert not np.array_equal(wd, g.densities)
    geo = recon.create_geometry(0)
    for a in (0.0, 90.0, 200.0):
        geo.add_projection(a, pkg.defaults.DEFAULTS.detector_lateral_displacement, 0.0)
    img = fp.prepare_image_for_rtk(wd, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
    np.testing.assert_array_equal(got, fp.project_forward(img, geo, detector_size=(80, 40), detector_pixel_spacing=(4.0, 4.0)).array)


def _water_cylinder_with_bone_rod():
    """The phantom of tests/test_fdk.py::test_mc_scan_to_fdk_round_trip (MC [x, y, z], 5 mm voxels)."""
    M = cases.materials
    shape, vs = (48, 48, 32), (5.0, 5.0, 5.0)
    x, y, z = np.meshgrid(*[(np.arange(n) + 0.5 - n / 2) * s for n, s in zip(shape, vs)], indexing="ij", sparse=True)
    mats = np.full(shape, M.material_number("air"), np.uint8)
    dens = np.full(shape, 0.0012, np.float32)
    body = (x ** 2 + y ** 2 <= 100.0 ** 2) & (np.abs(z) <= 65)
    mats[body], dens[body] = M.material_number("h2o"), 1.0
    bone = ((x - 45) ** 2 + (y - 20) ** 2 <= 18.0 ** 2) & (np.abs(z) <= 40)
    mats[bone], dens[bone] = M.material_number("bone_050"), 1.6
    hole = ((x + 30) ** 2 + (y + 50) ** 2 <= 14.0 ** 2) & (np.abs(z - 10) <= 30)
    mats[hole], dens[hole] = M.material_number("air"), 0.0012
    return pkg.geometry.MCGeometry(mats, dens, vs)


def _phantom_on_grid(g, px, py, pz):
    shape, vs = g.image_shape, g.image_spacing
    ix, iy, iz = [np.floor(p / s + n / 2).astype(int) for p, s, n in zip((px, py, pz), vs, shape)]
    ok = (ix >= 0) & (ix < shape[0]) & (iy >= 0) & (iy < shape[1]) & (iz >= 0) & (iz < shape[2])
    return np.where(ok, g.densities[np.clip(ix, 0, shape[0] - 1), np.clip(iy, 0, shape[1] - 1), np.clip(iz, 0, shape[2] - 1)], 0.0)


@pytest.mark.gpu
def test_fp_then_fdk_returns_the_density(engine, tmp_path):
    """A density forward projection reconstructed by FDK returns density: water cylinder + bone rod on 360 half-fan angles."""
    g = _water_cylinder_with_bone_rod()
    geo = fp.create_geometry(360, start_angle=90.0)
    det, pix = (256, 192), (1.552, 1.552)
    img = fp.prepare_image_for_rtk(g.densities, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
    stack = fp.project_forward(img, geo, detector_size=det, detector_pixel_spacing=pix)
    w = engine.StackWriter(tmp_path / "density_fp.mha", det[0], det[1], 360, pix)
    for plane in stack.array:
        w.append(plane)
    w.finish(replace_zeros=False)
    fp.save_geometry(geo, tmp_path / "geometry.xml")
    dim, sp = (64, 48, 64), (4.0, 4.0, 4.0)
    # pad = 0: the phantom is inside the field of view, so no row is truncated but the half-fan cut, where the feathered extension of
    # pad = 1 adds data that is not there (measured: the water interior comes back 3.7 % high with pad = 1)
    out, _ = recon.reconstruct_3d(tmp_path / "density_fp.mha", tmp_path / "geometry.xml", dimension=dim, spacing=sp, pad=0.0)
    vol, _, _ = recon.read_mha(out)
    X, Y, Z = [-(n - 1) / 2 * s + s * np.arange(n) for n, s in zip(dim, sp)]
    zi, yi, xi = np.meshgrid(Z, Y, X, indexing="ij")
    ref = _phantom_on_grid(g, xi, -zi, -yi)
    cc = np.corrcoef(ref.ravel(), vol.ravel())[0, 1]
    assert cc > 0.95, cc
    inner = _phantom_on_grid(g, xi + 8, -zi, -yi) + _phantom_on_grid(g, xi - 8, -zi, -yi) + _phantom_on_grid(g, xi, -zi + 8, -yi) \
        + _phantom_on_grid(g, xi, -zi - 8, -yi)
    water = vol[(np.abs(ref - 1.0) < 1e-6) & (np.abs(inner - 4.0) < 1e-5) & (np.abs(yi) < 40)]
    assert water.size > 1000 and abs(water.mean() - 1.0) < 0.03, (water.size, water.mean())


MC_ALIGNMENT_MIN_CC = 0.98  # measured on an MI355X: 0.990 (mirrored 0.987, shifted 0.941, rotated by 180 degrees 0.986)


@pytest.mark.gpu
def test_mc_projections_line_up_with_the_density_fp(engine, tmp_path):
    """The reference's own geometry check (scripts/brute_force_test_geometry_fp.py): the air-normalised Monte Carlo stack
    (half-fan crop) correlates with mu_water x the density FP on the scan's RTK geometry (start angle 90 degrees) better than
    with the FPs of the mirrored or shifted phantom."""
    g = _water_cylinder_with_bone_rod()
    n_proj, det = 40, dict(n_detector_pixels=(462, 192), detector_size=(717.024, 297.984))
    sim = pkg.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), n_histories=int(1.5e7), n_projections=n_proj,
                                      angle_between_projections=360.0 / n_proj, **det)
    inp = sim.prepare_simulation(tmp_path, compress_geometry=False, engine=engine, binary_sidecar=True)
    air = pkg.simulation.MCSimulation(pkg.geometry.MCAirGeometry(), cases.material_files(), cases.spectrum_file(), n_histories=int(1e9), n_projections=1, **det)
    air_inp = air.prepare_simulation(tmp_path / "air", compress_geometry=False, engine=engine)
    with engine.create(air_inp, device=0) as ctx:
        ctx.run_scan(mode="fast", crop_nx=256, output_folder=tmp_path / "air", pixel_spacing=(1.552, 1.552))
    with engine.create(inp, device=0) as ctx:
        ctx.run_scan(mode="fast", crop_nx=256, output_folder=tmp_path, air_stack=tmp_path / "air" / "projections_total.mha", air_sigma=(3.0, 3.0),
                     pixel_spacing=(1.552, 1.552))
    mc, _, _ = recon.read_mha(tmp_path / "projections_total_normalized.mha")
    geo = fp.create_geometry(n_proj, start_angle=90.0)
    mu_water = 0.019  # 1/mm; the correlation does not depend on it

    def density_fp(dens, angle_shift=0.0):
        gg = fp.create_geometry(n_proj, start_angle=90.0 + angle_shift)
        img = fp.prepare_image_for_rtk(dens, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
        return mu_water * fp.project_forward(img, gg, detector_size=(256, 192), detector_pixel_spacing=(1.552, 1.552)).array

    assert mc.shape == (n_proj, 192, 256) and len(geo.gantry_angles) == n_proj
    cc = lambda a: float(np.corrcoef(mc.ravel(), a.ravel())[0, 1])
    right = cc(density_fp(g.densities))
    mirrored = cc(density_fp(g.densities[::-1].copy()))
    shifted = cc(density_fp(np.roll(g.densities, 6, axis=1)))
    rotated = cc(density_fp(g.densities, angle_shift=180.0))
    print(f"MC vs density FP correlation: right {right:.4f} mirrored {mirrored:.4f} shifted {shifted:.4f} rotated by 180 deg {rotated:.4f}")
    assert right > MC_ALIGNMENT_MIN_CC, right
    assert right > max(mirrored, shifted, rotated), (right, mirrored, shifted, rotated)


@pytest.mark.gpu
def test_4d_density_fp_slices_are_the_host_fp_of_each_state(engine, tmp_path):
    """density_fp_4d.mha (scripts/run_mc_simulations.py:491-556): slice i = FP of projection i's warped geometry at FP angle =
    MC angle - 180 degrees, projected on the resident context; equal to the host FP of the host-warped arrays."""
    g = _slab()
    R = pkg.respiratory.RespiratorySignal
    model = _ShiftModel(g.image_shape)
    n_proj, step, fdet, fpix = 12, 30.0, (64, 40), (6.0, 6.0)
    sim4d = cases.simulation.MCSimulation4D(model, g, cases.material_files(), cases.spectrum_file(), n_histories=100_000, n_projections=n_proj,
                                            frame_rate=15.0, angle_between_projections=step, **cases.SMALL_DET)
    signal = R.create_sin4(total_seconds=2.0, period=1.0, sampling_frequency=25.0)
    rep = sim4d.run_simulation(signal, 2, tmp_path / "out", engine, mode="fast", forward_projection=True, fp_detector_size=fdet,
                               fp_detector_pixel_spacing=fpix)
    assert rep["unique_states"] >= 2
    stack, sp, org = recon.read_mha(tmp_path / "out" / "density_fp_4d.mha")
    assert stack.shape == (n_proj, fdet[1], fdet[0])
    assert sp == pytest.approx([6.0, 6.0, 1.0]) and org == pytest.approx([-0.5 * 64 * 6.0, -0.5 * 40 * 6.0, 0.0])
    sig = signal.resample(15.0)
    s, ds = R.quantize_signal(sig.signal[:n_proj], 2), R.quantize_signal(sig.dt_signal[:n_proj], 2)
    seen = set()
    for (sv, dsv), idx in R.get_unique_signals(s, ds).items():
        wm, wd = warp_ref.warp_nearest(g.materials, g.densities, model.predict(np.array([sv, dsv])), cases.materials.material_number("air"),
                                       cases.materials.MATERIALS_125KEV["air"])
        img = fp.prepare_image_for_rtk(wd, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
        geo = fp.create_geometry(0)
        for i in idx:
            geo.add_projection(270.0 + i * step - 180.0, pkg.defaults.DEFAULTS.detector_lateral_displacement, 0.0)
        want = fp.project_forward(img, geo, detector_size=fdet, detector_pixel_spacing=fpix).array
        np.testing.assert_array_equal(stack[idx], want)
        seen.update(idx)
    assert seen == set(range(n_proj))
