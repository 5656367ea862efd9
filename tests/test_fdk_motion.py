"""Row f15: motion-compensated FDK.  CPU: the float64 restatement (tests/fdk_motion_ref.py) against the FDK oracle and a moving
sphere, the frame conversion of `MotionModel.from_correspondence_model`, the plumbing of `build_default(inverse=True)`.
GPU: backproject_motion_kernel through `fdk_motion` against the restatement, its determinism, the C ABI's refusals and the file flow
of `reconstruct_3d_mc`.  Parity against RTK's warp back-projector is unpinned (RTK is absent)."""
import ctypes as C
import functools

import numpy as np
import pytest

import abi_layout
import cases
import fdk_motion_ref as mr
import registration_ref as R
from fdk_motion_ref import fo

pkg = cases.pkg
recon = pkg.reconstruction
CorrespondenceModel = pkg.correspondence.CorrespondenceModel

BATCH = 32                 # kMotionBatch of csrc/fdk.hip
TOLERANCE = 2e-4           # x max|want|: the project's figure for float32 kernels against the float64 restatement (tests/test_fdk.py)
MASK_CAP = 0.01            # the ambiguous voxels left out of the comparison: at most 1 %


def _half_fan_case(n=120, nu=96, nv=64, du=4.0, off_x=-80.0):
    """The case of tests/test_fdk.py: a sphere of 60 mm radius off the axis, 4 mm pixels."""
    geo = recon.create_geometry(n, start_angle=90.0, detector_offset_x=off_x)
    u0, v0 = -(nu - 1) / 2 * du, -(nv - 1) / 2 * du
    proj = fo.sphere_projections(0.02, 60.0, (20.0, 5.0, -10.0), n, nu, nv, du, du, u0, v0, geo.source_to_isocenter, geo.source_to_detector,
                                 np.array(geo.gantry_angles), np.array(geo.projection_offsets_x), np.array(geo.projection_offsets_y))
    return geo, proj, (du, du), (u0, v0)


def _geo_args(geo):
    return geo.source_to_isocenter, geo.source_to_detector, np.array(geo.gantry_angles), np.array(geo.projection_offsets_x), np.array(geo.projection_offsets_y)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def test_zero_model_restatement_equals_the_fdk_oracle():
    geo, proj, (du, dv), (u0, v0) = _half_fan_case(n=24)
    dim, sp = (24, 12, 20), (5.0, 5.0, 6.0)
    proj = proj + 0.05 * np.random.default_rng(2).normal(size=proj.shape)
    want = fo.reconstruct(proj, du, dv, u0, v0, *_geo_args(geo), dim, sp, hann=1.0, hann_y=1.0, pad=0.5)
    zero = np.zeros((3, dim[2], dim[1], dim[0]), np.float32)
    got = mr.reconstruct(proj, du, dv, u0, v0, *_geo_args(geo), zero, zero[None], np.ones((24, 1)), dim, sp, hann=1.0, hann_y=1.0, pad=0.5)
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------- CPU: the frame conversion
def _model_from_fields(fields, signals):
    return CorrespondenceModel().fit(np.asarray(fields, dtype=np.float32), signals, reference_phase=0)


def test_a_constant_field_converts_to_the_fdk_frame():
    """(1, 2, 3) voxels along MC x, y, z at spacing (2, 3, 5) mm = (2, -15, -6) mm along IEC X, Y, Z: (ux sx, -uz sz, -uy sy)."""
    shape = (4, 5, 6)
    base = np.broadcast_to(np.array([1.0, 2.0, 3.0])[:, None, None, None], (3,) + shape)
    signals = np.array([[-1.0], [0.0], [1.0]])
    model = _model_from_fields(np.stack([base * (1.0 + 0.5 * s[0]) for s in signals]), signals)
    motion = recon.MotionModel.from_correspondence_model(model, (2.0, 3.0, 5.0))
    assert motion.dimension == (4, 6, 5) and motion.spacing == (2.0, 5.0, 3.0) and motion.n_signal_dims == 1
    assert motion.mean.dtype == np.float32 and motion.mean.shape == (3, 5, 6, 4) and motion.coefficients.shape == (1, 3, 5, 6, 4)
    for c, want in enumerate((2.0, -15.0, -6.0)):
        assert np.allclose(motion.mean[c], want, rtol=1e-6, atol=0)
        assert np.allclose(motion.coefficients[0, c], 0.5 * want, rtol=1e-5, atol=0)
    assert np.allclose(motion.delta([[0.25]]), 0.25) and motion.mean_signal.shape == (1,)
    with pytest.raises(ValueError, match="grid"):
        motion.check_grid((4, 5, 6), (2.0, 5.0, 3.0))
    with pytest.raises(ValueError, match="spacing"):
        motion.check_grid((4, 6, 5), (2.0, 3.0, 5.0))


def _convert64(u, spacing):
    """The conversion rule in float64, without the model's float32 rounding: [3, gx, gy, gz] voxels -> [3, nz, ny, nx] mm."""
    to = pkg.water_precorrection.to_fdk_frame
    return np.stack([to(u[0] * spacing[0]), to(-u[2] * spacing[2]), to(-u[1] * spacing[1])])


def test_a_warp_commutes_with_the_frame_conversion():
    """to_fdk_frame(warp(img, u)) = trilinear sampling of to_fdk_frame(img) at the converted displacements: the permutation, the signs
    and the scaling of the components fit the axis rule of the arrays.  Also: from_correspondence_model is that rule, rounded."""
    to = pkg.water_precorrection.to_fdk_frame
    shape, spacing = (10, 12, 14), (2.0, 3.0, 5.0)
    rng = np.random.default_rng(11)
    img = rng.normal(size=shape)
    u = 1.5 * R.smooth(rng.normal(size=(3,) + shape), (2.0, 2.0, 2.0)) / 0.2
    assert 0.5 < np.abs(u).max() < 5.0
    d = _convert64(u, spacing)                       # mm along IEC X, Y, Z on [nz][ny][nx]
    nz, ny, nx = d.shape[1:]
    assert (nx, ny, nz) == (10, 14, 12)
    sX, sY, sZ = spacing[0], spacing[2], spacing[1]
    iz, iy, ix = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    got = R.sample(to(img), [iz + d[2] / sZ, iy + d[1] / sY, ix + d[0] / sX])
    want = to(R.warp(img, u))
    assert np.abs(got - want).max() < 1e-12
    signals = np.array([[-1.0], [1.0]])
    motion = recon.MotionModel.from_correspondence_model(_model_from_fields(np.stack([0.5 * u, 1.5 * u]), signals), spacing)
    assert np.abs(motion.mean - d).max() < 1e-5 and np.abs(motion.coefficients[0] - 0.5 * d).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------- CPU: build_default
@pytest.mark.parametrize("masked", [True, False])
def test_build_default_inverse_swaps_the_roles(monkeypatch, masked):
    rng = np.random.default_rng(0)
    images = rng.normal(size=(4, 6, 5, 4)).astype(np.float32)
    masks = (rng.uniform(size=images.shape) > 0.5).astype(np.uint8)
    signals = np.array([[0.0, 1.0], [1.0, 0.5], [2.0, -1.0], [3.0, 0.0]])
    calls = []

    def register(fixed, moving, fixed_mask=None, gpu_id=0, **parameters):
        calls.append((fixed, moving, fixed_mask, gpu_id, parameters))
        return np.full((3,) + fixed.shape, float(len(calls)), np.float32), {}

    monkeypatch.setattr(pkg.registration, "register", register)
    for inverse in (True, False, None):
        calls.clear()
        kw = {} if inverse is None else dict(inverse=inverse)
        model = CorrespondenceModel.build_default(images, signals=signals, masks=masks, reference_phase=1, masked_registration=masked, gpu_id=2, iterations=3, **kw)
        assert len(calls) == 4 and model.is_fitted and model.reference_phase == 1
        for t, (fixed, moving, fixed_mask, gpu_id, parameters) in enumerate(calls):
            assert gpu_id == 2 and parameters == dict(iterations=3)
            if inverse:
                assert fixed is not None and np.shares_memory(fixed, images[1]) and np.array_equal(moving, images[t]) and np.shares_memory(moving, images[t])
                assert (fixed_mask is None) if not masked else np.shares_memory(fixed_mask, masks[1])
            else:
                assert np.shares_memory(fixed, images[t]) and np.shares_memory(moving, images[1])
                assert (fixed_mask is None) if not masked else np.shares_memory(fixed_mask, masks[t])


# ---------------------------------------------------------------------------------------------------------------- the moving sphere
SPHERE = dict(n=90, nu=96, nv=64, du=4.0, dim=(40, 32, 40), sp=(4.0, 4.0, 4.0), mu=0.02, radius=24.0, centre=(8.0, -4.0, 12.0), a=(6.0, 8.0, 4.0))


@functools.lru_cache(maxsize=None)
def _sphere_case():
    """A sphere of radius 6 voxels whose centre moves rigidly by a s_i, s_i the breathing curve in [-1, 1]: peak to peak 2 |a| = 21.5 mm
    = 5.4 voxels, of which 4 voxels along the axis (Y) and 3.6 voxels in the plane.  -> geometry, static and moving projections
    (float32), the signals and the model (mean 0, coefficients = a, K = 1)."""
    c = SPHERE
    n, nu, nv, du = c["n"], c["nu"], c["nv"], c["du"]
    geo = recon.create_geometry(n, start_angle=90.0, detector_offset_x=0.0)
    u0, v0 = -(nu - 1) / 2 * du, -(nv - 1) / 2 * du
    s, _ = mr.breathing(n)
    angles, offx, offy = np.array(geo.gantry_angles), np.array(geo.projection_offsets_x), np.array(geo.projection_offsets_y)
    static = fo.sphere_projections(c["mu"], c["radius"], c["centre"], n, nu, nv, du, du, u0, v0, geo.source_to_isocenter, geo.source_to_detector, angles, offx, offy)
    moving = np.concatenate([fo.sphere_projections(c["mu"], c["radius"], tuple(np.array(c["centre"]) + np.array(c["a"]) * s[i]), 1, nu, nv, du, du, u0, v0,
                                                   geo.source_to_isocenter, geo.source_to_detector, angles[i:i + 1], offx[i:i + 1], offy[i:i + 1]) for i in range(n)])
    nx, ny, nz = c["dim"]
    mean = np.zeros((3, nz, ny, nx), np.float32)
    coefficients = np.broadcast_to(np.array(c["a"], np.float32)[None, :, None, None, None], (1, 3, nz, ny, nx)).copy()
    return geo, static.astype(np.float32), moving.astype(np.float32), (du, du), (u0, v0), s[:, None], mean, coefficients


def _sphere_rms(vol):
    c = SPHERE
    inside, shell = mr.sphere_masks(c["dim"], c["sp"], c["centre"], c["radius"], 1.0 * c["sp"][0], 4.0 * c["sp"][0])
    err = np.concatenate([vol[inside] - c["mu"], vol[shell]])
    return float(np.sqrt(np.mean(err ** 2)))


def test_restatement_sharpens_a_moving_sphere():
    """rms error against the analytic static sphere over its interior (r < R - 1 voxel) and a shell (R + 1 .. R + 4 voxels), in
    units of mu = 0.02:  e_static = 0.0054 mu (FDK of the static projections), e_blur = 0.1353 mu (plain FDK of the moving ones, 25 x
    e_static where 3 x is asked), e_mc = 0.0060 mu (the restatement on the moving projections with the model that moved the sphere).
    The assertion: e_mc <= (e_static + e_blur) / 2."""
    geo, static, moving, (du, dv), (u0, v0), signals, mean, coefficients = _sphere_case()
    c = SPHERE
    e_static = _sphere_rms(fo.reconstruct(static, du, dv, u0, v0, *_geo_args(geo), c["dim"], c["sp"], hann=1.0))
    e_blur = _sphere_rms(fo.reconstruct(moving, du, dv, u0, v0, *_geo_args(geo), c["dim"], c["sp"], hann=1.0))
    e_mc = _sphere_rms(mr.reconstruct(moving, du, dv, u0, v0, *_geo_args(geo), mean, coefficients, signals, c["dim"], c["sp"], hann=1.0))
    print(f"moving sphere, float64: e_static {e_static / c['mu']:.4f} mu, e_blur {e_blur / c['mu']:.4f} mu, e_mc {e_mc / c['mu']:.4f} mu")
    assert e_blur >= 3.0 * e_static, (e_static, e_blur)
    assert e_mc <= 0.5 * (e_static + e_blur), (e_static, e_blur, e_mc)


# ---------------------------------------------------------------------------------------------------------------- GPU: the kernel
# name -> K, off_x, n, dim, hann, hann_y, pad, wpc, amplitude [mm] (at most 2 voxels of 5 x 5 x 6 mm), offset of the mean [mm]
_BASE = dict(K=2, off_x=-80.0, n=90, dim=(48, 30, 40), hann=0.0, hann_y=0.0, pad=0.0, wpc=None, amplitude=(10.0, 10.0, 12.0), offset=(0.0, 0.0, 0.0))
CASES = {
    "k1_plain": dict(K=1),
    "k2_centred_filters_wpc": dict(off_x=0.0, hann=0.7, hann_y=0.5, pad=0.5, wpc=(0.0, 1.05, 0.01)),
    "k4_right_hann": dict(K=4, off_x=150.0, hann=1.0, hann_y=1.0),
    "batch_plus_one": dict(n=BATCH + 1, hann=1.0),
    "below_one_batch": dict(n=5, K=1, hann_y=1.0),
    "k3_below_one_batch": dict(K=3, n=7, dim=(45, 7, 11)),
    "odd_grid": dict(dim=(45, 7, 11), K=4, pad=0.3),                        # 3465 voxels: 13 blocks and 137 threads
    "one_column": dict(dim=(1, 30, 40), hann=1.0),
    "off_the_detector": dict(offset=(110.0, 45.0, -30.0), hann=1.0, hann_y=1.0),  # the range test refuses samples along u and along v
}
SP = (5.0, 5.0, 6.0)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = dict(_BASE, **CASES[name])
    geo, proj, (du, dv), (u0, v0) = _half_fan_case(n=c["n"], off_x=c["off_x"])
    proj = (proj + 0.05 * np.random.default_rng(5).normal(size=proj.shape)).astype(np.float32)
    mean, coefficients = mr.smooth_model(c["dim"], SP, c["K"], c["amplitude"], offset_mm=c["offset"])
    return c, geo, proj, (du, dv), (u0, v0), mean, coefficients, mr.signal_columns(c["n"], c["K"])


@functools.lru_cache(maxsize=None)
def _want(name):
    """(restatement, mask of the ambiguous voxels, stats) of a case, computed once."""
    c, geo, proj, (du, dv), (u0, v0), mean, coefficients, delta = _case(name)
    stats = {}
    want = mr.reconstruct(proj, du, dv, u0, v0, *_geo_args(geo), mean, coefficients, delta, c["dim"], SP, hann=c["hann"], hann_y=c["hann_y"], wpc=c["wpc"],
                          pad=c["pad"], stats=stats)
    mask = mr.ambiguous_voxels(proj.shape[2], proj.shape[1], du, dv, u0, v0, *_geo_args(geo), mean, coefficients, delta, c["dim"], SP)
    return want, mask, stats


@pytest.mark.parametrize("name", list(CASES))
def test_the_ambiguous_voxels_stay_under_the_cap(name):
    """Checked without a GPU: the comparison of test_kernel_equals_the_restatement leaves out at most 1 % of a case's voxels; the
    displacement stays within 2 voxels (plus the constant offset); the off-detector case really is refused along u and along v."""
    c, geo, proj, _, _, mean, coefficients, delta = _case(name)
    want, mask, stats = _want(name)
    assert mask.mean() <= MASK_CAP, mask.mean()
    moved = np.abs(mean - np.array(c["offset"], np.float32)[:, None, None, None]) + sum(np.abs(coefficients[k]) * np.abs(delta[:, k]).max() for k in range(c["K"]))
    assert all(0.0 < moved[i].max() <= 2.0 * SP[i] for i in range(3)), [moved[i].max() for i in range(3)]
    if name == "off_the_detector":
        _, _, usual = _want("k1_plain")   # the same grid and detector with a model that stays inside
        assert stats["refused_u"] > usual["refused_u"] + 0.05 * want.size * c["n"] and stats["refused_v"] > usual["refused_v"] + 0.05 * want.size * c["n"]
        assert np.count_nonzero(want) > 0.25 * want.size


def _fdk_motion(name, **over):
    c, geo, proj, ds, org, mean, coefficients, delta = _case(name)
    motion = recon.MotionModel(mean, coefficients, np.zeros(c["K"]))
    return recon.fdk_motion(proj, geo, ds, org, motion, delta, c["dim"], SP, hann=c["hann"], hann_y=c["hann_y"], water_pre_correction=c["wpc"], pad=c["pad"], **over)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement(engine, name):
    """backproject_motion_kernel against the float64 restatement, the ambiguous voxels (<= 1 %) left out: 2e-4 x max |want|, the
    figure of test_hip_fdk_matches_the_oracle.  Measured on an MI355X: 5e-7 .. 5e-6 over the cases, so the wider bound the extra
    float32 rounding of the displaced coordinate could have asked for is not needed."""
    want, mask, _ = _want(name)
    got, rep = _fdk_motion(name)
    scale = np.abs(want).max()
    assert got.shape == want.shape and scale > 0 and np.isfinite(got).all()
    err = float(np.abs(got - want)[~mask].max() / scale)
    print(f"{name}: max |kernel - restatement| = {err:.3e} x max|want|, {mask.mean() * 100:.3f} % of the voxels masked")
    assert err < TOLERANCE
    assert rep["ms_backproject"] > 0 and rep["ms_upload_model"] > 0 and rep["peak_device_bytes"] > 4 * want.size * (1 + 3 * (1 + _case(name)[0]["K"]))


@pytest.mark.gpu
def test_zero_model_agrees_with_plain_fdk(engine):
    c, geo, proj, ds, org, mean, coefficients, delta = _case("k4_right_hann")
    zero = recon.MotionModel(np.zeros_like(mean), np.zeros_like(coefficients), np.zeros(c["K"]))
    got, _ = recon.fdk_motion(proj, geo, ds, org, zero, delta, c["dim"], SP, hann=c["hann"], hann_y=c["hann_y"])
    plain, _ = recon.fdk(proj, geo, ds, org, c["dim"], SP, hann=c["hann"], hann_y=c["hann_y"])
    scale = np.abs(plain).max()
    mask = fo.ambiguous_voxels(proj.shape[2], proj.shape[1], *ds, *org, *_geo_args(geo), c["dim"], SP)
    assert mask.mean() <= MASK_CAP
    err = float(np.abs(got - plain)[~mask].max() / scale)
    print(f"zero model against plain FDK: {err:.3e} x max")
    assert err < TOLERANCE


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes(engine):
    a, _ = _fdk_motion("k4_right_hann")
    b, _ = _fdk_motion("k4_right_hann")
    assert a.tobytes() == b.tobytes() and np.abs(a).max() > 0


@pytest.mark.gpu
def test_fdk_motion_sharpens_a_moving_sphere(engine):
    """test_restatement_sharpens_a_moving_sphere through the public functions, under the same assertion."""
    geo, static, moving, ds, org, signals, mean, coefficients = _sphere_case()
    c = SPHERE
    e_static = _sphere_rms(recon.fdk(static, geo, ds, org, c["dim"], c["sp"], hann=1.0)[0])
    e_blur = _sphere_rms(recon.fdk(moving, geo, ds, org, c["dim"], c["sp"], hann=1.0)[0])
    motion = recon.MotionModel(mean, coefficients, [0.0], spacing=c["sp"])
    e_mc = _sphere_rms(recon.fdk_motion(moving, geo, ds, org, motion, signals, c["dim"], c["sp"], hann=1.0)[0])
    print(f"moving sphere, device: e_static {e_static / c['mu']:.4f} mu, e_blur {e_blur / c['mu']:.4f} mu, e_mc {e_mc / c['mu']:.4f} mu")
    assert e_blur >= 3.0 * e_static, (e_static, e_blur)
    assert e_mc <= 0.5 * (e_static + e_blur), (e_static, e_blur, e_mc)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """mcgpu_fdk_motion and mcgpu_fdk_motion_report: the header's field names in order, sizeof and every offsetof as the C compiler
    lays them out, against the ctypes mirrors (tests/abi_layout.py)."""
    mirrors = [("mcgpu_fdk_motion", recon._FdkMotion), ("mcgpu_fdk_motion_report", recon._FdkMotionReport)]
    abi_layout.assert_field_names(mirrors)
    cc = abi_layout.c_compiler()
    assert cc is not None, "no C compiler"
    c_side = abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    assert c_side["mcgpu_fdk_motion"] == "32"


class _Tiny:
    """mcgpu_fdk_reconstruct_motion through ctypes on the smallest valid problem (two projections, 2 x 2 pixels, one voxel, K = 2)."""

    def __init__(self):
        self.lib = pkg.engine.load_library()
        self.lib.mcgpu_fdk_reconstruct_motion.argtypes = [C.POINTER(recon._FdkOptions), C.POINTER(recon._FdkMotion), C.c_void_p, C.c_void_p,
                                                          C.POINTER(recon._FdkMotionReport)]
        self.lib.mcgpu_fdk_reconstruct_motion.restype = C.c_int
        self.angle = np.array([30.0, 200.0])
        self.proj = np.array([[[1.0, 2.0], [3.0, 4.0]], [[2.0, 1.0], [4.0, 3.0]]], np.float32)
        self.mean = np.zeros(3, np.float32)
        self.coefficients = np.full(6, 0.1, np.float32)
        self.delta = np.array([[0.5, -0.5], [1.0, 0.25]])

    def options(self):
        return recon._FdkOptions(C.sizeof(recon._FdkOptions), 2, 2, 2, 4.0, 4.0, -2.0, -2.0, 1000.0, 1500.0, self.angle.ctypes.data_as(C.POINTER(C.c_double)),
                                 None, None, 1, 1, 1, 1.0, 1.0, 1.0, *(float("nan"),) * 3, 0.0, 0.0, None, 0, 0, 0.0)

    def motion(self, **fields):
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        m = recon._FdkMotion(C.sizeof(recon._FdkMotion), 2, self.mean.ctypes.data_as(fp), self.coefficients.ctypes.data_as(fp), self.delta.ctypes.data_as(dp))
        for k, v in fields.items():
            setattr(m, k, v)
        return m

    def __call__(self, o, m, projections=True, volume=True):
        vol = np.full((1, 1, 1), -1.0, np.float32)
        rc = self.lib.mcgpu_fdk_reconstruct_motion(C.byref(o) if o is not None else None, C.byref(m) if m is not None else None,
                                                   self.proj.ctypes.data if projections else None, vol.ctypes.data if volume else None, None)
        return rc, vol, self.lib.mcgpu_last_error().decode(errors="replace")


_FN = "!!ERROR!! mcgpu_fdk_reconstruct_motion: "
_REFUSALS = {
    "motion": (lambda t: (t.options(), None), _FN + "set mcgpu_fdk_motion.struct_size = sizeof(mcgpu_fdk_motion)"),
    "struct_size": (lambda t: (t.options(), t.motion(struct_size=0)), _FN + "set mcgpu_fdk_motion.struct_size = sizeof(mcgpu_fdk_motion)"),
    "options": (lambda t: (None, t.motion()), _FN + "set mcgpu_fdk_options.struct_size = sizeof(mcgpu_fdk_options)"),
    "K=0": (lambda t: (t.options(), t.motion(n_signal_dims=0)), _FN + "n_signal_dims must lie in 1..4"),
    "K=5": (lambda t: (t.options(), t.motion(n_signal_dims=5)), _FN + "n_signal_dims must lie in 1..4"),
    "mean": (lambda t: (t.options(), t.motion(mean=C.POINTER(C.c_float)())), _FN + "bad argument"),
    "coefficients": (lambda t: (t.options(), t.motion(coefficients=C.POINTER(C.c_float)())), _FN + "bad argument"),
    "delta": (lambda t: (t.options(), t.motion(delta=C.POINTER(C.c_double)())), _FN + "bad argument"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(_REFUSALS) + ["projections", "volume", "nan", "inf", "beyond_float32"])
def test_abi_refuses_and_a_valid_call_follows(engine, what):
    """-1 and a message with the volume untouched, before any HIP call; the next, valid call on the thread succeeds."""
    t = _Tiny()
    if what in _REFUSALS:
        make, message = _REFUSALS[what]
        rc, vol, msg = t(*make(t))
    elif what in ("projections", "volume"):
        rc, vol, msg = t(t.options(), t.motion(), projections=what != "projections", volume=what != "volume")
        message = _FN + "bad argument"
    else:
        t.delta[1, 0] = dict(nan=np.nan, inf=-np.inf, beyond_float32=1e39)[what]
        rc, vol, msg = t(t.options(), t.motion())
        message = _FN + "delta is not finite"
        t.delta[1, 0] = 1.0
    assert rc == -1 and msg == message and np.all(vol == -1.0)
    rc, vol, msg = t(t.options(), t.motion())
    assert rc == 0, msg
    assert np.isfinite(vol).all() and vol[0, 0, 0] != -1.0


# ---------------------------------------------------------------------------------------------------------------- the file flow
@pytest.mark.gpu
def test_reconstruct_3d_mc_file_flow(engine, tmp_path):
    """Stack + geometry.xml + a fitted correspondence model in, recon_fdk3d_mc.mha (+ .yaml with the model's hash and K) out, at the
    offset and spacing reconstruct_3d writes; equal to fdk_motion on the converted model; a model on another grid is refused."""
    import yaml
    geo, proj, (du, dv), (u0, v0) = _half_fan_case(n=20, off_x=-80.0)
    recon.write_mha(tmp_path / "projections_total_normalized.mha", proj.astype(np.float32), (du, dv, 1.0), (u0, v0, 0.0))
    geo.write(tmp_path / "geometry.xml")
    shape, voxel = (12, 10, 8), (10.0, 12.0, 14.0)          # MCGeometry: [x, y, z] -> the FDK grid (12, 8, 10) at (10, 14, 12) mm
    dim, sp = (12, 8, 10), (10.0, 14.0, 12.0)
    rng = np.random.default_rng(4)
    base = R.smooth(rng.normal(size=(3,) + shape), (2.0, 2.0, 2.0)) * 4.0
    model_signals = np.array([[-1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, -1.0]])
    model = _model_from_fields(np.stack([base * s[0] + base[::-1] * 0.3 * s[1] for s in model_signals]), model_signals)
    signals = mr.signal_columns(20, 2)
    out, rep = recon.reconstruct_3d_mc(tmp_path / "projections_total_normalized.mha", tmp_path / "geometry.xml", model, signals, voxel, dimension=dim, spacing=sp)
    assert out == tmp_path / "reconstructions" / "recon_fdk3d_mc.mha" and rep["ms_backproject"] > 0
    vol, vsp, vorg = recon.read_mha(out)
    plain_out, _ = recon.reconstruct_3d(tmp_path / "projections_total_normalized.mha", tmp_path / "geometry.xml", dimension=dim, spacing=sp)
    plain, psp, porg = recon.read_mha(plain_out)
    assert vol.shape == plain.shape == (10, 8, 12) and vsp == psp == [10.0, 14.0, 12.0] and vorg == porg == [-55.0, -49.0, -54.0]
    record = yaml.safe_load(out.with_suffix(".yaml").read_text())
    assert record["motion"] == model.model_hash[:7] and record["signal_n_dims"] == 2 and record["pad"] == 1.0 and record["hann"] == 1.0
    motion = recon.MotionModel.from_correspondence_model(model, voxel, dimension=dim, spacing=sp)
    direct, _ = recon.fdk_motion(proj.astype(np.float32), geo, (du, dv), (u0, v0), motion, signals, dim, sp, hann=1.0, hann_y=1.0, pad=1.0)
    assert vol.tobytes() == direct.tobytes() and np.abs(vol - plain).max() > 1e-3 * np.abs(plain).max()
    with pytest.raises(ValueError, match="resample the model"):
        recon.MotionModel.from_correspondence_model(model, voxel, dimension=(12, 10, 8), spacing=sp)
    with pytest.raises(ValueError, match="resample the model"):
        recon.reconstruct_3d_mc(tmp_path / "projections_total_normalized.mha", tmp_path / "geometry.xml", model, signals, (10.0, 12.0, 13.0), dimension=dim, spacing=sp)
    with pytest.raises(ValueError, match="resample the model"):
        recon.fdk_motion(proj.astype(np.float32), geo, (du, dv), (u0, v0), motion, signals, (12, 8, 11), sp)
