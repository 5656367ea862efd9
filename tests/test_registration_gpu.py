"""Demons registration on the device (csrc/registration.hip) against its restatement (tests/registration_ref.py): the
smoothing bit for bit against the restatement's float32 run, the other operators and the whole loop within 4 x the error of that float32
run against the float64 one (the project's rule for the two networks), the report's mean squared differences, the sphere recovery the
rule was chosen by, and CorrespondenceModel.build_default down to a warp of a resident geometry."""
import numpy as np
import pytest

import cases
import registration_ref as R
from fixed_sum_ref import grid_sum

pytestmark = pytest.mark.gpu

reg = cases.pkg.registration
CorrespondenceModel = cases.pkg.correspondence.CorrespondenceModel
RespiratorySignal = cases.pkg.respiratory.RespiratorySignal

# (17, 13, 11): odd everywhere; (70, 3, 5): the first axis spans three segments of the sliding window, the second is shorter than every
# radius; (1, 9, 130): a single plane, rows that span three tiles of the row pass
SHAPES = [(17, 13, 11), (70, 3, 5), (1, 9, 130)]
SIGMAS = [(1.25, 1.25, 1.25), (0.7, 2.0, 4.0), (0.0, 1.25, 0.0)]
ids = lambda v: "x".join(map(str, v))  # noqa: E731


def _inputs(shape, seed=0):
    """Two images, a mask with holes and a field whose taps leave the volume on every face (up to 6 voxels, every sign, plus the
    corners pushed outwards by 9)."""
    rng = np.random.default_rng(1000 * shape[0] + shape[2] + seed)
    fixed = rng.normal(size=shape).astype(np.float32)
    moving = rng.normal(size=shape).astype(np.float32)
    mask = (rng.uniform(size=shape) > 0.3).astype(np.uint8)
    u = rng.uniform(-6, 6, size=(3,) + shape).astype(np.float32)
    for axis in range(3):
        face = [slice(None)] * 3
        face[axis] = 0
        u[(axis,) + tuple(face)] = -9.0
        face[axis] = -1
        u[(axis,) + tuple(face)] = 9.0
    return fixed, moving, mask, u


def _within_four_times_the_float32_error(name, got, want64, want32):
    err, yard = np.abs(got.astype(np.float64) - want64).max(), np.abs(want32.astype(np.float64) - want64).max()
    print(f"{name}: max error {err:.3g}, float32 restatement {yard:.3g}, ratio {err / yard if yard else float(err > 0):.3g}, "
          f"equal to the float32 run: {np.array_equal(got, want32.astype(np.float32))}")
    assert err <= 4 * yard


@pytest.mark.parametrize("sigma", SIGMAS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_smooth_equals_the_float32_restatement_bit_for_bit(engine, shape, sigma):
    u = _inputs(shape)[3]
    got, report = reg.register_stage("smooth", field=u, sigma=sigma)
    want = R.smooth(u, sigma, np.float32)
    assert want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert report["peak_device_bytes"] >= 2 * u.nbytes
    if any(sigma):
        assert np.abs(got - u).max() > 0.1


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_resize_stages(engine, shape):
    """To the shapes of the next two levels and to a larger shape (the field's way up): nearest exactly, linear within the bound."""
    fixed, moving, mask, _ = _inputs(shape)
    for out_shape in (R.level_shape(shape, 1), R.level_shape(shape, 2), tuple(2 * n - (n > 1) for n in shape), shape):
        got, _ = reg.register_stage("resize_nearest", fixed_mask=mask, out_shape=out_shape)
        assert got.dtype == np.uint8 and np.array_equal(got, R.resize_nearest(mask, out_shape))
        got, _ = reg.register_stage("resize_linear", moving=moving, out_shape=out_shape)
        _within_four_times_the_float32_error(f"resize_linear {shape} -> {out_shape}", got, R.resize_linear(moving, out_shape), R.resize_linear(moving, out_shape, np.float32))
    assert np.array_equal(reg.register_stage("resize_linear", moving=moving, out_shape=shape)[0], moving)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_warp_and_force_stages(engine, shape):
    fixed, moving, mask, u = _inputs(shape)
    got, _ = reg.register_stage("warp_linear", moving=moving, field=u)
    _within_four_times_the_float32_error(f"warp_linear {shape}", got, R.warp(moving, u), R.warp(moving, u, np.float32))
    for m in (None, mask):
        got, _ = reg.register_stage("force_step", fixed=fixed, moving=moving, field=u, fixed_mask=m, tau=2.25)
        want64, want32 = R.force_step(fixed, moving, u, 2.25, m), R.force_step(fixed, moving, u, 2.25, m, np.float32)
        _within_four_times_the_float32_error(f"force_step {shape} mask {m is not None}", got, want64, want32)
        if m is not None:
            assert np.array_equal(got[:, m == 0], u[:, m == 0]) and np.abs(got[:, m != 0] - u[:, m != 0]).max() > 0.01


def _sphere_pair(shape, centre, shift, radius):
    moving = R.sphere(shape, centre, radius)
    fixed = R.sphere(shape, (centre[0], centre[1], centre[2] - shift), radius)
    return fixed, moving


def _noisy_sphere_pair(shape, centre, radius):
    """A sphere shifted by 2 voxels along axis 2, the fixed image with noise of 0.02."""
    fixed, moving = _sphere_pair(shape, centre, 2, radius)
    return fixed + 0.02 * np.random.default_rng(8).normal(size=shape).astype(np.float32), moving


def _whole_loop_case():
    """(24, 20, 16), two levels, 10 iterations, masked."""
    shape = (24, 20, 16)
    fixed, moving = _noisy_sphere_pair(shape, (12, 10, 9), 5.0)
    mask = np.ones(shape, dtype=np.uint8)
    mask[:3] = 0
    return fixed, moving, dict(fixed_mask=mask, iterations=10, tau=2.25, sigma=(1.25, 1.25, 1.25), n_levels=2)


def _sum_order_case():
    """(41, 40, 41): 67 240 voxels, 1 704 more than one sweep of the 256 x 256 reduce grid.  One level, one iteration."""
    fixed, moving = _noisy_sphere_pair((41, 40, 41), (20, 20, 21), 8.0)
    return fixed, moving, dict(iterations=1, tau=2.25, sigma=(1.25, 1.25, 1.25), n_levels=1)


def test_whole_loop(engine):
    """(24, 20, 16), two levels, 10 iterations, masked: the field against the float64 restatement, two calls, the report."""
    fixed, moving, kw = _whole_loop_case()
    shape = fixed.shape
    got, report = reg.register(fixed, moving, return_differences=True, **kw)
    again, report2 = reg.register(fixed, moving, **kw)
    assert got.dtype == np.float32 and got.shape == (3,) + shape and got.tobytes() == again.tobytes()
    assert report["msd_before"] == report2["msd_before"] and report["msd_after"] == report2["msd_after"]
    want64, ref64 = R.register(fixed, moving, **kw)
    want32, _ = R.register(fixed, moving, dtype=np.float32, **kw)
    assert np.abs(want64[2]).max() > 1.0
    _within_four_times_the_float32_error("whole loop", got, want64, want32)
    # the mean squared differences: float64 numpy over the float32 differences the call returns
    assert len(report["differences"]) == 2
    for level, (before, after) in zip((1, 0), report["differences"]):
        assert before.shape == R.level_shape(shape, level)
        for name, d in (("msd_before", before), ("msd_after", after)):
            terms = d.astype(np.float64) ** 2
            assert abs(report[name][level] - terms.sum() / d.size) <= d.size * 2.0 ** -52 * terms.sum() / d.size
            assert report[name][level] == pytest.approx(ref64[name][level], rel=1e-2)
    assert report["msd_after"][0] < report["msd_before"][1] and report["ms_force"] > 0 and report["ms_smooth"] > 0 and report["peak_device_bytes"] > 8 * fixed.nbytes
    # identical images: exact zeros
    zero, report = reg.register(fixed, fixed, **kw)
    assert not zero.any() and report["msd_after"] == [0.0, 0.0]


def test_msd_is_the_sum_in_the_order_of_the_reduce_grid(engine):
    """The report's mean squared differences are the float32 differences the call returns, squared and added in float64 in the order
    of csrc/fixed_sum.inc: some threads of the grid add a second voxel."""
    fixed, moving, kw = _sum_order_case()
    shape = fixed.shape
    _, report = reg.register(fixed, moving, return_differences=True, **kw)
    (before, after), = report["differences"]
    for name, d in (("msd_before", before), ("msd_after", after)):
        assert d.dtype == np.float32 and d.shape == shape
        terms = d.astype(np.float64).ravel() ** 2
        print(f"{name}: {report[name][0]!r}, in the grid's order {grid_sum(terms, 256) / d.size!r}, numpy's {float(terms.sum()) / d.size!r}")
        assert report[name][0] == grid_sum(terms, 256) / d.size
    assert report["msd_after"][0] < report["msd_before"][0]


def test_sphere_recovery_on_the_device(engine):
    """The s = 4 case of tests/test_registration.py: the same two caps, and a residual at most 1.1 x the float64 restatement's."""
    shape, s = (40, 36, 32), 4
    fixed, moving = _sphere_pair(shape, (20, 18, 16), s, 7.0)
    kw = dict(iterations=50, tau=2.25, sigma=(1.25, 1.25, 1.25), n_levels=3)
    u, report = reg.register(fixed, moving, **kw)
    _, ref = R.register(fixed, moving, **kw)
    initial = R.msd(fixed, moving, np.zeros((3,) + shape))
    ratio, mean_uz = report["msd_after"][0] / initial, float(u[2][fixed > 0.5].mean())
    print(f"sphere recovery on the device, s = {s}: residual ratio {ratio:.5f} (restatement {ref['msd_after'][0] / initial:.5f}), mean u_z {mean_uz:.4f}")
    assert ratio <= 0.05 and abs(mean_uz - s) <= 0.3
    assert report["msd_after"][0] <= 1.1 * ref["msd_after"][0]


def test_build_default_on_the_device(engine, tmp_path):
    """Five phases of a sphere that follows a cos^4 curve, signals [5, 2], reference phase 2, on the context of a (24, 20, 16) box."""
    g = cases.geometry.MCBoxGeometry(shape=(24, 20, 16), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[6:14, 5:15, 4:12] = cases.materials.material_number("bone_050")
    g.densities[6:14, 5:15, 4:12] = 1.4
    inp = cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), n_projections=2, angle_between_projections=70.0, n_histories=200_000,
                                        **cases.SMALL_DET).prepare_simulation(tmp_path / "box")
    shape = g.materials.shape
    curve = RespiratorySignal.create_cos4(total_seconds=5.0, period=5.0, sampling_frequency=1.0)
    signals = np.stack([curve.signal, curve.dt_signal], axis=1)
    assert signals.shape == (5, 2)
    images = np.stack([R.sphere(shape, (12, 10, 9 - 2.0 * a), 5.0) for a in curve.signal])
    kw = dict(iterations=10, n_levels=2)
    with engine.create(inp, device=0) as ctx:
        model = CorrespondenceModel.build_default(images, signals=signals, reference_phase=2, ctx=ctx, **kw)
        assert ctx.geti("correspondence_dims") == 2 and ctx._correspondence_model is model
        fields = np.stack([reg.register(images[t], images[2], **kw)[0] for t in range(5)])
        assert not fields[2].any() and np.abs(fields[0][2]).max() > 1.0
        want = CorrespondenceModel().fit(fields, signals, reference_phase=2, ctx=ctx)
        assert np.array_equal(model.mean_vector_field.view(np.uint32), want.mean_vector_field.view(np.uint32))
        assert np.array_equal(model.coefficients.view(np.uint64), want.coefficients.view(np.uint64)) and model.model_hash == want.model_hash
        assert model.spatial_shape == shape and model.reference_phase == 2
        base = ctx.host_table("voxel_mat_dens").copy()
        ctx.set_correspondence_model(model)
        ctx.warp_geometry_by_signal(signals[0])
        warped = ctx.host_table("voxel_mat_dens")
        assert warped.shape == base.shape and base.size >= int(np.prod(shape)) and np.count_nonzero(warped != base) > 0
