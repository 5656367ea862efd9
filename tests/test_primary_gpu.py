"""GPU tests of the ray-traced primary (csrc/primary_project.hip): the kernel against the float64 restatement of its rule
(tests/primary_ref.py, itself held to closed forms and to the reference's Monte Carlo by tests/test_primary_law.py), on every volume
source, after geometry and pose changes, as the expectation of the engine's own Monte Carlo; the Gaussian of mcgpu_smooth_planes
against scipy; the hybrid products of MCSimulation.run_simulation; refusals; repeatability.

Tolerance of kernel against restatement, per case: 4 x the largest relative error of the restatement run with float32 accumulators
(and float32 exponent, exp and spectrum sum) against float64 on the same planes, capped at 1e-4 of the pixel value.  Measured on an
MI355X, largest relative error of the kernel / of the float32 restatement over the planes of a case at 1 x 1 sub-points: water
2.4e-7 / 3.1e-7, slab_angles 5.3e-7 / 5.1e-7, catphan64 3.9e-7 / 3.7e-7, graded_u16 2.4e-6 / 2.1e-6, graded_raw 2.2e-6 / 2.3e-6,
tissue22 7.3e-7 / 8.1e-7, thorax64 5.4e-7 / 5.7e-7, cirs76 5.2e-7 / 5.7e-7 (2 x 3 sub-points: about half of each; the table is in
profiles/primary_ab.md).  Every test prints its figures before it asserts."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

import cases
import primary_ref as pr

pytestmark = pytest.mark.gpu

CASES = ["water", "slab_angles", "catphan64", "graded_u16", "graded_raw", "tissue22", "thorax64", "cirs76"]
SUBSAMPLES = [(1, 1), (2, 3)]
ENERGY_POINTS = (1, 2, 4)
HALF_FAN = 100                    # a crop inside the lit columns of the test detector
VOLUME_KIND = {"water": 0, "slab_angles": 0, "catphan64": 0, "graded_u16": 1, "graded_raw": 2, "tissue22": 0, "thorax64": 0, "cirs76": 0}


def held_to_restatement(ctx, P, p, subsamples, label):
    """The kernel's planes of projection p at every Qn, full width and cropped, against the restatement; returns the figures."""
    ref = P.planes(p, subsamples, ENERGY_POINTS)
    worst_gpu = worst_f32 = 0.0
    for qn in ENERGY_POINTS:
        want, f32 = ref[(qn, "f64")], ref[(qn, "f32")]
        lit = want > 0
        err_f32 = float(np.max(np.abs(f32 - want)[lit] / want[lit]))
        tol = min(4.0 * err_f32, 1.0e-4)
        got, report = ctx.primary_projection(p, subsamples=subsamples, energy_points=qn)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.all(got[~lit] == 0.0), label                                   # outside the aperture: exactly 0
        err = float(np.max(np.abs(got.astype(np.float64) - want)[lit] / want[lit]))
        print(f"{label} p{p} {subsamples} Qn {qn}: kernel {err:.2e}, float32 restatement {err_f32:.2e}, tolerance {tol:.2e}, "
              f"lit {int(lit.sum())}, kernel {report['ms_kernel']:.3f} ms")
        assert err <= tol, (label, p, subsamples, qn, err, tol)
        assert report["n_energy_points"] == qn * int(np.count_nonzero(P.prob > 0)) and abs(report["solid_angle"] - P.pose(p)["omega"]) <= 1e-12
        crop = HALF_FAN if P.nx > HALF_FAN else P.nx // 2 + 1
        cropped, _ = ctx.primary_projection(p, subsamples=subsamples, energy_points=qn, crop_nx=crop)
        assert cropped.shape == (want.shape[0], crop) and cropped.tobytes() == np.ascontiguousarray(got[:, :crop]).tobytes()
        worst_gpu, worst_f32 = max(worst_gpu, err), max(worst_f32, err_f32)
    return worst_gpu, worst_f32


# ---- 1 + 2: kernel = restatement, on every volume source ---------------------------------------------------------------------
@pytest.mark.parametrize("subsamples", SUBSAMPLES, ids=["1x1", "2x3"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_restatement(engine, case_dir, name, subsamples):
    with engine.create(case_dir(name), device=0) as ctx:
        assert ctx.geti("volume_kind") == VOLUME_KIND[name]
        P = pr.Primary(ctx)
        poses = range(ctx.num_projections) if name == "slab_angles" else range(min(ctx.num_projections, 2))
        for p in poses:
            held_to_restatement(ctx, P, p, subsamples, name)
        if name == "tissue22":
            assert ctx.primary_projection(0)[1]["n_materials"] == 22


@pytest.mark.parametrize("pixels,size", [((7, 5), (217.28, 155.2)), ((16, 16), (240.0, 240.0))], ids=["7x5", "16x16"])
def test_small_detectors(engine, case_dir, pixels, size):
    """A detector smaller than one workgroup tile, and one that is exactly a tile."""
    with engine.create(case_dir("water", n_detector_pixels=pixels, detector_size=size), device=0) as ctx:
        P = pr.Primary(ctx)
        assert (P.nx, P.nz) == pixels
        for ss in SUBSAMPLES:
            held_to_restatement(ctx, P, 0, ss, "water %dx%d" % pixels)


def test_u16_palette_beyond_8192_entries(engine, tmp_path):
    """graded_u16 holds 3000 palette entries; this volume holds more than the 8192 the Joseph projector stages in LDS."""
    sim = cases.simulation.MCSimulation(cases._graded(20000)(), cases.material_files(), cases.spectrum_file(), n_projections=1, n_histories=1000,
                                        **cases.SMALL_DET)
    with engine.create(sim.prepare_simulation(tmp_path), device=0) as ctx:
        assert ctx.geti("volume_kind") == 1 and ctx.geti("palette_size") > 8192
        held_to_restatement(ctx, pr.Primary(ctx), 0, (1, 1), "graded 20000")


# ---- 3: follows the resident geometry ----------------------------------------------------------------------------------------
def test_follows_geometry_and_pose_changes(engine, case_dir):
    with engine.create(case_dir("slab_angles"), device=0) as ctx:
        P = pr.Primary(ctx)
        before, _ = ctx.primary_projection(1)
        nx, ny, nz = (int(v) for v in P.n)
        # a whole-voxel shift on the device: out[z, y, x] = in[z - 1, y, x + 2], air where that falls outside
        field = np.zeros((3, nz, ny, nx), dtype=np.float32)
        field[0], field[2] = 2.0, -1.0
        ctx.warp_geometry(field, frame="engine")
        mat = np.zeros_like(P.vox_material)                                       # material number - 1 of air is 0
        den = np.full(P.vox_density.shape, np.float32(0.0013), dtype=np.float32)
        mat[1:, :, :nx - 2], den[1:, :, :nx - 2] = P.vox_material[:-1, :, 2:], P.vox_density[:-1, :, 2:]
        W = pr.Primary(ctx)
        assert np.array_equal(W.vox_material, mat) and np.array_equal(W.vox_density, den)
        W.set_voxels(mat, den)
        warped, _ = ctx.primary_projection(1)
        assert np.count_nonzero(warped != before) > 1000
        held_to_restatement(ctx, W, 1, (1, 1), "after warp_geometry")
        # another volume from host arrays: other shape, spacing, materials
        rng = np.random.default_rng(5)
        n2, spacing = (20, 26, 18), (1.1, 0.9, 1.3)
        mat2 = rng.choice(np.array([1, 4, 9], dtype=np.uint8), size=(n2[2], n2[1], n2[0]))
        den2 = rng.choice(np.array([0.5, 1.0, 1.25, 1.75], dtype=np.float32), size=mat2.shape)
        ctx.set_geometry_arrays(n2, spacing, mat2, den2)
        A = pr.Primary(ctx)
        assert tuple(A.n) == n2 and np.array_equal(A.vox_material, mat2.astype(np.int64) - 1) and np.array_equal(A.vox_density, den2)
        for p in (0, 2):
            held_to_restatement(ctx, A, p, (2, 3), "after set_geometry_arrays")
        # other poses
        old = A.source["position"].copy()
        ctx.set_projection_angles([270.0, 33.0, 201.5])
        B = pr.Primary(ctx)
        assert np.array_equal(B.source["position"][0], old[0]) and not np.allclose(B.source["position"][1:], old[1:], atol=1.0)
        previous, _ = ctx.primary_projection(2)
        for p in (1, 2):
            held_to_restatement(ctx, B, p, (1, 1), "after set_projection_angles")
        assert np.count_nonzero(ctx.primary_projection(2)[0] != previous) == 0


# ---- 4: expectation of the engine's own Monte Carlo --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "fast64"])
@pytest.mark.parametrize("name,p", [("water", 0), ("slab_angles", 1)])
def test_plane_is_the_expectation_of_the_engine_monte_carlo(engine, case_dir, name, p, mode):
    n = 100_000_000
    with engine.create(case_dir(name), device=0) as ctx:
        P = pr.Primary(ctx)
        image, w2, _, done = ctx.run_projection_with_variance(p, n, mode=mode, seed=20261020)
        assert done == n
        mc = image[0].astype(np.float64)
        var = np.maximum(w2[0].astype(np.float64) * 1048576.0 - mc * mc / n, 0.0)
        scale = 100.0 * n / (ctx.getf("inv_pixel_size_x") * ctx.getf("inv_pixel_size_z"))
        tested, _ = ctx.primary_projection(p, subsamples=(2, 2))
        fine = P.plane(p, (8, 8), 2, flip=False) * scale                         # the exclusion mask comes from the restatement
        same = P.plane(p, (2, 2), 2, flip=False) * scale
        kernel = tested[::-1].astype(np.float64) * scale
        assert np.max(np.abs(kernel - same)) <= 1e-4 * same.max()
        pr.expectation_statement(mc, var, kernel, fine, f"{name} p{p} {mode}")


# ---- 5: the Gaussian ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 96, 231), (2, 5, 7)], ids=["96x231", "5x7"])
@pytest.mark.parametrize("sigma", [(10, 10), (0, 3), (2.5, 0)])
def test_smooth_planes_is_scipy_gaussian_filter(engine, shape, sigma):
    rng = np.random.default_rng(shape[1])
    planes = (rng.random(shape) ** 3 * 40.0).astype(np.float32)
    got = engine.smooth_planes(planes, sigma)
    assert got.dtype == np.float32 and got.shape == planes.shape
    for k in range(shape[0]):
        want = ndimage.gaussian_filter(planes[k], sigma=sigma, truncate=4.0, mode="reflect")
        err = float(np.max(np.abs(got[k].astype(np.float64) - want.astype(np.float64))))
        assert err <= 1e-6 * float(planes[k].max()), (k, err)
    assert engine.smooth_planes(planes, (0, 0)).tobytes() == planes.tobytes()      # a sigma of 0 passes a plane through bit for bit
    one_axis = engine.smooth_planes(planes, (0, 3))
    assert one_axis.shape == planes.shape and np.array_equal(engine.smooth_planes(one_axis, (0.0, 0.0)), one_axis)


# ---- 6: hybrid products and the plain flow -----------------------------------------------------------------------------------
def sha256_of(folder):
    return {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(Path(folder).iterdir()) if f.is_file() and f.suffix == ".mha"}


def test_hybrid_products_and_the_plain_flow(engine, tmp_path):
    factory, kwargs = cases.CASES["catphan64_ct"]
    kwargs = dict(kwargs, n_histories=120_000)              # the case's 60 000 would be read as a time budget in seconds (scan.cpp: below 95 000)

    def simulate(folder, **extra):
        sim = cases.simulation.MCSimulation(factory(), cases.material_files(), cases.spectrum_file(), **kwargs)
        sim.run_simulation(folder, engine, gpu_ids=(0,), run_air_simulation=True, air_n_histories=2_000_000, **extra)
        return sim
    simulate(tmp_path / "plain")
    simulate(tmp_path / "hybrid", analytic_primary=True, scatter_sigma=(10, 10))
    plain, hybrid = sha256_of(tmp_path / "plain"), sha256_of(tmp_path / "hybrid")
    new = {"projections_unscattered_analytic.mha", "projections_scattered_smoothed.mha", "projections_total_hybrid.mha",
           "projections_total_hybrid_normalized.mha"}
    assert set(plain) == {"projections_total.mha", "projections_unscattered.mha", "projections_scattered.mha", "projections_total_normalized.mha"}
    assert set(hybrid) == set(plain) | new
    assert all(hybrid[k] == plain[k] for k in plain)                              # the plain outputs do not change by a byte
    pinned = json.loads((cases.GOLDEN / "primary_plain_flow_sha256.json").read_text())   # the plain folder on the parent commit
    assert plain == pinned
    head = lambda f: f.read_bytes().split(b"ElementDataFile")[0]
    for name in new:
        assert head(tmp_path / "hybrid" / name) == head(tmp_path / "hybrid" / "projections_total.mha"), name
    read = lambda name: engine.stack_read(tmp_path / "hybrid" / name)
    analytic, smoothed, total = read("projections_unscattered_analytic.mha"), read("projections_scattered_smoothed.mha"), read("projections_total_hybrid.mha")
    assert analytic.shape == smoothed.shape == total.shape == (4, 96, 231)
    assert total.tobytes() == (analytic + smoothed).tobytes()
    assert smoothed.tobytes() == engine.smooth_planes(read("projections_scattered.mha"), (10, 10)).tobytes()
    with engine.create(tmp_path / "hybrid" / "input.in", device=0) as ctx:
        assert analytic.tobytes() == ctx.primary_scan()[0].tobytes()
    engine.normalize_stack(tmp_path / "hybrid" / "projections_total_hybrid.mha", tmp_path / "hybrid" / "air" / "projections_total.mha",
                           tmp_path / "again.mha", sigma=(10, 10), spacing=cases.simulation.MCSimulation.STACK_PIXEL_SPACING)
    assert (tmp_path / "again.mha").read_bytes() == (tmp_path / "hybrid" / "projections_total_hybrid_normalized.mha").read_bytes()
    # the analytic plane is what the Monte Carlo unscattered plane scatters around
    mc = read("projections_unscattered.mha")
    lit = analytic > 0
    assert abs(float(mc[lit].sum()) / float(analytic[lit].sum()) - 1.0) < 0.02


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(engine, case_dir):
    with engine.create(case_dir("slab_angles"), device=-1) as host_only:
        with pytest.raises(engine.EngineError) as e:
            host_only.primary_projection(0)
        assert e.value.code == -1 and "device" in e.value.message
    with engine.create(case_dir("slab_angles"), device=0) as ctx:
        good, _ = ctx.primary_projection(2)
        for kwargs in (dict(first_projection=3, n_projections=1), dict(first_projection=-1, n_projections=1), dict(first_projection=1, n_projections=3),
                       dict(first_projection=0, n_projections=-2), dict(subsamples=(9, 1)), dict(subsamples=(1, -1)), dict(subsamples=(1, 9)),
                       dict(energy_points=5), dict(energy_points=-1)):
            with pytest.raises(engine.EngineError) as e:
                ctx.primary_scan(**{"first_projection": 0, "n_projections": 1, **kwargs})
            assert e.value.code == -1 and "mcgpu_primary_project" in e.value.message, kwargs
            assert ctx.primary_projection(2)[0].tobytes() == good.tobytes()
        o = engine.PrimaryOptions(4, 0, 1, 1, 1, 2, 0)                            # a struct_size that does not reach the first field
        out = np.zeros((96, 231), dtype=np.float32)
        assert ctx.lib.mcgpu_primary_project(ctx.h, o, out.ctypes.data, None) == -1 and not out.any()
        # a caller compiled before `crop_nx` existed, and one that wants no report
        import ctypes as C
        o = engine.PrimaryOptions(C.sizeof(engine.PrimaryOptions) - 4, 2, 1, 1, 1, 2, 50)
        assert ctx.lib.mcgpu_primary_project(ctx.h, o, out.ctypes.data, None) == 0 and out.tobytes() == good.tobytes()
        image, _, _ = ctx.run_projection(0, 100_000)                              # the Monte Carlo still runs on the context
        assert image.sum() > 0


# ---- 8: repeatability --------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(engine, case_dir):
    with engine.create(case_dir("cirs76"), device=0) as ctx:
        a, _ = ctx.primary_scan(subsamples=(2, 2))
        b, _ = ctx.primary_scan(subsamples=(2, 2))
        assert a.shape == (3, 96, 231) and a.tobytes() == b.tobytes() and float(a.max()) > 0
        for p in range(3):
            assert ctx.primary_projection(p, subsamples=(2, 2))[0].tobytes() == a[p].tobytes()     # a scan is its projections


# ---- the 4-D driver ----------------------------------------------------------------------------------------------------------
class _ShiftModel:
    """Stand-in correspondence model: a rigid shift proportional to the signal, a smaller one to its derivative."""

    def __init__(self, shape):
        self.shape = shape

    def predict(self, x):
        u = np.zeros((3,) + tuple(self.shape), dtype=np.float32)
        u[2] = 3.4 * float(x[0])
        u[0] = 0.5 * float(x[1])
        return u


def test_4d_scan_writes_each_projections_analytic_slice_after_its_warp(engine, tmp_path):
    import warp_ref
    g = cases.geometry.MCBoxGeometry(shape=(24, 20, 16), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[6:14, 5:15, 4:12] = cases.materials.material_number("bone_050")
    g.densities[6:14, 5:15, 4:12] = 1.4
    mats, spc = cases.material_files(), cases.spectrum_file()
    R = cases.pkg.respiratory.RespiratorySignal
    model = _ShiftModel(g.materials.shape)
    signal = R.create_sin4(total_seconds=2.0, period=1.0, sampling_frequency=25.0)
    n = 8

    def simulate(folder, **extra):
        sim = cases.simulation.MCSimulation4D(model, g, mats, spc, n_histories=100_000, n_projections=n, frame_rate=15.0, angle_between_projections=30.0,
                                              **cases.SMALL_DET)
        return sim.run_simulation(signal, 3, folder, engine, mode="fast", **extra)
    simulate(tmp_path / "plain")
    rep = simulate(tmp_path / "analytic", analytic_primary=True)
    assert rep["projections"] == n and rep["unique_states"] >= 2
    plain, with_primary = sha256_of(tmp_path / "plain"), sha256_of(tmp_path / "analytic")
    assert set(with_primary) == set(plain) | {"projections_unscattered_analytic.mha"} and all(with_primary[k] == plain[k] for k in plain)
    got = engine.stack_read(tmp_path / "analytic" / "projections_unscattered_analytic.mha")
    assert got.shape == (n, 96, 231)
    sig = signal.resample(15.0)
    s, ds = R.quantize_signal(sig.signal[:n], 3), R.quantize_signal(sig.dt_signal[:n], 3)
    seen = 0
    for k, ((sv, dsv), idx) in enumerate(R.get_unique_signals(s, ds).items()):
        wm, wd = warp_ref.warp_nearest(g.materials, g.densities, model.predict(np.array([sv, dsv])), cases.materials.material_number("air"),
                                       cases.materials.MATERIALS_125KEV["air"])
        angles = [270.0 + i * 30.0 for i in idx]
        one = cases.simulation.MCSimulation(cases.geometry.MCGeometry(wm, wd, g.image_spacing), mats, spc, n_histories=1000,
                                            projection_angles=angles[0:1] + angles, angle_between_projections=30.0, **cases.SMALL_DET)
        with engine.create(one.prepare_simulation(tmp_path / f"state{k}"), device=0) as ctx:
            for j, i in enumerate(idx):
                assert got[i].tobytes() == ctx.primary_projection(j + 1)[0].tobytes(), (k, i)
                seen += 1
    assert seen == n and len({got[i].tobytes() for i in range(n)}) == n
