"""GPU tests of the noise of the ray-traced primary (csrc/primary_project.hip: MOMENT PLANES, THE NOISE RULE) against the float64
restatement tests/primary_noise_ref.py (itself held to closed forms and to its own statistics by tests/test_primary_noise.py):
the moment kernel per moment, M_2 against the squared-weight tally of the engine's own Monte Carlo, the samplers pixel by pixel on
given planes, their statistics on constant planes, the noisy scan's repeatability and mean, the noisy hybrid products, refusals.

Tolerance of a moment plane against the restatement: the existing one of tests/test_primary_gpu.py, 4 x the largest relative error
of the restatement run with float32 accumulators, capped at 1e-4.  Every test prints its figures before it asserts."""
import ctypes as C
import hashlib
from pathlib import Path

import numpy as np
import pytest

import cases
import primary_noise_ref as nr
import primary_ref as pr

pytestmark = pytest.mark.gpu

SUBSAMPLES = [(1, 1), (2, 3)]
ENERGY_POINTS = (1, 2, 4)
HALF_FAN = 100


# ---- a: kernel = restatement, per moment -----------------------------------------------------------------------------------------
def moments_held_to_restatement(ctx, P, p, subsamples, label):
    ref = P.moment_planes(p, subsamples, ENERGY_POINTS, moments=(0, 1, 2))
    worst = 0.0
    for qn in ENERGY_POINTS:
        got, report = ctx.primary_moments(p, subsamples=subsamples, energy_points=qn)
        assert got.dtype == np.float32 and got.shape == (3,) + ref[(1, qn, "f64")].shape
        for k in (0, 1, 2):
            want, f32 = ref[(k, qn, "f64")], ref[(k, qn, "f32")]
            lit = want > 0
            err_f32 = float(np.max(np.abs(f32 - want)[lit] / want[lit]))
            tol = min(4.0 * err_f32, 1.0e-4)
            err = float(np.max(np.abs(got[k].astype(np.float64) - want)[lit] / want[lit]))
            print(f"{label} p{p} {subsamples} Qn {qn} M_{k}: kernel {err:.2e}, float32 restatement {err_f32:.2e}, tolerance {tol:.2e}, lit {int(lit.sum())}")
            assert np.all(got[k][~lit] == 0.0), (label, k)                        # outside the aperture: exactly 0
            assert err <= tol, (label, p, subsamples, qn, k, err, tol)
            worst = max(worst, err)
        plain, _ = ctx.primary_projection(p, subsamples=subsamples, energy_points=qn)
        assert got[1].tobytes() == plain.tobytes(), (label, qn)                   # plane 1 is primary_projection's, bit for bit
        crop = HALF_FAN if P.nx > HALF_FAN else P.nx // 2 + 1
        cropped, _ = ctx.primary_moments(p, subsamples=subsamples, energy_points=qn, crop_nx=crop)
        assert cropped.shape == (3, got.shape[1], crop) and cropped.tobytes() == np.ascontiguousarray(got[:, :, :crop]).tobytes()
        assert cropped[1].tobytes() == ctx.primary_projection(p, subsamples=subsamples, energy_points=qn, crop_nx=crop)[0].tobytes()
        assert report["n_energy_points"] == qn * int(np.count_nonzero(P.prob > 0))
    return worst


@pytest.mark.parametrize("subsamples", SUBSAMPLES, ids=["1x1", "2x3"])
@pytest.mark.parametrize("name", ["water", "slab_angles", "graded_u16", "graded_raw"])
def test_moment_kernel_equals_the_restatement(engine, case_dir, name, subsamples):
    with engine.create(case_dir(name), device=0) as ctx:
        P = nr.MomentPrimary(ctx)
        for p in (range(ctx.num_projections) if name == "slab_angles" else range(min(ctx.num_projections, 2))):
            moments_held_to_restatement(ctx, P, p, subsamples, name)
        scan, _ = ctx.primary_moments_scan(subsamples=subsamples)                  # a scan is its projections
        assert scan.shape[0] == ctx.num_projections and scan[-1].tobytes() == ctx.primary_moments(ctx.num_projections - 1, subsamples=subsamples)[0].tobytes()


@pytest.mark.parametrize("pixels,size", [((7, 5), (217.28, 155.2)), ((16, 16), (240.0, 240.0))], ids=["7x5", "16x16"])
def test_moment_kernel_on_small_detectors(engine, case_dir, pixels, size):
    with engine.create(case_dir("water", n_detector_pixels=pixels, detector_size=size), device=0) as ctx:
        P = nr.MomentPrimary(ctx)
        assert (P.nx, P.nz) == pixels
        for ss in SUBSAMPLES:
            moments_held_to_restatement(ctx, P, 0, ss, "water %dx%d" % pixels)


# ---- b: M_2 is what the engine tallies -------------------------------------------------------------------------------------------
_expect = {}


def w2_expectations(ctx, name, p, n):
    """The restatement's planes of one case, computed once and shared by the two modes."""
    if (name, p) not in _expect:
        _expect[(name, p)] = nr.w2_expectations(nr.MomentPrimary(ctx), p, n, (2, 2))
    return _expect[(name, p)]


@pytest.mark.parametrize("mode", ["fast", "fast64"])
@pytest.mark.parametrize("name,p", [("water", 0), ("slab_angles", 1)])
def test_second_moment_is_what_the_engine_tallies(engine, case_dir, name, p, mode):
    n = 100_000_000
    with engine.create(case_dir(name), device=0) as ctx:
        _, w2, _, done = ctx.run_projection_with_variance(p, n, mode=mode, seed=20261020)
        assert done == n
        mc = w2[0].astype(np.float64) * 1048576.0
        moments, _ = ctx.primary_moments(p, subsamples=(2, 2))
        tested = moments[2][::-1].astype(np.float64) * (n * ctx.pixel_area * 1.0e4)
        upper, lower, var, fine = w2_expectations(ctx, name, p, n)
        assert np.max(np.abs(tested - upper)) <= 1e-4 * upper.max()
        nr.w2_statement(mc, tested, upper, lower, var, fine, f"{name} p{p} {mode}")


# ---- c: sampler = restatement on given planes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", nr.SAMPLER_SHAPES, ids=["7x5", "16x16", "17x33"])
def test_sampler_equals_the_restatement(engine, shape):
    m0, m1, m2 = nr.sampler_inputs(shape)
    N, a = nr.SAMPLER_HISTORIES, nr.SAMPLER_AREA
    for seed, first in ((7, 5), (2 ** 63 + 11, 0)):
        want, count, ambiguous = nr.compound_poisson(m0, m1, m2, N, a, seed, first_projection=first)
        # the count alone: with M_1 = M_2 = M_0 the value is n / (N a)
        counted = engine.sample_compound_poisson(m0, m0, m0, N, a, seed, first_projection=first)
        got_count = counted.astype(np.float64) * (N * a)
        clear = ~ambiguous
        print(f"{shape} seed {seed}: pixels {m0.size}, ambiguous {int(ambiguous.sum())}, counts from {int(count.min())} to {int(count.max())}, "
              f"counts that differ {int(np.sum(np.abs(got_count - count)[clear] > 1e-3 * np.maximum(count[clear], 1.0)))}")
        assert ambiguous.sum() <= 0.001 * m0.size
        assert np.all(np.abs(got_count - count)[clear] <= 2.0 ** -23 * np.maximum(count[clear], 1.0))
        got = engine.sample_compound_poisson(m0, m1, m2, N, a, seed, first_projection=first)
        assert got.dtype == np.float32 and got.shape == m0.shape
        at_count, terms = nr.value_at_count(m0, m1, m2, N, a, seed, np.rint(got_count), first_projection=first)
        err = np.abs(got.astype(np.float64) - at_count)
        tol = nr.float32_tolerance(at_count, terms)
        print(f"   values: largest error {float(err.max()):.3e}, largest error / tolerance {float(np.max(err / tol)):.3f}, zeros {int(np.sum(got == 0))}")
        assert np.all(err <= tol)
        assert np.all(got[m0 == 0] == 0.0) and np.all(got[np.rint(got_count) == 0] == 0.0)
        assert np.array_equal(at_count[clear], want[clear])
        # the Gaussian sampler, with the clamp and a zero variance among the inputs
        mean = (m1.astype(np.float64) * np.where(np.arange(m1.size).reshape(m1.shape) % 5 == 0, -1.0, 1.0)).astype(np.float32)
        variance = (m2 / np.float32(N * a)).astype(np.float32)
        variance[:, ::2, ::3] = 0.0
        variance[:, 1::4, 1::2] *= np.float32(-1.0)                                # a negative variance reads as 0
        g = engine.sample_gaussian(mean, variance, seed, first_projection=first)
        g_want, g_terms = nr.gaussian(mean, variance, seed, first_projection=first)
        g_err = np.abs(g.astype(np.float64) - g_want)
        g_tol = nr.float32_tolerance(g_want, g_terms)
        print(f"   gaussian: largest error / tolerance {float(np.max(g_err / g_tol)):.3f}, clamped {int(np.sum(g == 0))}")
        assert np.all(g_err <= g_tol) and np.all(g[variance <= 0] == np.maximum(mean, 0)[variance <= 0]) and np.all(g >= 0)
        assert np.any(g == 0) and np.any(g > 0)


# ---- d: the statistical cases on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", nr.STAT_LAMBDAS)
def test_sampler_moments_on_constant_planes(engine, lam):
    m0, m1, m2, histories = nr.stat_case(lam)
    planes = [np.full((1,) + nr.STAT_SHAPE, v, dtype=np.float32) for v in (m0, m1, m2)]
    got = engine.sample_compound_poisson(*planes, histories, nr.STAT_AREA, seed=20261021)
    nr.sampler_statement(got, m0, m1, m2, histories, nr.STAT_AREA, f"device lambda {lam:g}")


# ---- e: the noisy scan -------------------------------------------------------------------------------------------------------------
def test_noisy_scan_is_seeded_and_splits_into_calls(engine, case_dir):
    with engine.create(case_dir("slab_angles"), device=0) as ctx:
        N = 2.0e6
        a, rep = ctx.primary_noisy_scan(N, seed=77)
        b, _ = ctx.primary_noisy_scan(N, seed=77)
        assert a.shape == (3, 96, 231) and a.dtype == np.float32 and rep["seed"] == 77 and rep["ms_sample"] > 0
        assert a.tobytes() == b.tobytes()                                          # the same seed gives the same bytes
        first, _ = ctx.primary_noisy_scan(N, seed=77, first_projection=0, n_projections=1)
        rest, _ = ctx.primary_noisy_scan(N, seed=77, first_projection=1, n_projections=2)
        assert np.concatenate([first, rest]).tobytes() == a.tobytes()              # two calls equal one call
        assert ctx.primary_noisy_projection(2, N, seed=77)[0].tobytes() == a[2].tobytes()
        other, _ = ctx.primary_noisy_scan(N, seed=78)
        differ = int(np.count_nonzero(other != a))
        drawn, rep2 = ctx.primary_noisy_scan(N)                                    # seed=None: one from os.urandom, reported
        print(f"pixels that differ between seeds 77 and 78: {differ} of {a.size}; drawn seed {rep2['seed']}")
        assert differ > 0.5 * np.count_nonzero(a) and drawn.tobytes() != a.tobytes()
        # the scan is the sampler on the moment planes: moments and sampler on the device, or the planes through the host
        moments, _ = ctx.primary_moments_scan()
        host = engine.sample_compound_poisson(moments[:, 0], moments[:, 1], moments[:, 2], N, ctx.pixel_area, 77)
        assert host.tobytes() == a.tobytes()
        cropped, _ = ctx.primary_noisy_scan(N, seed=77, crop_nx=HALF_FAN)
        assert cropped.shape == (3, 96, HALF_FAN) and cropped.tobytes() == np.ascontiguousarray(a[:, :, :HALF_FAN]).tobytes()
        assert np.all(a[moments[:, 0] == 0] == 0.0)


def test_mean_of_many_seeds_is_the_analytic_plane(engine, case_dir):
    with engine.create(case_dir("water"), device=0) as ctx:
        N, seeds = 1.0e6, 64
        moments, _ = ctx.primary_moments(0)
        m1 = moments[1].astype(np.float64)
        var = moments[2].astype(np.float64) / (N * ctx.pixel_area)                 # the rule's variance of one draw
        total = np.zeros_like(m1)
        for s in range(seeds):
            total += ctx.primary_noisy_projection(0, N, seed=1000 + s)[0]
        mean = total / seeds
        pull = abs(mean.sum() - m1.sum()) / np.sqrt(var.sum() / seeds)
        lit = m1 > 0
        z = (mean[lit] - m1[lit]) / np.sqrt(var[lit] / seeds)
        lam = N * ctx.pixel_area * moments[0][lit].astype(np.float64)
        print(f"water p0, {seeds} seeds at N = {N:g}: lambda {lam.min():.2f} .. {lam.max():.2f}, global pull {pull:.2f}, per-pixel z: mean {z.mean():.3f}, "
              f"std {z.std():.3f}, largest {np.abs(z).max():.2f}")
        assert pull <= 5.0
        assert np.all(mean[~lit] == 0.0)


# ---- f: the hybrid products --------------------------------------------------------------------------------------------------------
def sha256_of(folder):
    return {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(Path(folder).iterdir()) if f.is_file() and f.suffix == ".mha"}


def test_noisy_hybrid_products(engine, tmp_path):
    factory, kwargs = cases.CASES["catphan64_ct"]
    kwargs = dict(kwargs, n_histories=120_000)

    def simulate(folder, **extra):
        sim = cases.simulation.MCSimulation(factory(), cases.material_files(), cases.spectrum_file(), **kwargs)
        return sim.run_simulation(folder, engine, gpu_ids=(0,), run_air_simulation=True, air_n_histories=2_000_000, analytic_primary=True,
                                  scatter_sigma=(10, 10), **extra)
    simulate(tmp_path / "without", variance=True)
    N = 5.0e6
    report = simulate(tmp_path / "with", variance=True, hybrid_noise_histories=N, hybrid_noise_seed=99)
    without, with_noise = sha256_of(tmp_path / "without"), sha256_of(tmp_path / "with")
    new = {"projections_unscattered_analytic_noisy.mha", "projections_scattered_smoothed_noisy.mha", "projections_total_hybrid_noisy.mha",
           "projections_total_hybrid_noisy_normalized.mha"}
    print("files without:", sorted(without), "\nnew files:", sorted(set(with_noise) - set(without)))
    assert set(with_noise) == set(without) | new and "projections_total_hybrid.mha" in without
    assert all(with_noise[k] == without[k] for k in without)                      # every file of the run without keeps its bytes
    read = lambda name: engine.stack_read(tmp_path / "with" / name)
    primary, scatter, total = (read(f"projections_{n}.mha") for n in ("unscattered_analytic_noisy", "scattered_smoothed_noisy", "total_hybrid_noisy"))
    assert primary.shape == scatter.shape == total.shape == (4, 96, 231)
    assert total.tobytes() == (primary + scatter).tobytes()
    with engine.create(tmp_path / "with" / "input.in", device=0) as ctx:
        assert primary.tobytes() == ctx.primary_noisy_scan(N, seed=99)[0].tobytes()
    smoothed_var = engine.smooth_planes(read("projections_scattered_variance.mha"), (10, 10)) * np.float32(120_000 / N)
    assert scatter.tobytes() == engine.sample_gaussian(read("projections_scattered_smoothed.mha"), smoothed_var, 99).tobytes()
    analytic = read("projections_unscattered_analytic.mha")
    lit = analytic > 0
    ratio = float(primary[lit].sum() / analytic[lit].sum())
    print(f"noisy / analytic primary over the lit pixels: {ratio:.5f}; report seed {report.get('hybrid_noise_seed')}")
    assert abs(ratio - 1.0) < 0.01 and np.count_nonzero(primary != analytic) > 0.5 * lit.sum() and report["hybrid_noise_seed"] == 99
    engine.normalize_stack(tmp_path / "with" / "projections_total_hybrid_noisy.mha", tmp_path / "with" / "air" / "projections_total.mha",
                           tmp_path / "again.mha", sigma=(10, 10), spacing=cases.simulation.MCSimulation.STACK_PIXEL_SPACING)
    assert (tmp_path / "again.mha").read_bytes() == (tmp_path / "with" / "projections_total_hybrid_noisy_normalized.mha").read_bytes()
    sim = cases.simulation.MCSimulation(factory(), cases.material_files(), cases.spectrum_file(), **kwargs)
    with pytest.raises(ValueError, match="variance"):                              # the scatter's noise needs the variance stacks
        sim.run_simulation(tmp_path / "refused", engine, gpu_ids=(0,), analytic_primary=True, hybrid_noise_histories=N)
    assert not (tmp_path / "refused").exists() or not list((tmp_path / "refused").glob("*.mha"))


class _ShiftModel:
    """Stand-in correspondence model: a rigid shift proportional to the signal."""

    def __init__(self, shape):
        self.shape = shape

    def predict(self, x):
        u = np.zeros((3,) + tuple(self.shape), dtype=np.float32)
        u[2] = 3.4 * float(x[0])
        u[0] = 0.5 * float(x[1])
        return u


def test_4d_scan_writes_its_noisy_slices(engine, tmp_path):
    g = cases.geometry.MCBoxGeometry(shape=(24, 20, 16), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[6:14, 5:15, 4:12] = cases.materials.material_number("bone_050")
    g.densities[6:14, 5:15, 4:12] = 1.4
    R = cases.pkg.respiratory.RespiratorySignal
    signal = R.create_sin4(total_seconds=2.0, period=1.0, sampling_frequency=25.0)
    n, N = 8, 3.0e6

    def simulate(folder, **extra):
        sim = cases.simulation.MCSimulation4D(_ShiftModel(g.materials.shape), g, cases.material_files(), cases.spectrum_file(), n_histories=100_000,
                                              n_projections=n, frame_rate=15.0, angle_between_projections=30.0, **cases.SMALL_DET)
        return sim.run_simulation(signal, 3, folder, engine, mode="fast", analytic_primary=True, **extra)
    simulate(tmp_path / "analytic")
    rep = simulate(tmp_path / "noisy", hybrid_noise_histories=N, hybrid_noise_seed=5)
    before, after = sha256_of(tmp_path / "analytic"), sha256_of(tmp_path / "noisy")
    assert set(after) == set(before) | {"projections_unscattered_analytic_noisy.mha"} and all(after[k] == before[k] for k in before)
    analytic = engine.stack_read(tmp_path / "noisy" / "projections_unscattered_analytic.mha")
    noisy = engine.stack_read(tmp_path / "noisy" / "projections_unscattered_analytic_noisy.mha")
    lit = analytic > 0
    ratio = float(noisy[lit].sum() / analytic[lit].sum())
    distinct = len({noisy[i].tobytes() for i in range(n)})
    print(f"4-D: {rep['unique_states']} states, noisy / analytic {ratio:.5f}, distinct noisy slices {distinct} of {n}")
    assert noisy.shape == analytic.shape == (n, 96, 231) and rep["hybrid_noise_seed"] == 5 and rep["unique_states"] >= 2
    assert abs(ratio - 1.0) < 0.01 and distinct == n and np.all(noisy[~lit] == 0.0)
    assert np.count_nonzero(noisy != analytic) > 0.5 * lit.sum()


# ---- g: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(engine, case_dir):
    with engine.create(case_dir("slab_angles"), device=-1) as host_only:
        for call in (lambda: host_only.primary_moments(0), lambda: host_only.primary_noisy_projection(0, 1e6, seed=1)):
            with pytest.raises(engine.EngineError) as e:
                call()
            assert e.value.code == -1 and "device" in e.value.message
    with engine.create(case_dir("slab_angles"), device=0) as ctx:
        good, _ = ctx.primary_projection(2)
        bad = (dict(first_projection=3, n_projections=1), dict(first_projection=-1, n_projections=1), dict(first_projection=1, n_projections=3),
               dict(first_projection=0, n_projections=-2), dict(subsamples=(9, 1)), dict(subsamples=(1, -1)), dict(energy_points=5), dict(energy_points=-1))
        for kwargs in bad:
            for fn, call in (("mcgpu_primary_moments", lambda kw: ctx.primary_moments_scan(**kw)),
                             ("mcgpu_primary_noisy", lambda kw: ctx.primary_noisy_scan(1e6, 3, **kw))):
                with pytest.raises(engine.EngineError) as e:
                    call({"first_projection": 0, "n_projections": 1, **kwargs})
                assert e.value.code == -1 and fn in e.value.message, (fn, kwargs)
            assert ctx.primary_projection(2)[0].tobytes() == good.tobytes()
        for histories in (0.0, -5.0, float("inf"), float("nan")):
            with pytest.raises(engine.EngineError) as e:
                ctx.primary_noisy_scan(histories, seed=3)
            assert e.value.code == -1 and "histories" in e.value.message, histories
        out = np.zeros((3, 96, 231), dtype=np.float32)
        o = engine.PrimaryNoisyOptions(C.sizeof(engine.PrimaryNoisyOptions), 0, 1, 1, 1, 2, 0, 0, 1e6, 3)
        assert ctx.lib.mcgpu_primary_noisy(ctx.h, C.byref(o), None, None) == -1                        # null planes
        assert ctx.lib.mcgpu_primary_moments(ctx.h, C.byref(engine.PrimaryOptions(C.sizeof(engine.PrimaryOptions), 0, 1, 1, 1, 2, 0)), None, None) == -1
        o.struct_size = 4                                                                               # does not reach the first field
        assert ctx.lib.mcgpu_primary_noisy(ctx.h, C.byref(o), out.ctypes.data, None) == -1 and not out.any()
        o.struct_size = C.sizeof(engine.PrimaryNoisyOptions) - 16                                       # a caller without `histories`: read as 0, refused
        assert ctx.lib.mcgpu_primary_noisy(ctx.h, C.byref(o), out.ctypes.data, None) == -1 and not out.any()
        assert ctx.primary_projection(2)[0].tobytes() == good.tobytes()
    # the samplers on host planes
    plane = np.ones((2, 5, 7), dtype=np.float32)
    lib = engine.load_library()
    p = plane.ctypes.data
    for args in ((0, p, p, p, p, 2, 5, 7, 0.0, 0.01, 1, 0), (0, p, p, p, p, 2, 5, 7, float("nan"), 0.01, 1, 0), (0, p, p, p, p, 2, 5, 7, 1e6, 0.0, 1, 0),
                 (0, p, p, p, p, 2, 5, 7, 1e6, float("inf"), 1, 0), (0, None, p, p, p, 2, 5, 7, 1e6, 0.01, 1, 0), (0, p, p, p, None, 2, 5, 7, 1e6, 0.01, 1, 0),
                 (0, p, p, p, p, 0, 5, 7, 1e6, 0.01, 1, 0), (0, p, p, p, p, 2, 0, 7, 1e6, 0.01, 1, 0), (0, p, p, p, p, 2, 5, 7, 1e6, 0.01, 1, -1),
                 (0, p, p, p, p, 2, 65536, 65536, 1e6, 0.01, 1, 0)):
        assert lib.mcgpu_sample_compound_poisson(*args) == -1, args
        assert b"mcgpu_sample_compound_poisson" in lib.mcgpu_last_error()
    for args in ((0, None, p, p, 2, 5, 7, 1, 0), (0, p, None, p, 2, 5, 7, 1, 0), (0, p, p, p, 70000, 5, 7, 1, 0), (0, p, p, p, 2, 5, -7, 1, 0)):
        assert lib.mcgpu_sample_gaussian(*args) == -1, args
    with pytest.raises(ValueError):
        engine.sample_compound_poisson(plane, plane[:1], plane, 1e6, 0.01, 1)      # shapes that do not agree
    with pytest.raises(ValueError):
        engine.sample_gaussian(plane, plane[:, :4], 1)
    assert np.all(plane == 1.0)
