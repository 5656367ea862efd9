"""The correspondence model resident on the device (csrc/correspondence.hip, mcgpu_correspondence_*): predict, fused predict + warp,
fit, the 4-D driver on top of it.  Everything here is compared bit for bit with the numpy statement of the same arithmetic
(cbctmc_amd.correspondence) or with the route through a host field that was there before (mcgpu_warp_geometry)."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

CorrespondenceModel = cases.pkg.correspondence.CorrespondenceModel
KW = dict(n_projections=2, angle_between_projections=70.0, n_histories=200_000, **cases.SMALL_DET)


def _slab():
    g = cases.geometry.MCBoxGeometry(shape=(24, 20, 16), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[6:14, 5:15, 4:12] = cases.materials.material_number("bone_050")
    g.densities[6:14, 5:15, 4:12] = 1.4
    return g


def _odd_box():
    """No extent is a multiple of 4: every border tile of the index volume is padded."""
    g = cases.geometry.MCBoxGeometry(shape=(22, 19, 13), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[5:15, 4:12, 3:9] = cases.materials.material_number("bone_050")
    g.densities[5:15, 4:12, 3:9] = 1.4
    return g


def _geometry(case):
    return cases.CASES[case][0]() if case in cases.CASES else {"slab4d": _slab, "odd_box": _odd_box}[case]()


def _breathing(T):
    t = np.arange(T)
    return 0.5 + 0.5 * np.cos(2 * np.pi * t / T), -np.pi / T * np.sin(2 * np.pi * t / T)


def _random_model(shape, K, mean_dtype, seed):
    """A model with arbitrary arrays (predict does not care where they come from)."""
    rng = np.random.default_rng(seed)
    n = 3 * int(np.prod(shape))
    m = CorrespondenceModel()
    m.coefficients = rng.normal(scale=5.0, size=(n, K))
    m.mean_vector_field = rng.normal(scale=2.0, size=(n, 1)).astype(mean_dtype)
    m.mean_signal = rng.uniform(0.2, 0.6, size=(K, 1))
    m.timesteps, m.signal_n_dims, m.spatial_shape, m.reference_phase = 10, K, tuple(shape), 2
    m.signals = rng.uniform(0, 1, size=(K, 10))
    return m


def _warp_fields(shape, T=10):
    """Ten fields from the field formula of test_4d.py's device-warp test, scaled by the signal, plus a second smooth field
    scaled by the signal's derivative."""
    rng = np.random.default_rng(5)
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32) for n in shape], indexing="ij")
    F = np.stack([2.5 * np.sin(2.0 * y) + 0.5, 1.5 * x * z - 0.5, 3.0 * np.cos(1.5 * x) * (1 - z * z)]).astype(np.float32)
    F[:, ::7, ::5, ::3] += rng.uniform(-3, 3, size=F[:, ::7, ::5, ::3].shape).astype(np.float32)
    G = np.stack([4.0 * z * x, 3.0 * np.sin(3.0 * x + y), 2.0 * y * y - 1.0]).astype(np.float32)
    s, ds = _breathing(T)
    fields = np.stack([F * np.float32(2.0 * s[t]) + G * np.float32(ds[t]) for t in range(T)]).astype(np.float32)
    return fields, np.stack([s, ds], axis=1)


@pytest.mark.parametrize("case", ["cirs76", "odd_box"])
def test_device_predict_equals_the_numpy_statement(engine, case_dir, tmp_path, case):
    """ctx.predict_field(s) == model.predict_field32(s) bit for bit: float32 and float64 mean, K = 1, 2, 3 (and 4), on cirs76
    (77 x 75 x 38) and on a box with no extent a multiple of 4."""
    g = _geometry(case)
    inp = case_dir(case) if case in cases.CASES else cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), **KW).prepare_simulation(tmp_path / case)
    shape = g.materials.shape
    rng = np.random.default_rng(17)
    with engine.create(inp, device=0) as ctx:
        assert ctx.geti("correspondence_dims") == 0
        for K in (1, 2, 3, 4):
            for mean_dtype in (np.float32, np.float64):
                model = _random_model(shape, K, mean_dtype, seed=10 * K + (mean_dtype is np.float64))
                ctx.set_correspondence_model(model)
                assert ctx.geti("correspondence_dims") == K
                for s in (rng.uniform(-1, 2, size=K), model.mean_signal[:, 0]):
                    got, want = ctx.predict_field(s), model.predict_field32(s)
                    assert got.dtype == np.float32 and got.shape == (3,) + shape
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (K, mean_dtype)
                with pytest.raises(engine.EngineError) as e:
                    ctx.predict_field(np.zeros(K + 1))
                assert e.value.code == -1
        with pytest.raises(engine.EngineError) as e:  # five signal dimensions: the host route
            ctx.set_correspondence_model(_random_model(shape, 5, np.float32, seed=3))
        assert e.value.code == -5 and ctx.geti("correspondence_dims") == 0  # a failed upload leaves no model behind
        with pytest.raises(ValueError):
            ctx.set_correspondence_model(_random_model(shape[::-1], 2, np.float32, seed=3))


@pytest.mark.parametrize("case", ["cirs76", "slab4d", "thorax128_bone"])
def test_fused_predict_and_warp_equals_the_route_through_a_host_field(engine, tmp_path, case):
    """warp_geometry_by_signal(s) on one context against warp_geometry(model.predict_field32(s)) on another: the same voxels, Woodcock
    table, brick counters and COMPAT / FAST tallies, without tolerance (the field bits are equal by the predict test, and everything
    after the three components is the same code).  One element row sits on exact ties; the signals are mean_signal itself (field =
    mean), a state inside the fitted range and one far outside that pushes voxels out of the volume (default material)."""
    g = _geometry(case)
    mats, spc = cases.material_files(), cases.spectrum_file()
    shape = g.materials.shape
    fields, signals = _warp_fields(shape)
    model = CorrespondenceModel().fit(fields, signals)
    # ties along the first axis, for every signal: mean 0.5, coefficients 0 -> x + 0.5 exactly
    row = np.zeros((3,) + shape, dtype=bool)
    row[0, 1, :, :] = True
    model.coefficients[row.reshape(-1)] = 0.0
    model.mean_vector_field[row.reshape(-1)] = 0.5
    base = cases.simulation.MCSimulation(g, mats, spc, **KW).prepare_simulation(tmp_path / "base")
    air_density = np.float32(cases.materials.MATERIALS_125KEV["air"])
    with engine.create(base, device=0) as fused, engine.create(base, device=0) as host:
        fused.set_correspondence_model(model)
        base_voxels = fused.host_table("voxel_mat_dens").copy()
        n_air = []
        for s in (model.mean_signal[:, 0].copy(), np.array([0.85, 0.12]), np.array([6.0, -2.5])):
            field = model.predict_field32(s)
            assert np.all(field[0, 1] == np.float32(0.5))
            fused.warp_geometry_by_signal(s)
            host.warp_geometry(field, frame="geometry")
            assert fused.geti("warp_field_bytes") == 0 and host.geti("warp_field_bytes") == field.nbytes
            a, b = fused.host_table("voxel_mat_dens"), host.host_table("voxel_mat_dens")
            assert np.array_equal(a, b)
            assert np.count_nonzero(a.view("<f4") != base_voxels.view("<f4")) > 100
            n_air.append(int(np.count_nonzero(a.view("<f4") == air_density)))
            assert np.array_equal(fused.host_table("mfp_woodcock"), host.host_table("mfp_woodcock"))
            assert np.array_equal(fused.host_table("density_max"), host.host_table("density_max"))
            for key in ("bricks_mixed", "bricks_exterior", "sub_bricks_mixed", "brick_shift", "brick_count"):
                assert fused.geti(key) == host.geti(key), key
            for p in range(2):
                a, _, _ = fused.run_projection(p, 300, mode="compat", seed=5 + p, hpt=100)
                b, _, _ = host.run_projection(p, 300, mode="compat", seed=5 + p, hpt=100)
                assert np.array_equal(a, b) and a.sum() > 0
                a, _, _ = fused.run_projection(p, 400_000, mode="fast", seed=9)
                b, _, _ = host.run_projection(p, 400_000, mode="fast", seed=9)
                assert np.array_equal(a, b) and a.sum() > 0
        assert n_air[2] > n_air[1]  # the far signal samples from outside: the default (air at 0.0013) comes in


@pytest.mark.parametrize("T", [10, 3])
def test_device_fit_equals_the_host_fit(engine, case_dir, monkeypatch, T):
    """fit(..., ctx=ctx) == fit(...) bit for bit, mean and coefficients, with the fields passing through the device in several slabs
    (658 350 elements in slabs of 50 000: the last one is short), and the model is left resident."""
    monkeypatch.setenv("MCGPU_CORRESPONDENCE_SLAB", "50000")
    shape = cases.CASES["cirs76"][0]().materials.shape
    fields, signals = _warp_fields(shape, T=T)
    rng = np.random.default_rng(T)
    fields += rng.normal(scale=0.3, size=fields.shape).astype(np.float32)  # not exactly linear in the signal: the residual is fitted too
    on_host = CorrespondenceModel().fit(fields, signals)
    with engine.create(case_dir("cirs76"), device=0) as ctx:
        on_device = CorrespondenceModel().fit(fields, signals, ctx=ctx)
        assert on_device.mean_vector_field.dtype == np.float32 and on_device.coefficients.dtype == np.float64
        assert np.array_equal(on_device.mean_vector_field.view(np.uint32), on_host.mean_vector_field.view(np.uint32))
        assert np.array_equal(on_device.coefficients.view(np.uint64), on_host.coefficients.view(np.uint64))
        assert np.abs(on_host.coefficients).max() > 1.0
        assert np.array_equal(on_device.mean_signal, on_host.mean_signal) and on_device.model_hash == on_host.model_hash
        assert ctx.geti("correspondence_dims") == 2 and ctx._correspondence_model is on_device
        s = np.array([0.3, 0.1])
        assert np.array_equal(ctx.predict_field(s).view(np.uint32), on_host.predict_field32(s).view(np.uint32))
        # five signal dimensions: the device declines (-5) and fit takes the host route by itself
        wide = rng.uniform(0, 1, size=(T, 5))
        m5 = CorrespondenceModel().fit(fields, wide, ctx=ctx)
        assert np.array_equal(m5.coefficients, CorrespondenceModel().fit(fields, wide).coefficients) and ctx.geti("correspondence_dims") == 0


class _PredictOnly:
    """What MCSimulation4D took before: an object with nothing but predict."""

    def __init__(self, model):
        self._model = model

    def predict(self, signal):
        return self._model.predict(signal)


def test_4d_scan_with_a_resident_model_equals_the_scan_through_host_fields(engine, tmp_path, monkeypatch):
    """MCSimulation4D.run_simulation on the reduced CIRS scan of test_4d.py: with a CorrespondenceModel (uploaded once, every state a
    warp_geometry_by_signal) the three stacks are, byte for byte, those of a run with an object that exposes only predict (host
    predict + field upload per state)."""
    g = cases.CASES["cirs76"][0]()
    mats, spc = cases.material_files(), cases.spectrum_file()
    shape = g.materials.shape
    s, ds = _breathing(10)
    fields = np.zeros((10, 3) + shape, dtype=np.float32)
    for t in range(10):  # SI shift with the signal, a smaller AP shift with its derivative (input 4)
        fields[t, 2] = 3.4 * s[t]
        fields[t, 0] = 0.5 * ds[t]
    model = CorrespondenceModel().fit(fields, np.stack([s, ds], axis=1))
    calls = {"signal": 0, "field": 0, "upload": 0}
    for name, key in (("warp_geometry_by_signal", "signal"), ("warp_geometry", "field"), ("set_correspondence_model", "upload")):
        original = getattr(engine.Context, name)

        def counted(self, *a, _original=original, _key=key, **kw):
            calls[_key] += 1
            return _original(self, *a, **kw)

        monkeypatch.setattr(engine.Context, name, counted)
    R = cases.pkg.respiratory.RespiratorySignal
    signal = R.create_sin4(total_seconds=2.0, period=1.0, sampling_frequency=25.0)
    reports = {}
    for label, m in (("resident", model), ("host", _PredictOnly(model))):
        sim4d = cases.simulation.MCSimulation4D(m, g, mats, spc, n_histories=200_000, n_projections=12, frame_rate=15.0,
                                                angle_between_projections=30.0, **cases.SMALL_DET)
        reports[label] = sim4d.run_simulation(signal, 3, tmp_path / label, engine, mode="fast")
        if label == "resident":
            assert calls == {"signal": reports[label]["unique_states"], "field": 0, "upload": 1}
    assert reports["resident"] == reports["host"] and 2 <= reports["host"]["unique_states"] <= 9
    assert calls["field"] == reports["host"]["unique_states"] and calls["upload"] == 1
    for name in ("total", "unscattered", "scattered"):
        a, b = (tmp_path / "resident" / f"projections_{name}.mha").read_bytes(), (tmp_path / "host" / f"projections_{name}.mha").read_bytes()
        assert a == b and len(a) > 12 * 96 * 231 * 4, name
    total = engine.stack_read(tmp_path / "resident" / "projections_total.mha")
    assert total.shape == (12, 96, 231) and len({total[i].tobytes() for i in range(12)}) == 12


def test_a_state_change_copies_no_field_and_the_model_goes_with_its_context(engine, case_dir):
    """Residency.  What is checked: the engine counts the field bytes a geometry warp copies from the host (`warp_field_bytes`,
    set by the one hipMemcpy of the field in warp_resident_geometry) and reports whether the device buffer for such a field exists
    (`warp_field_buffer`).  After set_correspondence_model, warp_geometry_by_signal copies 0 field bytes and never allocates that
    buffer; the route through a host field copies 12 bytes per voxel.  What both routes still copy per state is the shared tail,
    independent of the field: the Woodcock table and the 4-bit brick codes up, 17 words and the brick classification down."""
    g = cases.CASES["cirs76"][0]()
    shape = g.materials.shape
    model = _random_model(shape, 2, np.float32, seed=1)
    model.coefficients *= 0.2
    s = np.array([0.5, 0.4])
    with engine.create(case_dir("cirs76"), device=0) as ctx:
        with pytest.raises(engine.EngineError) as e:  # nothing resident yet
            ctx.warp_geometry_by_signal(s)
        assert e.value.code == -5
        ctx.set_correspondence_model(model)
        for signal in (s, model.mean_signal[:, 0]):
            ctx.warp_geometry_by_signal(signal)
            assert ctx.geti("warp_field_bytes") == 0 and ctx.geti("warp_field_buffer") == 0
        with pytest.raises(engine.EngineError) as e:
            ctx.warp_geometry_by_signal(np.array([0.5]))
        assert e.value.code == -1
        with ctx.clone(0) as twin:  # a clone takes the warped voxels, not the model
            assert twin.geti("correspondence_dims") == 0
            assert np.array_equal(twin.host_table("voxel_mat_dens"), ctx.host_table("voxel_mat_dens"))
        ctx.warp_geometry(model.predict_field32(s), frame="geometry")
        assert ctx.geti("warp_field_bytes") == 12 * int(np.prod(shape)) and ctx.geti("warp_field_buffer") == 1
        assert ctx.geti("correspondence_dims") == 2  # the host route leaves the model where it is
        ctx.clear_correspondence_model()
        assert ctx.geti("correspondence_dims") == 0 and ctx._correspondence_model is None
        with pytest.raises(engine.EngineError) as e:
            ctx.warp_geometry_by_signal(s)
        assert e.value.code == -5
        ctx.clear_correspondence_model()  # nothing resident: still fine
        # a new device model (set_geometry) does not inherit the old one's correspondence model
        ctx.set_correspondence_model(model)
        ctx.set_geometry(g)
        assert ctx.geti("correspondence_dims") == 0 and ctx._correspondence_model is None
    with engine.create(case_dir("graded_u16"), device=0) as ctx:  # no palette volume: -5, the caller's host route
        shape = cases.CASES["graded_u16"][0]().materials.shape
        ctx.set_correspondence_model(_random_model(shape, 2, np.float32, seed=2))
        with pytest.raises(engine.EngineError) as e:
            ctx.warp_geometry_by_signal(s)
        assert e.value.code == -5


def test_a_refused_geometry_change_keeps_the_warp_base_and_the_model(engine, tmp_path):
    """A geometry change that is refused -- an image without body segmentation (unmapped voxels), arrays with a material the input
    names no data file for (the file's odd box; the context starts from the same box with muscle in place of the bone) -- leaves the resident model, the warp base and the Python context's record of the model where they were:
    the same warp and the same 100 000 FAST histories give the same tally word for word.  A change that succeeds takes the model
    with the superseded device model, on the device and in Python."""
    g, with_bone = _odd_box(), _odd_box()
    g.materials[g.materials == cases.materials.material_number("bone_050")] = cases.materials.material_number("muscle_tissue")
    shape = g.materials.shape
    files = cases.material_files()[:cases.materials.material_number("blood") - 1]  # the input names no file for blood and beyond: none for bone_050
    inp = cases.simulation.MCSimulation(g, files, cases.spectrum_file(), **KW).prepare_simulation(tmp_path / "odd_box")
    model = _random_model(shape, 1, np.float32, seed=4)
    model.coefficients *= 0.2
    s = np.array([0.5])
    rng = np.random.default_rng(6)
    image = rng.integers(-1100, 900, size=shape).astype(np.int16)
    no_body = {"bone": (rng.random(shape) < 0.25).astype(np.uint8)}
    with engine.create(inp, device=0) as ctx:
        ctx.set_correspondence_model(model)

        def warp_and_run():
            ctx.warp_geometry_by_signal(s)
            return ctx.run_projection(0, 100_000, mode="fast", seed=3)[0]

        tally = warp_and_run()
        assert tally.sum() > 0
        field_buffer = ctx.geti("warp_field_buffer")

        def refuse(change, *args):
            with pytest.raises(engine.EngineError) as e:
                change(*args)
            assert e.value.code == -2
            assert ctx.geti("correspondence_dims") == 1
            assert ctx.geti("warp_field_buffer") == field_buffer
            assert ctx._correspondence_model is model
            assert np.array_equal(warp_and_run(), tally)
            return e.value.message

        assert "voxels are unmapped" in refuse(ctx.set_geometry_image, image, no_body)
        assert "no data file" in refuse(ctx.set_geometry, with_bone)
        mats, dens, spacing_cm = g.mcgpu_arrays()
        ctx.set_geometry_arrays(mats.shape, spacing_cm, np.transpose(mats, (2, 1, 0)), np.transpose(dens, (2, 1, 0)))
        assert ctx.geti("correspondence_dims") == 0 and ctx._correspondence_model is None
        with pytest.raises(engine.EngineError) as e:
            ctx.warp_geometry_by_signal(s)
        assert e.value.code == -5
