"""Image resampling on the device (csrc/resample.hip; mcgpu_resample_volume, mcgpu_set_geometry_image_resampled): the kernels against
the numpy restatement `resample_ref` bit for bit, every voxel; `MCGeometry.from_image(image_spacing=..., engine_context=...)` on `.mha`
files against the host pipeline on the restatement's arrays; the device chain against the context the host route installs.

No tolerance anywhere but in the transposition test, whose bound is derived there.  Wall time of this file on one MI355X: 4 s."""
import numpy as np
import pytest

import cases
import resample_ref as ref

pytestmark = pytest.mark.gpu

geo = cases.geometry
recon = cases.pkg.reconstruction
KW = dict(n_projections=2, angle_between_projections=70.0, n_histories=200_000, **cases.SMALL_DET)
TABLES = ("voxel_mat_dens", "voxel_size", "density_max", "mfp_woodcock", "woodcock_coarse", "mfp_a", "mfp_b", "palette")
COUNTERS = ("palette_size", "volume_kind", "brick_shift", "brick_count", "bricks_mixed", "bricks_exterior", "sub_bricks_mixed", "tile_records",
            "tiles_in_mixed_bricks", "num_voxels_x", "num_voxels_y", "num_voxels_z", "num_materials_used")
CT = (0.9765625, 0.9765625, 2.5)  # a clinical CT's spacing
ONE = (1.0, 1.0, 1.0)

# (shape, spacing, new spacing, resampled shape, default value)
INPUTS = {
    "ct": ((23, 17, 9), CT, ONE, (22, 17, 22), -1000.0),
    "outside_and_ties": ((11, 7, 3), (2.0, 3.0, 2.5), ONE, (22, 21, 8), 1e6),   # the default clamps to 32767 / 255
    "downsampled": ((12, 15, 20), (1.0, 0.5, 0.7), (2.0, 1.25, 1.0), (6, 6, 14), -1000.0),
    "identity": ((13, 5, 4), CT, CT, (13, 5, 4), -1000.0),
    "several_workgroups": ((70, 65, 33), CT, ONE, (68, 63, 82), -1000.0),        # ragged tails on every axis
}


def _data(shape, dtype, seed=3):
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        return (rng.normal(size=shape) * 700.0).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, size=shape).astype(dtype)  # the full range: negative fractional results pin the truncation


def _base(tmp_path, files=None):
    g = geo.MCBoxGeometry(shape=(12, 10, 8), image_spacing=(20.0, 20.0, 20.0), material="h2o")
    return cases.simulation.MCSimulation(g, files or cases.material_files(), cases.spectrum_file(), **KW).prepare_simulation(tmp_path / "base")


@pytest.fixture(scope="module")
def ctx(engine, tmp_path_factory):
    """One context for the tests that only resample: resample_volume does not touch the context's state."""
    with engine.create(_base(tmp_path_factory.mktemp("resample")), device=0) as c:
        yield c


@pytest.mark.parametrize("interpolator", ["nearest", "linear"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_resample_volume_equals_the_restatement_bit_for_bit(ctx, name, interpolator):
    shape, spacing, new, out_shape, default = INPUTS[name]
    for dtype in ("uint8", "int16", "float32"):
        a = _data(shape, dtype)
        want = ref.resample_ref(a, spacing, new, interpolator, default)
        got = ctx.resample_volume(a, spacing, new, interpolator=interpolator, default_value=default)
        assert got.dtype == a.dtype == want.dtype and got.shape == want.shape == out_shape, dtype
        assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), (dtype, int(np.count_nonzero(got != want)))
        rep = ctx.last_resample_report
        assert rep["kernel_bytes"] == a.nbytes + want.nbytes and rep["ms_kernel"] > 0.0
        if name == "identity":
            assert got.tobytes() == a.tobytes()
    if name == "outside_and_ties":  # what the case is there for
        a = _data(shape, "int16")
        want = ref.resample_ref(a, spacing, new, interpolator, default)
        inside = np.ones(out_shape, bool)
        for k, (n, s, t) in enumerate(zip(shape, spacing, new)):
            inside &= np.expand_dims(ref.plan_axis(n, s, t)["inside"], tuple(j for j in range(3) if j != k))
        assert (~inside).any() and np.all(want[~inside] == 32767)
        if interpolator == "linear":
            raw = ref.resample_ref(a, spacing, new, "linear", default, raw=True)
            assert np.count_nonzero(inside & (raw < 0) & (raw != np.trunc(raw)) & (want == np.trunc(raw)) & (want != np.floor(raw))) > 100


def test_transposed_input_gives_the_transposed_result(ctx):
    """resample(a.transpose(2, 0, 1), permuted spacings) == resample(a).transpose(2, 0, 1): a mixed-up axis anywhere between Python and
    the kernel shows as a wrong shape or as differences of the size of the data.  Nearest neighbour and the integer types' inside tests
    are exact under the permutation.  The lerps run along the array's axes, so float32 'linear' results may differ in rounding: three
    lerps of values bounded by max|a|, each with a relative error of 2^-53, far below one float32 ulp of max|a|; after the cast the two
    results are therefore equal or neighbouring float32 values, i.e. within one ulp of max|a|."""
    shape, spacing, new = (23, 17, 9), CT, ONE
    perm = (2, 0, 1)
    for dtype, interpolator in (("uint8", "nearest"), ("int16", "nearest"), ("float32", "nearest"), ("float32", "linear")):
        a = _data(shape, dtype, seed=9)
        straight = ctx.resample_volume(a, spacing, new, interpolator=interpolator, default_value=-1000.0)
        turned = ctx.resample_volume(np.ascontiguousarray(a.transpose(perm)), [spacing[k] for k in perm], [new[k] for k in perm],
                                     interpolator=interpolator, default_value=-1000.0)
        assert turned.shape == tuple(straight.shape[k] for k in perm) and straight.shape == (22, 17, 22)
        if interpolator == "nearest":
            assert np.array_equal(turned, straight.transpose(perm)), (dtype, interpolator)
        else:
            ulp = np.spacing(np.float32(np.abs(a).max()))
            assert np.all(np.abs(turned.astype(np.float64) - straight.transpose(perm).astype(np.float64)) <= float(ulp))
            assert np.array_equal(turned, ref.resample_ref(a.transpose(perm), [spacing[k] for k in perm], [new[k] for k in perm], "linear", -1000.0))


def _patient(shape, dtype, seed):
    """Random HU around the mapping's thresholds and random masks of four segmentations."""
    rng = np.random.default_rng(seed)
    image = rng.integers(-1100, 900, size=shape).astype(np.int16)
    if dtype == "float32":
        image = image.astype(np.float32) + rng.random(shape).astype(np.float32)
    segs = {"body": (rng.random(shape) < 0.9).astype(np.uint8) * rng.integers(1, 4, size=shape).astype(np.uint8),
            "bone": (rng.random(shape) < 0.4).astype(np.uint8), "lung": (rng.random(shape) < 0.25).astype(np.uint8),
            "lung_vessel": (rng.random(shape) < 0.1).astype(np.uint8)}
    return image, segs


def _write(tmp_path, image, segs, spacing):
    element_type = "MET_FLOAT" if image.dtype == np.float32 else "MET_SHORT"
    recon.write_mha(tmp_path / "ct.mha", image.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0), element_type=element_type)
    paths = {}
    for name, seg in segs.items():
        paths[f"{name}_segmentation_filepath"] = recon.write_mha(tmp_path / f"{name}.mha", seg.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0),
                                                                 element_type="MET_UCHAR")
    return paths


def _execute(image, segs):
    return geo.MaterialMapperPipeline.create_default_pipeline(**{f"{k}_segmentation": v for k, v in segs.items()}).execute(image)


def _resampled_ref(image, segs, spacing, new):
    return (ref.resample_ref(image, spacing, new, "linear", -1000.0),
            {k: ref.resample_ref(v, spacing, new, "nearest", 0.0) for k, v in segs.items()})


class _StubSegmenter:
    """Records the image it is shown; predicts body everywhere and nothing else."""

    def __init__(self):
        self.seen = None

    def segment(self, image):
        self.seen = np.array(image, copy=True)
        prediction = np.zeros((cases.pkg.segmentation.N_LABELS,) + image.shape, dtype=np.uint8)
        return prediction, prediction.astype(np.float32)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_from_image_resamples_files_on_the_device(ctx, tmp_path, dtype):
    """`.mha` files at a CT's spacing -> `from_image(image_spacing=(1, 1, 1), engine_context=ctx)`: the host pipeline on the
    restatement's arrays, in the resampled shape, carrying the new spacing; a segmenter is shown the resampled image."""
    image, segs = _patient((23, 17, 9), dtype, seed=21)
    paths = _write(tmp_path, image, segs, CT)
    want_image, want_segs = _resampled_ref(image, segs, CT, ONE)
    m, d = _execute(want_image, want_segs)
    assert len(np.unique(m)) >= 6
    got = geo.MCGeometry.from_image(tmp_path / "ct.mha", image_spacing=ONE, engine_context=ctx, **paths)
    assert got.image_shape == (22, 17, 22) and got.image_spacing == ONE
    assert np.array_equal(got.materials, m) and np.array_equal(got.densities.view(np.uint32), d.view(np.uint32))
    loaded, spacing, loaded_segs = geo.load_image_and_segmentations(tmp_path / "ct.mha", image_spacing=ONE, engine_context=ctx,
                                                                    **{k[:-len("_segmentation_filepath")]: v for k, v in paths.items()})
    assert spacing == ONE and loaded.dtype == image.dtype and loaded.tobytes() == want_image.tobytes()
    assert sorted(loaded_segs) == sorted(segs) and all(np.array_equal(loaded_segs[k], want_segs[k]) for k in segs)
    stub = _StubSegmenter()
    seen = geo.MCGeometry.from_image(tmp_path / "ct.mha", segmenter=stub, image_spacing=ONE, engine_context=ctx,
                                     lung_segmentation_filepath=paths["lung_segmentation_filepath"])
    assert stub.seen.dtype == image.dtype and stub.seen.tobytes() == want_image.tobytes()
    body = np.ones(want_image.shape, np.uint8)  # the stub's prediction: background nowhere
    m2, d2 = _execute(want_image, {"body": body, **{k: np.zeros_like(body) for k in ("bone", "muscle", "fat", "liver", "stomach", "lung_vessel")},
                                   "lung": want_segs["lung"]})
    assert np.array_equal(seen.materials, m2) and np.array_equal(seen.densities, d2) and seen.image_spacing == ONE


def _same_context(a, b):
    for key in COUNTERS:
        assert a.geti(key) == b.geti(key), key
    for name in TABLES:
        assert np.array_equal(a.host_table(name), b.host_table(name)), name


def _same_tallies(a, b):
    for mode, count in (("fast", 100_000), ("compat", 4096)):
        x, _, nx = a.run_projection(1, count, mode=mode, seed=77, hpt=8)
        y, _, ny = b.run_projection(1, count, mode=mode, seed=77, hpt=8)
        assert nx == ny and x.sum() > 0 and np.array_equal(x, y), mode


def _to_engine(a):
    """[gx, gy, gz] of the MCGeometry frame -> [nz, ny, nx] of the engine's (rot90(k=3) in the x/y plane, x fastest)."""
    return np.ascontiguousarray(np.transpose(np.rot90(a, k=3, axes=(0, 1)), (2, 1, 0)))


def _from_engine(a):
    return np.ascontiguousarray(np.rot90(np.transpose(a, (2, 1, 0)), k=1, axes=(0, 1)))


BIG = tuple(10.0 * s for s in CT)   # the CT's ratios at ten times the size: the phantom fills the beam, so the tallies depend on it
TEN = (10.0, 10.0, 10.0)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_device_chain_installs_the_context_of_the_host_route(engine, tmp_path, dtype):
    """`set_geometry_from_image(image_spacing=...)` -- one call to mcgpu_set_geometry_image_resampled -- against
    `set_geometry(from_image(..., image_spacing=..., engine_context=ctx))`: grid, voxel size, tables, palette, brick counters and the
    tallies of a short FAST and a short COMPAT launch.  Then the entry point directly in the engine's frame, against the host route fed
    with the restatement's arrays of that frame (resampling does not commute with the frame's flip: the output grid is anchored at
    voxel 0)."""
    image, segs = _patient((23, 17, 9), dtype, seed=33)
    paths = _write(tmp_path, image, segs, BIG)
    with engine.create(_base(tmp_path), device=0) as dev, engine.create(_base(tmp_path), device=0) as host:
        want = geo.MCGeometry.from_image(tmp_path / "ct.mha", image_spacing=TEN, engine_context=host, **paths)
        assert want.image_shape == (22, 17, 22) and want.image_spacing == TEN
        host.set_geometry(want)
        rep = dev.set_geometry_from_image(tmp_path / "ct.mha", image_spacing=TEN, **paths)
        assert rep["unmapped"] == 0 and sum(rep["count"]) == 22 * 17 * 22
        assert dev.last_resample_report["kernel_bytes"] == (image.itemsize + 4) * (image.size + 22 * 17 * 22)
        assert (dev.geti("num_voxels_x"), dev.geti("num_voxels_y"), dev.geti("num_voxels_z")) == (17, 22, 22)
        _same_context(dev, host)
        _same_tallies(dev, host)
        # frame 1 through the entry point itself gives the same context again
        dev.set_geometry_image(np.zeros((4, 4, 4), np.int16), {"body": np.ones((4, 4, 4), np.uint8)})
        dev.set_geometry_image_resampled(image, segs, BIG, TEN, frame="geometry")
        _same_context(dev, host)
        # frame 0
        image_e, segs_e = _to_engine(image), {k: _to_engine(v) for k, v in segs.items()}
        big_e, ten_e = (BIG[2], BIG[0], BIG[1]), (10.0, 10.0, 10.0)   # [nz][ny][nx] = [gz][gx reversed][gy]
        want_image, want_segs = _resampled_ref(image_e, segs_e, big_e, ten_e)
        m, d = _execute(want_image, want_segs)
        host.set_geometry(geo.MCGeometry(_from_engine(m), _from_engine(d), TEN))
        dev.set_geometry_image_resampled(image_e, segs_e, big_e, ten_e, frame="engine")
        assert (dev.geti("num_voxels_x"), dev.geti("num_voxels_y"), dev.geti("num_voxels_z")) == (17, 22, 22)
        _same_context(dev, host)
        _same_tallies(dev, host)


def test_a_refused_chain_call_leaves_the_context_as_it_was(engine, tmp_path):
    """A class whose material has no data file (-2, after the resampling and the mapping ran), an unmapped volume (-2) and a bad spacing
    (-1, before any device call): the context still launches and gives its earlier tallies; a call that succeeds then changes them."""
    image, segs = _patient((23, 17, 9), "int16", seed=41)
    files = cases.material_files()[:cases.materials.material_number("blood") - 1]  # the input names no file for blood and beyond
    with engine.create(_base(tmp_path, files), device=0) as ctx:
        before = {name: ctx.host_table(name) for name in TABLES}
        tally, _, _ = ctx.run_projection(0, 100_000, mode="fast", seed=3)
        with pytest.raises(engine.EngineError) as e:
            ctx.set_geometry_image_resampled(image, segs, BIG, TEN)  # bone -> bone_020 ..., lung vessels -> blood
        assert e.value.code == -2 and "no data file" in e.value.message
        no_body = {k: v for k, v in segs.items() if k != "body"}
        _, want_segs = _resampled_ref(image, no_body, BIG, TEN)
        want_image = ref.resample_ref(image, BIG, TEN, "linear", -1000.0)
        unmapped = int(np.count_nonzero(geo.classify_image(want_image, want_segs) == geo.UNMAPPED_CLASS))
        with pytest.raises(engine.EngineError) as e:
            ctx.set_geometry_image_resampled(image, no_body, BIG, TEN)
        assert unmapped > 0 and e.value.code == -2 and f"mcgpu_set_geometry_image_resampled: {unmapped} voxels are unmapped" in e.value.message
        assert ctx.last_image_report["unmapped"] == unmapped
        for bad in ((1.0, float("nan"), 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, 1e4)):   # the last one rounds an axis to 0
            with pytest.raises(engine.EngineError) as e:
                ctx.set_geometry_image_resampled(image, segs, BIG, bad)
            assert e.value.code == -1, bad
        for name in TABLES:
            assert np.array_equal(ctx.host_table(name), before[name]), name
        again, _, _ = ctx.run_projection(0, 100_000, mode="fast", seed=3)
        assert np.array_equal(again, tally)
        ok = {k: v for k, v in segs.items() if k not in ("lung_vessel", "bone")}
        ctx.set_geometry_image_resampled(image, ok, BIG, TEN)
        assert ctx.geti("num_voxels_x") == 17 and ctx.geti("correspondence_dims") == 0
        after, _, _ = ctx.run_projection(0, 100_000, mode="fast", seed=3)
        assert after.sum() > 0 and not np.array_equal(after, tally)
