"""CT image + segmentations -> geometry on the device (csrc/image_map.hip; mcgpu_map_image, mcgpu_set_geometry_image).  The mapping is
compared bit for bit with the numpy pipeline (`geometry.MaterialMapperPipeline.execute`), the installed context with the one the host
route builds from the host-mapped arrays (`set_geometry`): tables, brick counters, palette, tallies and a later warp, without tolerance.

Wall time of this file on one MI355X: DESIGN.md section 1, row f8."""
import hashlib

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

geo = cases.geometry
synthetic_ct = cases.pkg.workloads.synthetic_ct
KW = dict(n_projections=2, angle_between_projections=70.0, n_histories=200_000, **cases.SMALL_DET)
TABLES = ("voxel_mat_dens", "density_max", "mfp_woodcock", "woodcock_coarse", "mfp_a", "mfp_b", "palette")
COUNTERS = ("palette_size", "volume_kind", "brick_shift", "brick_count", "bricks_mixed", "bricks_exterior", "sub_bricks_mixed", "tile_records",
            "tiles_in_mixed_bricks", "num_voxels_x", "num_voxels_y", "num_voxels_z", "num_materials_used")


def _random_case(shape, seed, bone_everywhere=False):
    """Random HU and random masks of every segmentation (the body covering most of the volume, its values 1..3: "> 0" is inside)."""
    rng = np.random.default_rng(seed)
    image = rng.integers(-1100, 900, size=shape).astype(np.int16)
    segs = {"body": (rng.random(shape) < 0.9).astype(np.uint8) * rng.integers(1, 4, size=shape).astype(np.uint8)}
    for name in geo.SEGMENTATION_NAMES[1:]:
        segs[name] = (rng.random(shape) < 0.25).astype(np.uint8)
    if bone_everywhere:  # the bone mask touches all six faces: a solid block with a few holes, dense HU in most of it
        segs["bone"] = (rng.random(shape) < 0.97).astype(np.uint8)
        image[rng.random(shape) < 0.8] = 500
        for name in ("lung", "liver", "stomach", "muscle", "fat", "lung_vessel"):
            segs[name] = (rng.random(shape) < 0.03).astype(np.uint8)
    return image, segs


def _case(name):
    if name == "thorax128_bone":
        return synthetic_ct(cases.CASES[name][0]())
    if name == "odd_box":        # no extent is a multiple of 4: every border tile of the index volume is padded
        return _random_case((22, 19, 13), 1)
    if name == "sliver":         # one voxel thick: every voxel lies on two faces of the volume
        return _random_case((1, 9, 11), 2)
    if name == "bone_to_all_faces":
        return _random_case((21, 18, 10), 3, bone_everywhere=True)
    raise KeyError(name)


def _as(image, dtype):
    """The int16 image, or a float32 one with fractional values, values exactly on the thresholds and NaNs."""
    if dtype == "int16":
        return image
    f = image.astype(np.float32) + np.float32(0.5)
    flat = f.reshape(-1)
    flat[::7] = np.float32(150.0)
    flat[3::11] = np.float32(300.0)
    flat[5::13] = np.float32(-900.0)
    flat[1::17] = np.nan
    return f


def _execute(image, segs):
    return geo.MaterialMapperPipeline.create_default_pipeline(**{f"{k}_segmentation": v for k, v in segs.items()}).execute(image)


def _to_engine(a):
    """[gx, gy, gz] of the MCGeometry frame -> [nz, ny, nx] of the engine's (rot90(k=3) in the x/y plane, x fastest)."""
    return np.ascontiguousarray(np.transpose(np.rot90(a, k=3, axes=(0, 1)), (2, 1, 0)))


def _base(tmp_path, files=None):
    g = geo.MCBoxGeometry(shape=(12, 10, 8), image_spacing=(20.0, 20.0, 20.0), material="h2o")
    return cases.simulation.MCSimulation(g, files or cases.material_files(), cases.spectrum_file(), **KW).prepare_simulation(tmp_path / "base")


def _same_context(a, b):
    for key in COUNTERS:
        assert a.geti(key) == b.geti(key), key
    for name in TABLES:
        assert np.array_equal(a.host_table(name), b.host_table(name)), name


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("case", ["thorax128_bone", "odd_box", "sliver", "bone_to_all_faces"])
def test_mapping_equals_the_numpy_pipeline_bit_for_bit(engine, tmp_path, case, dtype):
    """ctx.map_image == MaterialMapperPipeline.execute on the arrays of the geometry frame and on the same arrays in the engine's frame,
    and the volume set_geometry_image installs from either frame is the host-mapped one voxel by voxel (the tiled kernel, its LDS
    permutation, the padded border tiles and the bone halo across tile and block borders)."""
    image, segs = _case(case)
    image = _as(image, dtype)
    m, d = _execute(image, segs)
    assert len(np.unique(m)) >= 8
    host_mapped = geo.MCGeometry(m, d, (3.0, 4.0, 5.0))
    with engine.create(_base(tmp_path), device=0) as ctx, engine.create(_base(tmp_path), device=0) as host:
        gm, gd = ctx.map_image(image, segs)
        assert gm.dtype == np.uint8 and gd.dtype == np.float32 and gm.shape == image.shape
        assert np.array_equal(gm, m) and np.array_equal(gd.view(np.uint32), d.view(np.uint32))
        rep = ctx.last_image_report
        assert rep["unmapped"] == 0 and sum(rep["count"]) == image.size
        cls = geo.classify_image(image, segs)
        assert rep["count"] == list(np.bincount(cls.ravel(), minlength=12))
        assert rep["first"] == [int(np.flatnonzero(cls.ravel() == c)[0]) if (cls == c).any() else -1 for c in range(12)]
        image_e, segs_e = _to_engine(image), {k: _to_engine(v) for k, v in segs.items()}
        em, ed = ctx.map_image(image_e, segs_e)
        assert np.array_equal(em, _to_engine(m)) and np.array_equal(ed.view(np.uint32), _to_engine(d).view(np.uint32))
        host.set_geometry(host_mapped)
        want = host.host_table("voxel_mat_dens")
        ctx.set_geometry_image(image, segs, frame="geometry", image_spacing=(3.0, 4.0, 5.0))
        assert np.array_equal(ctx.host_table("voxel_mat_dens"), want)
        assert np.array_equal(ctx.host_table("voxel_size"), host.host_table("voxel_size"))
        ctx.set_geometry_image(image_e, segs_e, frame="engine", image_spacing=(0.4 * 10, 0.3 * 10, 0.5 * 10))
        assert np.array_equal(ctx.host_table("voxel_mat_dens"), want)
        assert np.array_equal(ctx.host_table("voxel_size"), host.host_table("voxel_size"))
        ecls = _to_engine(cls)
        rep = ctx.last_image_report  # first occurrences in the [z][y][x] scan of the engine's frame: what orders the palette
        assert rep["first"] == [int(np.flatnonzero(ecls.ravel() == c)[0]) if (ecls == c).any() else -1 for c in range(12)]


@pytest.mark.parametrize("case, frame", [("thorax128_bone", "geometry"), ("odd_box", "engine"), ("bone_to_all_faces", "geometry")])
def test_installed_context_equals_the_host_route(engine, tmp_path, case, frame):
    """set_geometry_image against set_geometry(host-mapped geometry): the same tables (voxels, density_max, Woodcock table and its
    coarse copy, cross sections), the same PALETTE in the same order (pinned directly: the order of the palette cannot change a tally,
    which depends on a voxel's (material, density) only), the same brick and tile counters, identical FAST and COMPAT tallies on two
    projections, and the same result of a later warp_geometry on top of it."""
    image, segs = _case(case)
    m, d = _execute(image, segs)
    spacing = (4.0, 4.0, 4.0) if case == "thorax128_bone" else (12.0, 10.0, 14.0)
    shape = image.shape
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32) for n in shape], indexing="ij")
    field = np.stack([2.5 * np.sin(2.0 * y) + 0.5, 1.5 * x * z - 0.5, 3.0 * np.cos(1.5 * x) * (1 - z * z)]).astype(np.float32)
    with engine.create(_base(tmp_path), device=0) as dev, engine.create(_base(tmp_path), device=0) as host:
        host.set_geometry(geo.MCGeometry(m, d, spacing))
        if frame == "geometry":
            dev.set_geometry_image(image, segs, frame="geometry", image_spacing=spacing)
        else:
            dev.set_geometry_image(_to_engine(image), {k: _to_engine(v) for k, v in segs.items()}, frame="engine",
                                   image_spacing=(spacing[1], spacing[0], spacing[2]))
        _same_context(dev, host)
        palette = dev.host_table("palette", "<f4").reshape(-1, 2)
        assert palette.shape[0] == dev.geti("palette_size") >= len(np.unique(m))
        # first-occurrence order of the [z][y][x] scan, air at 0.0013 last when no voxel holds it
        em, ed = _to_engine(m).ravel(), _to_engine(d).ravel()
        _, first = np.unique(em.astype(np.uint64) << np.uint64(32) | ed.view(np.uint32), return_index=True)
        assert np.array_equal(palette[:len(first), 0], ed[np.sort(first)])
        for p in range(2):
            for mode, count in (("fast", 150_000), ("compat", 4096)):
                a, _, na = dev.run_projection(p, count, mode=mode, seed=77, hpt=8)
                b, _, nb = host.run_projection(p, count, mode=mode, seed=77, hpt=8)
                assert na == nb and a.sum() > 0 and np.array_equal(a, b), (p, mode)
        dev.warp_geometry(field, frame="geometry")
        host.warp_geometry(field, frame="geometry")
        _same_context(dev, host)
        assert np.count_nonzero(dev.host_table("voxel_mat_dens").view("<f4").reshape(-1, 2)[:, 1] != _to_engine(d).ravel()) > 20
        a, _, _ = dev.run_projection(1, 150_000, mode="fast", seed=5)
        b, _, _ = host.run_projection(1, 150_000, mode="fast", seed=5)
        assert a.sum() > 0 and np.array_equal(a, b)


def test_errors_leave_the_context_as_it_was(engine, tmp_path):
    """Without a body segmentation the call fails with the number of unmapped voxels; a class whose material has no data file gives -2,
    as on the host route; after either the context still holds -- and simulates -- its previous geometry.  A correspondence model goes
    with a successful call only."""
    image, segs = _case("odd_box")
    no_body = {k: v for k, v in segs.items() if k != "body"}
    unmapped = int(np.count_nonzero(geo.classify_image(image, no_body) == geo.UNMAPPED_CLASS))
    assert unmapped > 0
    files = cases.material_files()[:cases.materials.material_number("blood") - 1]  # the input names no file for blood and beyond
    with engine.create(_base(tmp_path, files), device=0) as ctx:
        before = {name: ctx.host_table(name) for name in TABLES}
        tally, _, _ = ctx.run_projection(0, 100_000, mode="fast", seed=3)
        with pytest.raises(engine.EngineError) as e:
            ctx.set_geometry_image(image, no_body)
        assert e.value.code == -2 and f"{unmapped} voxels are unmapped" in e.value.message and "ERROR" in e.value.message
        assert ctx.last_image_report["unmapped"] == unmapped
        with pytest.raises(ValueError, match=f"^{unmapped} voxels are unmapped"):
            ctx.map_image(image, no_body)
        with pytest.raises(engine.EngineError) as e:
            ctx.set_geometry_image(image, segs)  # bone -> bone_020 ..., lung vessels -> blood
        assert e.value.code == -2 and "no data file" in e.value.message
        with pytest.raises(engine.EngineError) as e2:  # the host route says the same
            ctx.set_geometry(geo.MCGeometry(*_execute(image, segs), (10.0, 10.0, 10.0)))
        assert e2.value.code == -2 and e2.value.message == e.value.message
        for name in TABLES:
            assert np.array_equal(ctx.host_table(name), before[name]), name
        again, _, _ = ctx.run_projection(0, 100_000, mode="fast", seed=3)
        assert np.array_equal(again, tally)
        # blood and the three bone classes are denser than every material the input names a file for: without them every class has its file
        ok = {k: v for k, v in segs.items() if k not in ("lung_vessel", "bone")}
        ctx.set_geometry_image(image, ok, image_spacing=(10.0, 10.0, 10.0))
        assert ctx.geti("num_voxels_x") == image.shape[1] and ctx.geti("correspondence_dims") == 0
        after, _, _ = ctx.run_projection(0, 100_000, mode="fast", seed=3)
        assert after.sum() > 0 and not np.array_equal(after, tally)


def test_from_image_files_on_the_device(engine, tmp_path):
    """`.mha` files -> `MCGeometry.from_image(engine_context=...)` and `Context.set_geometry_from_image`: the arrays and the context of
    the host flow."""
    recon = cases.pkg.reconstruction
    image, segs = _case("odd_box")
    spacing = (6.0, 7.0, 8.0)
    recon.write_mha(tmp_path / "ct.mha", image.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0), element_type="MET_SHORT")
    paths = {}
    for name, seg in segs.items():
        paths[f"{name}_segmentation_filepath"] = recon.write_mha(tmp_path / f"{name}.mha", seg.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0), element_type="MET_UCHAR")
    want = geo.MCGeometry.from_image(tmp_path / "ct.mha", **paths)
    with engine.create(_base(tmp_path), device=0) as dev, engine.create(_base(tmp_path), device=0) as host:
        got = geo.MCGeometry.from_image(tmp_path / "ct.mha", engine_context=dev, **paths)
        assert np.array_equal(got.materials, want.materials) and np.array_equal(got.densities, want.densities) and got.image_spacing == spacing
        dev.set_geometry_from_image(tmp_path / "ct.mha", **paths)
        host.set_geometry(want)
        _same_context(dev, host)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_launch_shape_of_the_reference(engine, tmp_path):
    """One run at the reference's own size, 512 x 512 x 256 (the bone-textured thorax as a synthetic CT), in both frames: the installed
    volume by SHA-256 against the numpy result."""
    g = geo.MCThoraxLikeGeometry(bone_texture=True)
    image, segs = synthetic_ct(g)
    del g
    assert image.shape == (512, 512, 256)
    m, d = _execute(image, segs)
    md = np.empty((image.size, 2), dtype=np.float32)   # voxel_mat_dens: {material + 0.0001f, density as the voxel file prints it}
    md[:, 0] = _to_engine(m).ravel().astype(np.float32) + np.float32(0.0001)
    dq = {v: np.float32(f"{float(v):.6f}") for v in np.unique(d)}
    ed = _to_engine(d).ravel()
    md[:, 1] = ed
    for v, q in dq.items():
        if q != v:
            md[ed == v, 1] = q
    want = _sha(md)
    del md, ed
    with engine.create(_base(tmp_path), device=0) as ctx:
        gm, gd = ctx.map_image(image, segs)
        assert _sha(gm) == _sha(m) and _sha(gd) == _sha(d)
        del gm, gd
        rep = ctx.set_geometry_image(image, segs, frame="geometry")
        assert rep["unmapped"] == 0 and sum(rep["count"]) == image.size and min(rep["count"]) > 0
        assert _sha(ctx.host_table("voxel_mat_dens")) == want
        ctx.set_geometry_image(_to_engine(image), {k: _to_engine(v) for k, v in segs.items()}, frame="engine")
        assert _sha(ctx.host_table("voxel_mat_dens")) == want
        assert (ctx.geti("num_voxels_x"), ctx.geti("num_voxels_y"), ctx.geti("num_voxels_z")) == (512, 512, 256)
        tally, _, n = ctx.run_projection(0, 200_000, mode="fast", seed=9)
        assert n == 200_000 and tally.sum() > 0
