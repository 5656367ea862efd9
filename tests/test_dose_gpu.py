"""The dose tallies of the three transport kernels (tally_dose in csrc/track_common.inc, flushed in track_kernel.inc and
track_pool.inc), word for word wherever the arithmetic allows it.

An absorbed history leaves nothing on the detector: a history that a FAST scheduler drops, duplicates or mis-trades after its
absorption is invisible to every image test, and the dose tally is its only witness.  So, beside COMPAT against the oracle bit for
bit (every volume kind, all 22 materials, ROIs on a face of the volume, one voxel thick, a single voxel, either tally alone), the
FAST kernels are held to exact integer statements -- the voxel tally sums to the material tally, a sub-ROI is a crop, the tallies
do not move the image, no scheduling knob moves a word, launches add up -- and to the oracle statistically, with the variances
both sides tally (parity.dose_z; the CPU half of that statement is in tests/test_dose.py).
"""
import numpy as np
import pytest

import cases
import oracle_lib as ol
import parity
import warp_ref
from parity import DOSE_STAT_CASES as STAT_CASES, WHOLE_ROI_INPUT as WHOLE, edge_rois, every_projection, single_voxel_roi, water_arrays

pytestmark = pytest.mark.gpu

INPUT_ROI = [8, 55, 4, 59, 16, 47]  # of _prepare's default ROI, 0-based
BOTH = dict(tally_material_dose=True, tally_voxel_dose=True)
COMPAT_CASES = ["slab_angles", "tissue22", "graded_u16", "graded_raw", "thorax64"]
FAST_MODES = ["fast", "fast64"]
N_FAST = 300_000


def to_input(roi):
    """0-based roi6 -> the input file's ((x0, x1), (y0, y1), (z0, z1)), 1-based."""
    return tuple((roi[2 * k] + 1, roi[2 * k + 1] + 1) for k in range(3))


def tallies(ctx, runs, mode, **kw):
    """Clear, run `runs` = [(projection, count, seed), ...] one after the other, read: (images, voxels, materials)."""
    ctx.dose_clear()
    images = []
    for p, n, seed in runs:
        img, _, done = ctx.run_projection(p, n, mode=mode, seed=seed, **kw)
        assert mode == "compat" or done == n
        images.append(img)
    return (images,) + ctx.dose_read()


def same(a, b):
    """Two (images, voxels, materials) results hold the same words (a tally that is off is None in both)."""
    return (len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
            and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a[1:], b[1:])))


def fast_runs(ctx, seed=11):
    """About N_FAST histories over every projection of the case (the tallies accumulate over the scan)."""
    k = ctx.num_projections
    return [(p, N_FAST // k + 17 * p, seed + p) for p in range(k)]


_whole = {}


def whole_volume_run(engine, case_dir, name, mode):
    """The FAST run of `name` with the whole volume as ROI and default knobs, shared by the tests below and left unchanged:
    (runs, (images, voxels, materials), voxel_mat_dens, num_voxels)."""
    if (name, mode) not in _whole:
        with engine.create(case_dir(name, dose_roi=WHOLE, **BOTH), device=0) as ctx:
            nvox = tuple(ctx.geti(f"num_voxels_{a}") for a in "xyz")
            assert ctx.dose_info() == (3, parity.whole_roi(nvox), nvox[::-1])
            runs = fast_runs(ctx)
            res = tallies(ctx, runs, mode)
            for a in list(res[0]) + [res[1], res[2]]:
                a.setflags(write=False)
            _whole[(name, mode)] = (runs, res, ctx.host_table("voxel_mat_dens", "<f4").copy(), nvox)
    return _whole[(name, mode)]


# ---- a. COMPAT against the oracle, bit for bit
@pytest.mark.parametrize("name", COMPAT_CASES)
def test_compat_dose_bit_exact_vs_oracle_at_roi_edges(engine, case_dir, name):
    nb, hpt = 64, 150
    whole = None
    for k in range(3):  # the whole volume; one voxel thick in z up to the +x face; the voxel with the largest deposit
        roi_in = WHOLE if k == 0 else to_input(edge_rois(nvox)[0] if k == 1 else single_voxel_roi(whole))
        with engine.create(case_dir(name, dose_roi=roi_in, **BOTH), device=0) as ctx:
            T = parity.tables_from_context(ctx)
            nvox = T.num_voxels
            flags, roi, shape = ctx.dose_info()
            assert flags == 3 and (roi == parity.whole_roi(nvox) if k == 0 else roi == parity.roi6(roi_in))
            runs = every_projection(ctx)
            got = tallies(ctx, [(p, nb, seed) for p, seed in runs], "compat", hpt=hpt)
            img_cpu, vox_cpu, mat_cpu = parity.oracle_dose(T, roi, runs, nb, hpt, ol.MATH_PORTABLE)
            assert got[1].shape == vox_cpu.shape == shape + (2,)
            for a, b in zip(got[0], img_cpu):
                assert np.array_equal(a.reshape(-1), b), (k, roi)
            assert np.array_equal(got[1], vox_cpu) and int(vox_cpu[..., 0].sum()) > 0, (k, roi)
            assert np.array_equal(got[2], mat_cpu) and int(mat_cpu[:, 0].sum()) > 0, (k, roi)
            if k == 0:
                whole = vox_cpu
                if name == "tissue22":
                    assert np.count_nonzero(mat_cpu[:, 0]) >= 20
            else:
                assert np.array_equal(got[1], parity.crop(whole, roi, parity.whole_roi(nvox))), (k, roi)


def test_compat_either_tally_alone(engine, case_dir):
    """Materials only and voxels only: dose_read gives None for the tally that is off, the other is its half of the both-on run
    (which the test above holds to the oracle), and the image does not move."""
    name, nb, hpt = "tissue22", 64, 150
    res = {}
    for flags, kw in ((3, BOTH), (1, dict(tally_material_dose=True, tally_voxel_dose=False)), (2, dict(tally_material_dose=False, tally_voxel_dose=True))):
        with engine.create(case_dir(name, dose_roi=WHOLE, **kw), device=0) as ctx:
            assert ctx.dose_info()[0] == flags
            res[flags] = tallies(ctx, [(p, nb, seed) for p, seed in every_projection(ctx)], "compat", hpt=hpt)
    assert res[1][1] is None and res[2][2] is None and int(res[3][1].sum()) > 0 and int(res[3][2].sum()) > 0
    assert same(res[1], (res[3][0], None, res[3][2]))
    assert same(res[2], (res[3][0], res[3][1], None))


# ---- b. FAST and fast64: exact integer statements
@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("name", ["tissue22", "thorax64", "slab_angles", "graded_u16"])
def test_fast_voxel_tally_sums_to_the_material_tally(engine, case_dir, name, mode):
    """Every deposit goes to the voxel it happened in and to that voxel's material (pinned on the oracle by tests/test_dose.py):
    voxel index and ROI strides, material_of_compact, the LDS accumulators and their flush have to agree integer for integer."""
    _, (_, vox, mat), vmd, nvox = whole_volume_run(engine, case_dir, name, mode)
    want = parity.voxel_sums_per_material(vox, vmd)
    assert np.array_equal(want, mat), np.flatnonzero((want != mat).any(axis=1))
    assert vox.sum(axis=(0, 1, 2), dtype=np.uint64).tolist() == mat.sum(axis=0, dtype=np.uint64).tolist() and int(mat[:, 0].sum()) > 0
    if name == "tissue22":
        assert np.count_nonzero(mat[:, 0]) >= 20


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("name", ["tissue22", "thorax64", "slab_angles", "graded_u16"])
def test_fast_sub_roi_is_a_crop_of_the_whole_volume_tally(engine, case_dir, name, mode):
    runs, whole, _, nvox = whole_volume_run(engine, case_dir, name, mode)
    for roi in edge_rois(nvox) + [single_voxel_roi(whole[1])]:
        with engine.create(case_dir(name, dose_roi=to_input(roi), **BOTH), device=0) as ctx:
            assert ctx.dose_info()[1] == roi
            got = tallies(ctx, runs, mode)
        assert int(got[1].sum()) > 0, roi
        assert same(got, (whole[0], parity.crop(whole[1], roi, parity.whole_roi(nvox)), whole[2])), roi


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("name", ["tissue22", "thorax64", "slab_angles"])
def test_fast_dose_tallies_do_not_move_the_image(engine, case_dir, name, mode):
    runs, whole, _, _ = whole_volume_run(engine, case_dir, name, mode)
    with engine.create(case_dir(name), device=0) as ctx:  # both tallies off
        assert ctx.dose_info()[0] == 0
        assert same(tallies(ctx, runs, mode), (whole[0], None, None))
    with engine.create(case_dir(name, dose_roi=WHOLE, tally_material_dose=True, tally_voxel_dose=False), device=0) as ctx:
        assert same(tallies(ctx, runs, mode), (whole[0], None, whole[2]))
    with engine.create(case_dir(name, dose_roi=WHOLE, tally_material_dose=False, tally_voxel_dose=True), device=0) as ctx:
        assert same(tallies(ctx, runs, mode), (whole[0], whole[1], None))


SCHEDULE_KNOBS = (
    [{"MCGPU_THRESH_COMPTON": "1", "MCGPU_THRESH_RAYLEIGH": "1", "MCGPU_THRESH_NEW": "1", "MCGPU_SWAP_BATCH": "1"},
     {"MCGPU_THRESH_COMPTON": "64", "MCGPU_THRESH_RAYLEIGH": "64", "MCGPU_THRESH_NEW": "64", "MCGPU_FLYABLE_LOW": "1", "MCGPU_SWAP_BATCH": "40"},
     {"MCGPU_THRESH_COMPTON": "7", "MCGPU_THRESH_NEW": "50", "MCGPU_FLYABLE_LOW": "40", "MCGPU_SWAP_BATCH": "3"}]
    + [{"MCGPU_SLOT_TRADE": str(t), "MCGPU_HOLD_Q": str(q)} for t in (0, 1, 2, 3) for q in (0, 6, 15)]
    + [{"MCGPU_SEGMENT_LOOP": s} for s in ("0", "1")]
    + [{"MCGPU_TALLY_STAGE": "0"}, {"MCGPU_TALLY_STAGE": "1"}, {"MCGPU_TALLY_STAGE": "1", "MCGPU_TALLY_STAGE_MAX_HISTORIES": "7001"}])


@pytest.mark.parametrize("sched", [0, 1])
@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("name", ["tissue22", "thorax64", "slab_angles"])
def test_fast_dose_is_independent_of_the_schedule(engine, case_dir, monkeypatch, name, mode, sched):
    """Both schedulers, the batching thresholds, slot trading and the segment-end rule, the segment loop, the staged detector tally
    and its sub-launches: image, voxel tally and material tally are the words of the default run."""
    runs, whole, _, _ = whole_volume_run(engine, case_dir, name, mode)
    monkeypatch.setenv("MCGPU_FAST_SCHED", str(sched))
    with engine.create(case_dir(name, dose_roi=WHOLE, **BOTH), device=0) as ctx:
        assert ctx.geti("fast_scheduler") == sched
        assert same(tallies(ctx, runs, mode), whole), "default knobs"
        for knobs in SCHEDULE_KNOBS:
            for k, v in knobs.items():
                monkeypatch.setenv(k, v)
            ctx.reload_env_knobs()
            if knobs.get("MCGPU_TALLY_STAGE") == "0":
                assert ctx.geti("tally_stage_bins") == 0
            got = tallies(ctx, runs, mode)
            for k in knobs:
                monkeypatch.delenv(k)
            assert same(got, whole), knobs
        ctx.reload_env_knobs()


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("name", ["tissue22", "thorax64", "slab_angles"])
def test_fast_dose_is_independent_of_the_brick_levels(engine, case_dir, monkeypatch, name, mode):
    """Without the exterior hop a lookup gives the same (material, density) whatever the two brick levels look like (see
    test_fast_image_is_independent_of_slot_trading_segment_rule_and_brick_levels): second level off / codes / records, three sizes
    of the first level."""
    runs, _, _, _ = whole_volume_run(engine, case_dir, name, mode)
    monkeypatch.setenv("MCGPU_NO_EXTERIOR", "1")
    ref, seen = None, set()
    for sub in ("0", "1", "records"):
        for max_bricks in (None, "300", "40"):
            monkeypatch.setenv("MCGPU_SUB_BRICKS", "1" if sub == "1" else "0")
            monkeypatch.setenv("MCGPU_TILE_RECORDS", "1" if sub == "records" else "0")
            if max_bricks:
                monkeypatch.setenv("MCGPU_MAX_BRICKS", max_bricks)
            else:
                monkeypatch.delenv("MCGPU_MAX_BRICKS", raising=False)
            with engine.create(case_dir(name, dose_roi=WHOLE, **BOTH), device=0) as ctx:
                assert ctx.geti("bricks_exterior") == 0
                seen.add((ctx.geti("brick_shift"), ctx.geti("tile_records"), ctx.geti("sub_bricks_mixed") > 0))
                got = tallies(ctx, runs, mode)
            ref = got if ref is None else ref
            assert same(got, ref) and int(got[1].sum()) > 0 and int(got[2].sum()) > 0, (sub, max_bricks)
    assert len(seen) > 1  # the knobs did change the lookup structures


@pytest.mark.parametrize("sched", [0, 1])
@pytest.mark.parametrize("mode", FAST_MODES)
def test_fast_dose_launches_add_up(engine, case_dir, monkeypatch, mode, sched):
    name = "thorax64"
    monkeypatch.setenv("MCGPU_FAST_SCHED", str(sched))
    inp = case_dir(name, dose_roi=WHOLE, **BOTH)

    def add(a, b):
        return ([x + y for x, y in zip(a[0], b[0])], a[1] + b[1], a[2] + b[2])

    with engine.create(inp, device=0) as ctx, engine.create(inp, device=0) as other:
        assert ctx.geti("fast_scheduler") == sched
        for first in (0, 2 ** 32 - 1000):
            whole = tallies(ctx, [(1, 1025, 5)], mode, first=first)
            head = tallies(ctx, [(1, 63, 5)], mode, first=first)
            tail = tallies(ctx, [(1, 962, 5)], mode, first=first + 63)
            assert int(whole[1].sum()) > 0 and int(head[2].sum()) > 0
            assert same(add(head, tail), whole), first
            assert same(add(head, tallies(other, [(1, 962, 5)], mode, first=first + 63)), whole), first  # split over two contexts
        # no history: no deposit
        none = tallies(ctx, [(1, 0, 5)], mode)
        assert not none[1].any() and not none[2].any() and not none[0][0].any()
        # two projections without a clear in between are the sum of two cleared runs; reading does not disturb the tallies
        a, b = tallies(ctx, [(0, 40_000, 8)], mode), tallies(ctx, [(1, 30_001, 9)], mode)
        both = tallies(ctx, [(0, 40_000, 8), (1, 30_001, 9)], mode)
        assert np.array_equal(both[1], a[1] + b[1]) and np.array_equal(both[2], a[2] + b[2]) and int(a[1].sum()) > 0 and int(b[1].sum()) > 0
        again = ctx.dose_read()
        assert np.array_equal(again[0], both[1]) and np.array_equal(again[1], both[2])
        ctx.dose_clear()
        vox0, mat0 = ctx.dose_read()
        assert not vox0.any() and not mat0.any()


# ---- c. FAST and fast64 against the oracle
@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("name", STAT_CASES)
def test_fast_dose_within_3_sigma_of_oracle(engine, case_dir, name, mode):
    """6e6 FAST histories against 4.5e5 of the libm oracle, whole volume, blocks of 4^3 voxels and the material rows, variances
    measured on both sides (parity.dose_z), the criteria of test_fast_kernel_within_3_sigma_of_oracle; two oracle samples meet
    them (tests/test_dose.py::test_two_oracle_samples_meet_the_dose_criteria), and a 2 % scale or a one-voxel shift does not.

    The Compton branch below the table cut-off (serve_compton: phase = PH_NEW without a second deposit) is reached too rarely to
    show here; it was compared with the oracle's statement by reading.  oracle/mcgpu_oracle.c, track_batch: after gcoa the energy
    lost is deposited (if above 0.001 eV), the new energy's table index is negative, and the loop ends -- the photon's remaining
    energy is deposited nowhere and nothing reaches the image.  serve_compton does the same: tally_dose of e_in - E, then PH_NEW."""
    n_gpu = 6_000_000
    with engine.create(case_dir(name, dose_roi=WHOLE, **BOTH), device=0) as ctx:
        vox_cpu, mat_cpu, n_cpu = parity.oracle_dose_sample(ctx, name, 42)
        _, vox, mat = tallies(ctx, [(ctx.num_projections - 1, n_gpu, 7)], mode)
    fig = parity.dose_figures(vox, mat, n_gpu, vox_cpu, mat_cpu, n_cpu)
    print(f"{name} {mode}: {fig}")
    assert parity.dose_criteria_missed(fig) == [], fig


# ---- the ROI across geometry changes (csrc/engine_geometry.cpp)
def _boxes():
    """Two geometries of one physical size (the source and the detector of an input file follow the size) and different voxel
    counts: 64^3 voxels of 4 mm, and 32 x 64 x 20 voxels with inserts."""
    g0 = cases.geometry.MCBoxGeometry(shape=(64, 64, 64), image_spacing=(4.0, 4.0, 4.0), material="h2o")
    g0.materials[20:40, 24:50, 20:44] = cases.materials.material_number("bone_050")
    g0.densities[20:40, 24:50, 20:44] = 1.4
    g1 = cases.geometry.MCBoxGeometry(shape=(32, 64, 20), image_spacing=(8.0, 4.0, 12.8), material="h2o")
    g1.materials[8:20, 20:50, 6:18] = cases.materials.material_number("bone_050")
    g1.densities[8:20, 20:50, 6:18] = 1.4
    g1.materials[22:30, 4:16, :] = cases.materials.material_number("lung")
    g1.densities[22:30, 4:16, :] = 0.3
    return g0, g1


def _prepare(g, out, roi=((9, 56), (5, 60), (17, 48))):
    kw = dict(n_projections=2, angle_between_projections=90.0, n_histories=60_000, dose_roi=roi, **BOTH, **cases.SMALL_DET)
    return cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), **kw).prepare_simulation(out)


def _fast_and_compat(ctx):
    return (tallies(ctx, [(1, 200_000, 4)], "fast"), tallies(ctx, [(0, 64, 5)], "compat", hpt=150))


def test_set_geometry_with_dose_equals_a_fresh_context(engine, tmp_path):
    """After a change to a volume of other voxel counts the ROI is the input's, clipped to the new volume, and the tallies restart
    from zero: a FAST and a COMPAT projection give the words of a fresh context on the new geometry's files with the same input
    ROI.  A refused change in between leaves ROI and tallies as they were."""
    g0, g1 = _boxes()
    f0, f1 = _prepare(g0, tmp_path / "g0"), _prepare(g1, tmp_path / "g1")
    with engine.create(f0, device=0) as dev, engine.create(f1, device=0) as ref:
        assert np.array_equal(dev.host_table("source_data"), ref.host_table("source_data"))
        assert dev.dose_info()[1] == INPUT_ROI
        before = _fast_and_compat(dev)  # leaves the COMPAT run's tallies on the device
        held = dev.dose_read()
        assert int(held[0].sum()) > 0 and int(held[1].sum()) > 0
        with pytest.raises(engine.EngineError) as e:
            dev.set_geometry_arrays(*water_arrays((6, 6, 6)))
        assert e.value.code == -2 and dev.dose_info()[1] == INPUT_ROI
        kept = dev.dose_read()
        assert np.array_equal(kept[0], held[0]) and np.array_equal(kept[1], held[1])
        after = _fast_and_compat(dev)
        assert same(after[0], before[0]) and same(after[1], before[1])
        dev.set_geometry(g1)
        assert dev.dose_info() == ref.dose_info() and dev.dose_info()[1] != INPUT_ROI
        assert np.array_equal(dev.host_table("voxel_mat_dens"), ref.host_table("voxel_mat_dens"))
        vox0, mat0 = dev.dose_read()
        assert not vox0.any() and not mat0.any() and vox0.shape == ref.dose_read()[0].shape
        got, want = _fast_and_compat(dev), _fast_and_compat(ref)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert all(int(r[1].sum()) > 0 and int(r[2].sum()) > 0 for r in want)
        dev.set_geometry(g0)  # and back: the input's ROI again
        assert dev.dose_info()[1] == INPUT_ROI
        again = _fast_and_compat(dev)
        assert same(again[0], before[0]) and same(again[1], before[1])


def test_warp_geometry_then_dose_clear_equals_a_fresh_context(engine, tmp_path):
    g = cases.geometry.MCBoxGeometry(shape=(24, 20, 16), image_spacing=(10.0, 10.0, 10.0), material="h2o")
    g.materials[6:14, 5:15, 4:12] = cases.materials.material_number("bone_050")
    g.densities[6:14, 5:15, 4:12] = 1.4
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32) for n in g.materials.shape], indexing="ij")
    field = np.stack([2.5 * np.sin(2.0 * y) + 0.5, 1.5 * x * z - 0.5, 3.0 * np.cos(1.5 * x) * (1 - z * z)]).astype(np.float32)
    air = cases.materials.material_number("air")
    wm, wd = warp_ref.warp_nearest(g.materials, g.densities, field, air, cases.materials.MATERIALS_125KEV["air"])
    assert (wm != g.materials).sum() > 100
    roi = ((3, 500), (2, 17), (5, 12))  # reaches the +x face
    base = _prepare(g, tmp_path / "base", roi)
    warped = _prepare(cases.geometry.MCGeometry(wm, wd, g.image_spacing), tmp_path / "warped", roi)
    with engine.create(base, device=0) as dev, engine.create(warped, device=0) as ref:
        unwarped = _fast_and_compat(dev)
        dev.warp_geometry(field, frame="geometry")  # the tallies belong to the caller: a warp keeps them, dose_clear starts over
        assert np.array_equal(dev.host_table("voxel_mat_dens"), ref.host_table("voxel_mat_dens")) and dev.dose_info() == ref.dose_info()
        got, want = _fast_and_compat(dev), _fast_and_compat(ref)
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert not same(got[0], unwarped[0]) and int(want[0][1].sum()) > 0 and int(want[1][2].sum()) > 0


def test_set_geometry_image_clips_the_inputs_roi_or_refuses(engine, tmp_path):
    """The second geometry-change site (mcgpu_set_geometry_image, volumes mapped on the device) keeps the same ROI rule."""
    def ct(nz, ny, nx):
        rng = np.random.default_rng(nz)
        return rng.integers(-1100, 900, size=(nz, ny, nx)).astype(np.int16), {"body": np.ones((nz, ny, nx), np.uint8)}

    with engine.create(_prepare(_boxes()[0], tmp_path / "g0"), device=0) as ctx:
        before = ctx.dose_info()
        assert before[1] == INPUT_ROI
        held = tallies(ctx, [(1, 100_000, 4)], "fast")
        with pytest.raises(engine.EngineError) as e:
            ctx.set_geometry_image(*ct(6, 6, 6), frame="engine", image_spacing=(4.0, 4.0, 4.0))
        assert e.value.code == -2 and "region-of-interest" in e.value.message and "is not valid" in e.value.message
        kept = ctx.dose_read()
        assert ctx.dose_info() == before and np.array_equal(kept[0], held[1]) and np.array_equal(kept[1], held[2]) and int(kept[0].sum()) > 0
        assert same(tallies(ctx, [(1, 100_000, 4)], "fast"), held)
        ctx.set_geometry_image(*ct(40, 30, 40), frame="engine", image_spacing=(4.0, 4.0, 4.0))
        assert ctx.dose_info() == (3, [8, 39, 4, 29, 16, 39], (24, 26, 32))
        vox0, mat0 = ctx.dose_read()
        assert vox0.shape == (24, 26, 32, 2) and not vox0.any() and not mat0.any()
        got = tallies(ctx, [(1, 100_000, 4)], "fast")
        assert int(got[1].sum()) > 0 and int(got[2].sum()) > 0
        ctx.set_geometry_image(*ct(70, 80, 90), frame="engine", image_spacing=(4.0, 4.0, 4.0))
        assert ctx.dose_info() == before  # the input's ROI again, not the clipped one
