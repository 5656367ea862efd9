"""Field inversion on the device (csrc/field_inverse.hip) against its restatement (tests/field_inverse_ref.py): one
step, the residual and the whole loop within 4 x the error of the restatement's float32 run against its float64 run (the project's
yardstick), the report's norms, the exact cases, determinism, and `CorrespondenceModel.build_pair` / `pair_residual` on the five-phase
fixture of tests/test_field_inverse.py."""
import numpy as np
import pytest

import cases
import field_inverse_ref as FI
import registration_ref as R
from fixed_sum_ref import grid_sum
from test_registration_gpu import _inputs, _within_four_times_the_float32_error

pytestmark = pytest.mark.gpu

reg = cases.pkg.registration
recon = cases.pkg.reconstruction
CorrespondenceModel = cases.pkg.correspondence.CorrespondenceModel

# (17, 13, 11): odd everywhere; (70, 3, 5): axes shorter than any displacement; (1, 9, 130): a single plane whose rows cross wave and
# 256-thread block edges
SHAPES = [(17, 13, 11), (70, 3, 5), (1, 9, 130)]
# (41, 40, 41): 67 240 voxels, 1 704 more than one sweep of the 256 x 256 reduce grid: some threads add a second voxel
SUM_SHAPES = SHAPES + [(41, 40, 41)]
ids = lambda v: "x".join(map(str, v))  # noqa: E731


def _fields(shape):
    """The wild field of test_registration_gpu (taps leave the volume on every face, the corners are pushed out by 9) and a random v_0
    in [-6, 6]."""
    u = _inputs(shape)[3]
    v0 = np.random.default_rng(7 + shape[0]).uniform(-6, 6, size=u.shape).astype(np.float32)
    return u, v0


@pytest.mark.parametrize("relaxation", [1.0, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_step(engine, shape, relaxation):
    u, v0 = _fields(shape)
    got, report = reg.invert_field(u, iterations=1, relaxation=relaxation, initial=v0)
    assert got.dtype == np.float32 and got.shape == u.shape and report["iterations"] == 1
    _within_four_times_the_float32_error(f"invert step {shape} relaxation {relaxation}", got, FI.step(u, v0, relaxation), FI.step(u, v0, relaxation, np.float32))
    assert np.abs(got - v0).max() > 1.0 and report["peak_device_bytes"] >= 3 * u.nbytes


@pytest.mark.parametrize("shape", SUM_SHAPES, ids=ids)
def test_residual_and_its_norms(engine, shape):
    u, v0 = _fields(shape)
    got, report = reg.composition_residual(u, v0)
    want64, want32 = FI.residual(u, v0), FI.residual(u, v0, np.float32)
    _within_four_times_the_float32_error(f"residual {shape}", got, want64, want32)
    yard = np.abs(want32.astype(np.float64) - want64).max()
    top, rms = FI.norms(want64)
    print(f"residual norms {shape}: max {report['residual_max']!r} (float64 {top!r}), rms {report['residual_rms']!r} (float64 {rms!r}), yardstick {yard:.3g}")
    assert abs(report["residual_max"] - top) <= 4 * yard and abs(report["residual_rms"] - rms) <= 4 * yard
    # the report is the norm of what was stored, exactly: the squares added in the order of csrc/fixed_sum.inc (voxel by voxel, the
    # components of a voxel in order), one division and one root
    assert report["residual_max"] == float(np.abs(got).max())
    in_order = grid_sum(got.reshape(3, -1).T.astype(np.float64) ** 2, 256)
    print(f"residual rms {shape}: sum in the grid's order {in_order!r}, numpy's {float((got.astype(np.float64) ** 2).sum())!r}")
    assert report["residual_rms"] == float(np.sqrt(in_order / (3 * got[0].size)))
    # the same norms come with an inversion's report, before its first step
    _, inversion = reg.invert_field(u, iterations=0, initial=v0)
    assert inversion["residual_max_before"] == report["residual_max"] and inversion["residual_rms_before"] == report["residual_rms"]


def test_exact_cases(engine):
    """A zero field and a translation, byte for byte, the clamped border included."""
    zero, report = reg.invert_field(np.zeros((3, 6, 5, 4), dtype=np.float32), iterations=7)
    assert zero.tobytes() == bytes(zero.nbytes) and report["residual_max_after"] == 0.0 and report["residual_rms_before"] == 0.0
    u = np.empty((3, 9, 8, 10), dtype=np.float32)
    u[0], u[1], u[2] = 1.0, -2.0, 3.0
    v, report = reg.invert_field(u, iterations=5, relaxation=1.0)
    assert v.tobytes() == (-u).tobytes() and report["residual_max_before"] == 3.0 and report["residual_max_after"] == 0.0 and report["residual_rms_after"] == 0.0
    # relaxation 0.5 halves the error per step, in exact binary fractions
    v, report = reg.invert_field(u, iterations=5, relaxation=0.5)
    assert v.tobytes() == (-u * np.float32(1 - 2.0 ** -5)).tobytes() and report["residual_max_after"] == 3.0 * 2.0 ** -5
    v, report = reg.invert_field(u, iterations=40, relaxation=0.5)
    assert v.tobytes() == (-u).tobytes() and report["residual_max_after"] == 0.0
    r, report = reg.composition_residual(u, u)
    assert r.tobytes() == (2 * u).tobytes() and report["residual_max"] == 6.0


@pytest.fixture(scope="module")
def demons_field():
    shape = (24, 20, 16)
    u, _ = R.register(R.sphere(shape, (12, 10, 7), 5.0), R.sphere(shape, (12, 10, 9), 5.0), iterations=60, n_levels=2)
    return u.astype(np.float32)


def test_whole_loop_on_the_demons_field(engine, demons_field):
    """The defaults (40 steps, relaxation 0.5) on the (24, 20, 16) demons field: the float64 restatement within the yardstick, a residual
    of at most 1e-3 voxel, two calls the same bytes, no steps the initial field."""
    u = demons_field
    got, report = reg.invert_field(u)
    again, report2 = reg.invert_field(u, tolerance=1e-3)
    assert got.tobytes() == again.tobytes() and all(report[k] == report2[k] for k in report if k.startswith("residual"))
    want64, ref64 = FI.invert(u)
    want32, _ = FI.invert(u, dtype=np.float32)
    _within_four_times_the_float32_error("whole loop", got, want64, want32)
    print(f"residual max before {report['residual_max_before']:.4g} after {report['residual_max_after']:.4g} (float64 {ref64['residual_max_after']:.4g}), "
          f"rms after {report['residual_rms_after']:.4g}")
    assert report["residual_max_after"] <= 1e-3 and report["residual_max_before"] == pytest.approx(ref64["residual_max_before"], rel=1e-5)
    assert report["iterations"] == 40 and report["ms_step"] > 0 and report["ms_reduce"] > 0 and report["peak_device_bytes"] >= 3 * u.nbytes
    # relaxation 1 stalls on this field, and the tolerance says so
    with pytest.raises(RuntimeError, match="did not converge"):
        reg.invert_field(u, relaxation=1.0, tolerance=0.05)
    # no steps: v_0 unchanged, the two reports equal
    same, report = reg.invert_field(u, iterations=0, initial=got)
    assert same.tobytes() == got.tobytes() and report["iterations"] == 0
    assert report["residual_max_before"] == report["residual_max_after"] and report["residual_rms_before"] == report["residual_rms_after"]
    # a warm start from the answer stays there
    warm, report = reg.invert_field(u, iterations=3, initial=got)
    assert np.abs(warm - got).max() < 1e-5 and report["residual_max_after"] <= 1e-3


def test_build_pair_on_the_device(engine, tmp_path):
    """The five-phase fixture on the context of a (24, 20, 16) box: the derived pair against from_reference with the independently
    registered inverse=True model (the criteria of tests/test_field_inverse.py), the inversion reports, the same-direction mistake,
    and the way into the reconstruction."""
    g = cases.geometry.MCBoxGeometry(shape=FI.PHASE_SHAPE, image_spacing=(10.0, 10.0, 10.0), material="h2o")
    inp = cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), n_projections=2, angle_between_projections=70.0, n_histories=200_000,
                                        **cases.SMALL_DET).prepare_simulation(tmp_path / "box")
    images, signals = FI.phase_images(), FI.PHASE_SIGNALS
    with engine.create(inp, device=0) as ctx:
        from_reference, to_reference = CorrespondenceModel.build_pair(images, signals=signals, reference_phase=2, ctx=ctx, **FI.PHASE_REGISTRATION)
        assert ctx._correspondence_model is from_reference and ctx.geti("correspondence_dims") == 2
    independent = CorrespondenceModel.build_default(images, signals=signals, reference_phase=2, inverse=True, **FI.PHASE_REGISTRATION)
    assert len(to_reference.inversion_reports) == 5 and all(r["residual_max_after"] <= 0.05 and r["iterations"] == 40 for r in to_reference.inversion_reports)
    ours = [from_reference.pair_residual(to_reference, s) for s in signals]
    theirs = [from_reference.pair_residual(independent, s) for s in signals]
    print("pair residual rms per state, derived: " + ", ".join(f"{r['rms']:.3f}" for r in ours) + "; independent: " + ", ".join(f"{r['rms']:.3f}" for r in theirs))
    assert np.mean([r["rms"] for r in ours]) <= 0.5 * np.mean([r["rms"] for r in theirs])
    assert all(a["rms"] < b["rms"] and a["rms"] <= a["max"] for a, b in zip(ours, theirs))
    # two models of one direction: about 2 |u| at an end state
    same = from_reference.pair_residual(from_reference, signals[0])
    assert same["max"] > 1.0 and same["rms"] > 1.0
    motion = recon.MotionModel.from_correspondence_model(to_reference, (10.0, 10.0, 10.0), dimension=(24, 16, 20), spacing=(10.0, 10.0, 10.0))
    assert motion.dimension == (24, 16, 20) and motion.n_signal_dims == 2
