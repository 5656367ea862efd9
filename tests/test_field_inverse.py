"""Field inversion without a GPU: the float64 restatement (tests/field_inverse_ref.py) on known answers and on the
demons field the defaults were chosen by, the plumbing of `CorrespondenceModel.inverted` / `build_pair` with the restatement in the place
of the device calls, the consistency of the derived pair against two independently registered models, every refusal of the C entry
points (the options are checked before the first device call), the Python layer's ValueErrors and the C layout of the ABI structs."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_layout
import cases
import field_inverse_ref as FI
import registration_ref as R

pkg = cases.pkg
reg = pkg.registration
CorrespondenceModel = pkg.correspondence.CorrespondenceModel


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_zero_field_gives_zeros(dtype):
    v, report = FI.invert(np.zeros((3, 6, 5, 4)), iterations=7, relaxation=0.5, dtype=dtype)
    assert v.dtype == dtype and v.shape == (3, 6, 5, 4) and not v.any()
    assert report["residual_max_before"] == 0.0 and report["residual_rms_after"] == 0.0 and report["residual_max_after"] == 0.0


def _translation(dtype=np.float64):
    u = np.empty((3, 9, 8, 10), dtype=dtype)
    u[0], u[1], u[2] = 1.0, -2.0, 3.0
    return u


@pytest.mark.parametrize("relaxation", [1.0, 0.5])
def test_a_translation_is_inverted_exactly(relaxation):
    """u = (1, -2, 3) on (9, 8, 10): v = (-1, 2, -3) everywhere, exactly, and a residual of exactly 0 -- also on the border, where the
    taps are clamped (a constant field reads the same value there).

    Relaxation 1 is there after the first step and stays there: checked after 5 steps.  Relaxation 0.5 cannot be there after 5 steps,
    by the rule itself: on a constant field a step is v <- v - w (v + u), which maps v = -(1 - e) u to -(1 - (1 - w) e) u, so from zero
    v = -(1 - 2^-k) u after k steps, all of it exact binary arithmetic.  (The expectation "exact after 5 steps" was written down for both
    relaxations and verified for 1 only.)  For 0.5 the test therefore holds the 5 steps to that closed form, exactly, (-0.96875, 1.9375,
    -2.90625) with residual_max 3 x 2^-5, and holds the end state to what was asked, exactly (-1, 2, -3) and a residual of exactly 0, once
    2^-k u has fallen below the last bit of u: after 80 steps in float64 (53 + 2 bits would do)."""
    u = _translation()
    v, report = FI.invert(u, iterations=5, relaxation=relaxation)
    print(f"relaxation {relaxation}: v = {v[:, 0, 0, 0]}, residual max after 5 steps {report['residual_max_after']}")
    assert report["residual_max_before"] == 3.0
    if relaxation == 0.5:
        assert np.array_equal(v, -(1 - 2.0 ** -5) * u) and report["residual_max_after"] == 3.0 * 2.0 ** -5
        v, report = FI.invert(u, iterations=80, relaxation=relaxation)
    assert np.array_equal(v, -u) and report["residual_max_after"] == 0.0 and report["residual_rms_after"] == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_relaxation_one_half_halves_the_error_of_a_translation_exactly(dtype):
    """v = -(1 - 2^-k) u after k steps, in exact binary fractions and on the clamped border too, until the step falls below the last
    bit: exactly -u with a residual of exactly 0 after 80 steps (float32: after 30)."""
    u = _translation(dtype)
    v, report = FI.invert(u, iterations=5, relaxation=0.5, dtype=dtype)
    assert v.dtype == dtype and np.array_equal(v, -u * dtype(1 - 2.0 ** -5)) and report["residual_max_after"] == 3.0 * 2.0 ** -5
    v, report = FI.invert(u, iterations=80, relaxation=0.5, dtype=dtype)
    assert np.array_equal(v, -u) and report["residual_max_after"] == 0.0 and report["residual_rms_after"] == 0.0
    v, report = FI.invert(u, iterations=5, relaxation=1.0, dtype=dtype)
    assert np.array_equal(v, -u) and report["residual_max_after"] == 0.0


@pytest.fixture(scope="module")
def demons_field():
    """The sphere pair of test_registration_gpu.py: fixed at z = 7, moving at z = 9, radius 5 on (24, 20, 16)."""
    shape = (24, 20, 16)
    u, _ = R.register(R.sphere(shape, (12, 10, 7), 5.0), R.sphere(shape, (12, 10, 9), 5.0), iterations=60, n_levels=2)
    return u


def test_the_defaults_invert_the_demons_field_and_relaxation_one_does_not(demons_field, capsys):
    """Finite differences of 1.69: relaxation 1 stalls (3.0 voxels), 0.5 reaches 1.4e-8 voxel in 40 steps in float64."""
    u = demons_field
    slope = max(float(np.abs(np.diff(u[i], axis=axis)).max()) for i in range(3) for axis in range(3))
    v, report = FI.invert(u, iterations=40, relaxation=0.5)
    _, stalled = FI.invert(u, iterations=40, relaxation=1.0)
    with capsys.disabled():
        print(f"\ndemons field: max |u| {np.abs(u).max():.3f}, largest finite difference {slope:.3f}; residual max after 40 steps: "
              f"relaxation 0.5: {report['residual_max_after']:.3g}, relaxation 1: {stalled['residual_max_after']:.3g}")
    assert slope > 1.0 and np.abs(u[2]).max() > 1.5
    assert report["residual_max_after"] < 1e-3 and report["residual_rms_after"] <= report["residual_max_after"] < report["residual_max_before"]
    assert stalled["residual_max_after"] > 1.0
    # what the inverse is for: the fixed image pulled by v gives the moving one about as well as u gives the fixed one
    shape = u.shape[1:]
    fixed, moving = R.sphere(shape, (12, 10, 7), 5.0), R.sphere(shape, (12, 10, 9), 5.0)
    assert R.msd(moving, fixed, v) < 0.1 * R.msd(moving, fixed, np.zeros_like(v))
    # the tolerance check of invert_field, on the reports of the restatement
    reg.check_residual(report, 0.05)
    reg.check_residual(stalled, None)
    with pytest.raises(RuntimeError, match="did not converge"):
        reg.check_residual(stalled, 0.05)
    with pytest.raises(RuntimeError, match="did not converge"):
        reg.check_residual(dict(stalled, residual_max_after=float("nan")), 0.05)


# ---------------------------------------------------------------------------------------------------------------- the models
def _restatement_as_register(fixed, moving, fixed_mask=None, gpu_id=0, **parameters):
    u, report = R.register(fixed, moving, fixed_mask=fixed_mask, **parameters)
    return u.astype(np.float32), report


@pytest.fixture(scope="module")
def models():
    """from_reference, the independently registered inverse=True model, and from_reference.inverted(), all from the restatements."""
    images = FI.phase_images()
    device_register = reg.register
    reg.register = _restatement_as_register
    try:
        from_reference = CorrespondenceModel.build_default(images, signals=FI.PHASE_SIGNALS, reference_phase=2, **FI.PHASE_REGISTRATION)
        independent = CorrespondenceModel.build_default(images, signals=FI.PHASE_SIGNALS, reference_phase=2, inverse=True, **FI.PHASE_REGISTRATION)
    finally:
        reg.register = device_register
    calls = []
    derived = from_reference.inverted(gpu_id=3, _invert=FI.as_invert_field(calls=calls))
    return from_reference, independent, derived, calls


def _pair_rms(a, b, signal):
    """The pair's residual as `pair_residual` defines it, from the float64 restatement."""
    return FI.norms(FI.residual(a.predict_field32(signal), b.predict_field32(signal)))[1]


def test_inverted_is_a_fit_to_the_inverses_of_the_predicted_fields(models):
    from_reference, _, derived, calls = models
    assert derived is not from_reference and derived.is_fitted and from_reference.inversion_reports is None
    assert calls == [dict(iterations=40, relaxation=0.5, gpu_id=3)] * 5 and len(derived.inversion_reports) == 5
    assert all(r["residual_max_after"] <= 0.05 and r["iterations"] == 40 for r in derived.inversion_reports)
    fields = np.stack([FI.invert(from_reference.predict_field32(s))[0].astype(np.float32) for s in FI.PHASE_SIGNALS])
    want = CorrespondenceModel().fit(fields, FI.PHASE_SIGNALS, reference_phase=2)
    assert np.array_equal(derived.mean_vector_field, want.mean_vector_field) and np.array_equal(derived.coefficients, want.coefficients)
    assert derived.model_hash == want.model_hash and derived.reference_phase == 2 and derived.timesteps == 5 and derived.signal_n_dims == 2
    assert derived.spatial_shape == FI.PHASE_SHAPE and np.array_equal(derived.signals, from_reference.signals)
    # the opposite direction: the fields point the other way at the end states
    end = FI.PHASE_SIGNALS[0]
    inside = FI.phase_images()[0] > 0.5
    assert from_reference.predict_field32(end)[2][inside].mean() < -1.0 and derived.predict_field32(end)[2][inside].mean() > 1.0


def test_the_derived_pair_is_more_consistent_than_two_registered_models(models, capsys):
    """At every training state the rms of r = v + u(x + v) of (from_reference, inverted) is below that of (from_reference, the
    inverse=True model), and its mean over the five states is at most half of the other's.  Measured with the float64 restatement:
    the ratio of the means is 0.14, the ratios per state are 0.05 to 0.46."""
    from_reference, independent, derived, _ = models
    ours = [_pair_rms(from_reference, derived, s) for s in FI.PHASE_SIGNALS]
    theirs = [_pair_rms(from_reference, independent, s) for s in FI.PHASE_SIGNALS]
    with capsys.disabled():
        print("\npair residual rms per state, derived: " + ", ".join(f"{v:.3f}" for v in ours) + "; independent: " + ", ".join(f"{v:.3f}" for v in theirs) +
              f"; ratio of the means {np.mean(ours) / np.mean(theirs):.3f}, per state " + ", ".join(f"{a / b:.2f}" for a, b in zip(ours, theirs)))
    assert np.mean(ours) <= 0.5 * np.mean(theirs)
    assert all(a < b for a, b in zip(ours, theirs))
    # the same-direction mistake shows: about 2 |u| at an end state
    assert FI.norms(FI.residual(from_reference.predict_field32(FI.PHASE_SIGNALS[0]), from_reference.predict_field32(FI.PHASE_SIGNALS[0])))[0] > 1.0
    assert _pair_rms(from_reference, from_reference, FI.PHASE_SIGNALS[0]) > 1.0  # measured: 5.2
    # the swapped pair does not: it differs from the pair only where the clamp at the border acts (measured: 0.10 to 0.67 rms) and stays
    # below what two independently registered models give
    swapped = [_pair_rms(derived, from_reference, s) for s in FI.PHASE_SIGNALS]
    assert all(a < b for a, b in zip(swapped[:2] + swapped[3:], theirs[:2] + theirs[3:])) and max(swapped) < 1.0


def test_inverted_refuses_what_does_not_converge_and_what_is_not_fitted(models):
    from_reference = models[0]
    with pytest.raises(RuntimeError, match="did not converge"):
        from_reference.inverted(relaxation=1.0, _invert=FI.as_invert_field())
    with pytest.raises(RuntimeError, match="did not converge"):
        from_reference.inverted(iterations=2, _invert=FI.as_invert_field())
    assert len(from_reference.inverted(iterations=2, tolerance=None, _invert=FI.as_invert_field()).inversion_reports) == 5
    with pytest.raises(RuntimeError, match="not fitted"):
        CorrespondenceModel().inverted(_invert=FI.as_invert_field())
    with pytest.raises(RuntimeError, match="not fitted"):
        from_reference.pair_residual(CorrespondenceModel(), FI.PHASE_SIGNALS[0])


def test_build_pair_is_build_default_and_its_inverse(monkeypatch):
    images = FI.phase_images()[:, ::2, ::2, ::2]
    register_calls, invert_calls = [], []

    def register(fixed, moving, **kw):
        register_calls.append(kw)
        return _restatement_as_register(fixed, moving, **{k: v for k, v in kw.items() if k != "gpu_id"})

    monkeypatch.setattr(reg, "register", register)
    monkeypatch.setattr(reg, "invert_field", FI.as_invert_field(calls=invert_calls))
    kw = dict(signals=FI.PHASE_SIGNALS, reference_phase=2, iterations=5, n_levels=1)
    from_reference, to_reference = CorrespondenceModel.build_pair(images, gpu_id=1, inversion=dict(iterations=30, tolerance=0.5), **kw)
    assert len(register_calls) == 5 and all(c["gpu_id"] == 1 and c["iterations"] == 5 for c in register_calls)
    assert invert_calls == [dict(iterations=30, relaxation=0.5, gpu_id=1)] * 5
    want = CorrespondenceModel.build_default(images, **kw)
    assert from_reference.model_hash == want.model_hash and to_reference.model_hash == want.inverted(iterations=30, tolerance=0.5).model_hash
    assert to_reference.model_hash != from_reference.model_hash and len(to_reference.inversion_reports) == 5
    with pytest.raises(ValueError, match="inverse"):
        CorrespondenceModel.build_pair(images, inverse=True, **kw)


def test_pair_residual_refuses_models_that_do_not_match(models):
    from_reference, _, derived, _ = models
    small = CorrespondenceModel().fit(np.zeros((5, 3, 4, 4, 4), dtype=np.float32), FI.PHASE_SIGNALS, reference_phase=2)
    one_dim = CorrespondenceModel().fit(np.stack([derived.predict_field32(s) for s in FI.PHASE_SIGNALS]), FI.PHASE_SIGNALS[:, :1] + np.arange(5)[:, None], reference_phase=2)
    with pytest.raises(ValueError, match="do not form a pair"):
        from_reference.pair_residual(small, FI.PHASE_SIGNALS[0])
    with pytest.raises(ValueError, match="do not form a pair"):
        from_reference.pair_residual(one_dim, FI.PHASE_SIGNALS[0])


# ---------------------------------------------------------------------------------------------------------------- options and ABI
def _options(**fields):
    o = reg._InvertOptions(C.sizeof(reg._InvertOptions), nx=4, ny=3, nz=2, iterations=1, device=0, relaxation=0.5)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def test_every_refusal_comes_without_a_device():
    """struct_size 0, a null pointer, a size below 1, 2^31 voxels, negative iterations, a relaxation that is not finite or outside (0, 1]:
    each returns -1 with a message, none reaches a HIP call (this test runs without a GPU), and the library goes on working."""
    _, lib = reg._library()
    lib.mcgpu_last_error.restype = C.c_char_p
    u = np.zeros((3, 4, 3, 2), dtype=np.float32)
    v = np.zeros_like(u)

    def invert(o, field=u.ctypes.data, out=v.ctypes.data, report=None):
        return lib.mcgpu_invert_field(C.byref(o) if o is not None else None, field, out, report)

    def residual(o, a=u.ctypes.data, b=v.ctypes.data, report=None):
        return lib.mcgpu_field_residual(C.byref(o) if o is not None else None, a, b, None, report)

    bad_options = [dict(struct_size=0), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=2048, ny=1024, nz=1024), dict(nx=65536, ny=65536, nz=4), dict(iterations=-1),
                   dict(relaxation=0.0), dict(relaxation=-0.5), dict(relaxation=1.5), dict(relaxation=float("nan")), dict(relaxation=float("inf")), dict(device=-1)]
    for name, call in (("mcgpu_invert_field", invert), ("mcgpu_field_residual", residual)):
        for fields in bad_options:
            assert call(_options(**fields)) == -1, (name, fields)
            message = lib.mcgpu_last_error().decode()
            assert name in message, (fields, message)
            assert lib.mcgpu_abi_version() == 1
        assert call(None) == -1
        short = reg._InvertReport(4)
        assert call(_options(), report=C.byref(short)) == -1 and "struct_size" in lib.mcgpu_last_error().decode()
    assert invert(_options(), field=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert invert(_options(), out=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert residual(_options(), a=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert residual(_options(), b=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert (2047 * 1024 * 1024) < 2 ** 31 <= 2048 * 1024 * 1024  # the first size that is refused
    assert not v.any()


def test_python_layer_refuses_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(reg, "_library", lambda: pytest.fail("the checks come first"))
    field = np.zeros((3, 4, 4, 4), dtype=np.float32)
    for bad in (np.zeros((2, 4, 4, 4)), np.zeros((3, 4, 4)), np.zeros((3, 4, 4, 0)), np.zeros((1, 3, 4, 4, 4))):
        with pytest.raises(ValueError, match=r"a field \[3, x, y, z\]"):
            reg.invert_field(bad)
    for poison in (np.nan, np.inf, -np.inf):
        bad = field.copy()
        bad[1, 2, 3, 0] = poison
        with pytest.raises(ValueError, match="not finite"):
            reg.invert_field(bad)
        with pytest.raises(ValueError, match="initial is not finite"):
            reg.invert_field(field, initial=bad)
        with pytest.raises(ValueError, match="not finite"):
            reg.composition_residual(field, bad)
    for relaxation in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="relaxation"):
            reg.invert_field(field, relaxation=relaxation)
    with pytest.raises(ValueError, match="iterations"):
        reg.invert_field(field, iterations=-1)
    with pytest.raises(ValueError, match="expected"):
        reg.invert_field(field, initial=np.zeros((3, 4, 4, 5)))
    with pytest.raises(ValueError, match="expected"):
        reg.composition_residual(field, np.zeros((3, 4, 5, 4)))
    assert reg.check_invert_parameters(40, 1.0) == (40, 1.0) and reg.check_invert_parameters(0, 0.5) == (0, 0.5)


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """Field names in the header's order; sizeof and every offsetof / size as the C compiler lays the header out; the entry points are
    declared and exported."""
    mirrors = [("mcgpu_invert_options", reg._InvertOptions), ("mcgpu_invert_report", reg._InvertReport)]
    abi_layout.assert_field_names(mirrors)
    header = abi_layout.HEADER.read_text()
    for name in ("mcgpu_invert_field", "mcgpu_field_residual"):
        assert re.search(r"int %s\(" % name, header) and name in pkg.engine.ABI_SYMBOLS, name
    cc = abi_layout.c_compiler()
    if cc is not None:
        abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    print("mirrors:", [m[0] for m in mirrors], "C compiler:", cc)
