"""Demons registration without a GPU: the float64 restatement (tests/registration_ref.py) against scipy's Gaussian
and sampler and on known answers, the sphere recovery the rule was chosen by, the option checks and the C layout of the ABI structs,
`RespiratorySignal.from_masks` against the reference's steps, and the plumbing of `CorrespondenceModel.build_default` with the
restatement in the place of the device call."""
import ctypes as C
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.ndimage
from scipy.signal import savgol_filter

import cases
import registration_ref as R

pkg = cases.pkg
reg = pkg.registration
CorrespondenceModel = pkg.correspondence.CorrespondenceModel
RespiratorySignal = pkg.respiratory.RespiratorySignal
HEADER = Path(__file__).resolve().parents[1] / "include" / "mcgpu_amd.h"

SPHERE_SHAPE, SPHERE_CENTRE = (40, 36, 32), (20, 18, 16)


# ---------------------------------------------------------------------------------------------------------------- the rule's pieces
@pytest.mark.parametrize("shape, sigma", [((17, 13, 11), (1.25, 1.25, 1.25)), ((17, 13, 11), (0.7, 2.0, 4.0)), ((70, 3, 5), (1.25, 1.25, 1.25)),
                                          ((9, 3, 20), (0.7, 2.0, 4.0)), ((1, 9, 30), (0.0, 1.25, 0.0))])
def test_gaussian_equals_scipy(shape, sigma):
    """Per component, the three passes equal scipy.ndimage.gaussian_filter(mode="nearest", truncate=4.0) to 1e-12, also where an axis
    (3) is shorter than the radius (5, 8, 16)."""
    rng = np.random.default_rng(1)
    field = rng.normal(size=(3,) + shape)
    got = R.smooth(field, sigma)
    for c in range(3):
        want = scipy.ndimage.gaussian_filter(field[c], sigma=sigma, mode="nearest", truncate=4.0)
        assert np.abs(got[c] - want).max() < 1e-12
    assert R.radius(1.25) == 5 and R.radius(4.0) == 16 and R.radius(0.7) == 3
    assert R.gaussian_weights(1.25, np.float32).dtype == np.float32 and abs(R.gaussian_weights(1.25).sum() - 1) < 1e-15


def test_sampler_equals_map_coordinates():
    """Trilinear sampling with the coordinate clamp equals scipy's map_coordinates(order=1, mode="nearest") to 1e-12, with coordinates
    outside on every face."""
    rng = np.random.default_rng(2)
    vol = rng.normal(size=(7, 5, 6))
    coords = np.stack([rng.uniform(-3, n + 2, size=4000) for n in vol.shape])
    coords[:, :8] = np.array([[0, 6, 6.5, -1, 3, 3, 3, 3], [2, 2, 2, 2, 0, 4, -0.5, 4.5], [1, 1, 1, 1, 0, 5, 5.25, -2]], dtype=float)
    want = scipy.ndimage.map_coordinates(vol, coords, order=1, mode="nearest")
    assert np.abs(R.sample(vol, coords) - want).max() < 1e-12
    u = rng.uniform(-4, 4, size=(3,) + vol.shape)
    g = np.meshgrid(*(np.arange(n, dtype=float) for n in vol.shape), indexing="ij")
    want = scipy.ndimage.map_coordinates(vol, [g[i] + u[i] for i in range(3)], order=1, mode="nearest")
    assert np.abs(R.warp(vol, u) - want).max() < 1e-12


def test_central_differences_of_a_ramp_are_exact():
    """f = 3 x - 2 y + 0.5 z: the gradient is (3, -2, 0.5) inside and half of it on the faces (the clamped index), exactly."""
    x, y, z = np.meshgrid(np.arange(6.0), np.arange(5.0), np.arange(4.0), indexing="ij")
    g = R.gradient(3 * x - 2 * y + 0.5 * z)
    for axis, slope in enumerate((3.0, -2.0, 0.5)):
        inner = [slice(None)] * 3
        inner[axis] = slice(1, -1)
        assert np.all(g[axis][tuple(inner)] == slope)
        for face in (0, -1):
            inner[axis] = face
            assert np.all(g[axis][tuple(inner)] == slope / 2)


def test_identical_images_give_a_field_of_exact_zeros():
    rng = np.random.default_rng(3)
    image = rng.normal(size=(12, 10, 9)).astype(np.float32)
    mask = (rng.uniform(size=image.shape) > 0.3).astype(np.uint8)
    for dtype in (np.float64, np.float32):
        u, report = R.register(image, image, fixed_mask=mask, iterations=5, n_levels=2, dtype=dtype)
        assert u.shape == (3, 12, 10, 9) and u.dtype == dtype and not u.any()
        assert report["msd_before"] == [0.0, 0.0] and report["msd_after"] == [0.0, 0.0]


def test_level_shapes_and_the_rescaling_guard():
    """s_i = ceil(n_i / 2^l); an axis of 3 shrinks to 1 on the third level, and the field's component along it is then carried up with
    the factor 1 and not (s_new - 1) / 0."""
    assert [R.level_shape((40, 36, 32), level) for level in (2, 1, 0)] == [(10, 9, 8), (20, 18, 16), (40, 36, 32)]
    assert [R.level_shape((500, 501, 3), level) for level in (2, 1, 0)] == [(125, 126, 1), (250, 251, 2), (500, 501, 3)]
    assert reg.level_shape((500, 501, 3), 2) == (125, 126, 1)
    assert R.field_scale((125, 126, 1), (250, 251, 2)) == [float(np.float32(249 / 124)), 2.0, 1.0]
    u = np.ones((3, 5, 4, 1))
    up = R.resize_field(u, (9, 8, 2))
    assert up.shape == (3, 9, 8, 2) and np.all(up[0] == 2.0) and np.all(up[1] == float(np.float32(7 / 3))) and np.all(up[2] == 1.0)
    # align-corners positions: the corners are kept, the tables are those of linspace
    base, frac, nearest = R.resize_tables(6, 3)
    assert base.tolist() == [0, 2, 5] and frac.tolist() == [0.0, 0.5, 0.0] and nearest.tolist() == [0, 3, 5]
    assert R.resize_tables(3, 1)[0].tolist() == [0]
    vol = np.random.default_rng(4).normal(size=(6, 3, 5))
    assert np.array_equal(R.resize_linear(vol, vol.shape), vol)
    small = R.resize_linear(vol, (3, 2, 3))
    assert small[0, 0, 0] == vol[0, 0, 0] and small[-1, -1, -1] == vol[-1, -1, -1]
    rng = np.random.default_rng(5)
    fixed, moving = rng.normal(size=(9, 8, 3)).astype(np.float32), rng.normal(size=(9, 8, 3)).astype(np.float32)
    u, _ = R.register(fixed, moving, iterations=2, n_levels=3)
    assert np.isfinite(u).all()


@pytest.mark.parametrize("s", [2, 4, 6])
def test_sphere_recovery(s, capsys):
    """A sphere of radius 7 with a logistic edge of 1 voxel at (20, 18, 16) in `moving`, shifted by -s along z in `fixed`; three levels
    of 50 iterations, tau 2.25, sigma 1.25.  The residual mean squared difference is at most 0.05 of the initial one and the mean of
    u_z over the sphere (fixed > 0.5) is within 0.3 voxel of s.  The restatement gives (ratio, mean u_z): s = 2: 0.0265, 2.109;
    s = 4: 0.00953, 4.197; s = 6: 0.00441, 6.113 (printed below; profiles/registration_ab.md)."""
    moving = R.sphere(SPHERE_SHAPE, SPHERE_CENTRE)
    fixed = R.sphere(SPHERE_SHAPE, (SPHERE_CENTRE[0], SPHERE_CENTRE[1], SPHERE_CENTRE[2] - s))
    u, report = R.register(fixed, moving, iterations=50, tau=2.25, sigma=(1.25, 1.25, 1.25), n_levels=3)
    initial = R.msd(fixed, moving, np.zeros_like(u))
    ratio, mean_uz = report["msd_after"][0] / initial, float(u[2][fixed > 0.5].mean())
    with capsys.disabled():
        print(f"\nsphere recovery s = {s}: residual ratio {ratio:.5f}, mean u_z {mean_uz:.4f}")
    assert ratio <= 0.05
    assert abs(mean_uz - s) <= 0.3


# ---------------------------------------------------------------------------------------------------------------- options and ABI
def test_option_validation():
    image = np.zeros((4, 4, 4), dtype=np.float32)
    for name in ("tau_level_decay", "tau_iteration_decay", "sigma_level_decay", "sigma_iteration_decay"):
        with pytest.raises(ValueError, match=name):
            reg.register(image, image, **{name: 0.5})
    with pytest.raises(ValueError, match="largest_scale_factor"):
        reg.register(image, image, largest_scale_factor=0.5)
    with pytest.raises(ValueError, match="unknown registration parameter"):
        reg.register(image, image, affine=True)
    with pytest.raises(ValueError, match="sigma"):
        reg.register(image, image, sigma=(1.25, 4.5, 1.25))
    with pytest.raises(ValueError, match="sigma"):
        reg.register(image, image, sigma=(1.25, -1.0, 1.25))
    with pytest.raises(ValueError, match="n_levels"):
        reg.register(image, image, n_levels=0)
    with pytest.raises(ValueError, match="expected"):
        reg.register(image, np.zeros((4, 4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="expected"):
        reg.register(image, image, fixed_mask=np.ones((4, 5, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="volume"):
        reg.register(np.zeros((4, 4)), np.zeros((4, 4)))
    with pytest.raises(ValueError, match="field of shape"):
        reg.register_stage("smooth", field=np.zeros((2, 4, 4, 4)), shape=(4, 4, 4))
    with pytest.raises(ValueError, match="stage"):
        reg.register_stage("affine", field=np.zeros((3, 4, 4, 4)))
    # the values the reference passes are taken
    assert reg.check_parameters(800, 2.25, (1.25, 1.25, 1.25), 3, tau_level_decay=0.0, tau_iteration_decay=0.0, sigma_level_decay=0.0, sigma_iteration_decay=0.0,
                                largest_scale_factor=1.0) == (800, 2.25, (1.25, 1.25, 1.25), 3)


def _header_fields(struct):
    import re
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        parts = [re.sub(r"\[.*?\]", "", p).replace("*", " ").split() for p in decl.split(",")]
        if parts[0]:
            names += [parts[0][-1]] + [p[0] for p in parts[1:]]
    return names


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """Field names in the header's order; sizeof and every offsetof / size as the C compiler lays the header out; the stage numbers."""
    mirrors = [("mcgpu_register_options", reg._RegisterOptions), ("mcgpu_register_report", reg._RegisterReport)]
    for struct, cls in mirrors:
        assert _header_fields(struct) == [f[0] for f in cls._fields_], struct
    cc = next((shutil.which(c) for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mcgpu_amd.h"', "int main(void) {"]
    for struct, cls in mirrors:
        lines.append(f'  printf("{struct} %zu\\n", sizeof({struct}));')
        for name, _ in cls._fields_:
            lines.append(f'  printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct} *)0)->{name}));')
    for name in reg.STAGES:
        lines.append(f'  printf("stage.{name} %d\\n", MCGPU_REGISTER_STAGE_{name.upper()});')
    lines += ['  printf("max_levels %d\\n", MCGPU_REGISTER_MAX_LEVELS);', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    c_side = dict(line.split(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    py_side = {"max_levels": str(reg.MAX_LEVELS)}
    for struct, cls in mirrors:
        py_side[struct] = str(C.sizeof(cls))
        for name, _ in cls._fields_:
            f = getattr(cls, name)
            py_side[f"{struct}.{name}"] = f"{f.offset} {f.size}"
    for name, number in reg.STAGES.items():
        py_side[f"stage.{name}"] = str(number)
    assert c_side == py_side


def test_the_library_exports_the_entry_points_and_refuses_bad_options():
    """No device is needed for a refusal: the options are checked first."""
    _, lib = reg._library()
    image = np.zeros((4, 4, 4), dtype=np.float32)
    field = np.zeros((3, 4, 4, 4), dtype=np.float32)

    def call(**fields):
        o = reg._options((4, 4, 4), 1, 2.25, (1.25, 1.25, 1.25), 1, 0)
        for k, v in fields.items():
            setattr(o, k, v)
        return lib.mcgpu_register(C.byref(o), image.ctypes.data, image.ctypes.data, None, field.ctypes.data, None)

    assert call(struct_size=0) != 0
    assert call(nx=0) != 0
    assert call(n_levels=9) != 0
    assert call(iterations=-1) != 0
    o = reg._options((4, 4, 4), 1, 2.25, (1.25, 5.0, 1.25), 1, 0)
    assert lib.mcgpu_register(C.byref(o), image.ctypes.data, image.ctypes.data, None, field.ctypes.data, None) != 0
    o = reg._options((4, 4, 4), 1, 2.25, (1.25, 1.25, 1.25), 1, 0)
    assert lib.mcgpu_register(C.byref(o), None, image.ctypes.data, None, field.ctypes.data, None) != 0
    assert lib.mcgpu_register_stage(C.byref(o), 7, None, None, field.ctypes.data, None, field.ctypes.data, None) != 0


# ---------------------------------------------------------------------------------------------------------------- from_masks
def _from_masks_by_the_reference_steps(masks, timepoints, total_seconds=60.0, frequency=25.0, window=None, order=3, output_range=(-1, 1)):
    """cbctmc/mc/respiratory.py:158-209 written out."""
    volumes = np.array([np.sum(m > 0) for m in masks])
    timepoints = np.array(timepoints)
    span = timepoints.max() - timepoints.min()
    regular = np.linspace(timepoints.min(), timepoints.max(), int(span * frequency))
    volumes = np.interp(regular, timepoints, volumes)
    n_repeats = math.ceil(total_seconds * frequency / len(volumes))
    signal = np.tile(volumes, n_repeats)[: int(total_seconds * frequency)]
    if window != 0 and order is not None:
        if window is None:
            window = span
        signal = savgol_filter(signal, window_length=int(window * frequency), polyorder=order, mode="mirror")
    lo, hi = signal.min(), signal.max()
    signal = np.clip(((signal - lo) * (output_range[1] - output_range[0])) / (hi - lo) + output_range[0], *output_range)
    return signal, np.gradient(signal, 1 / frequency)


def _breathing_masks(timepoints, period=4.0):
    masks = []
    for t in timepoints:
        m = np.zeros((12, 10, 8), dtype=np.uint8)
        m[: 4 + int(round(6 * math.sin(math.pi * t / period) ** 2)), 2:9, 1:7] = 3
        masks.append(m)
    return masks


@pytest.mark.parametrize("timepoints", [np.arange(10) * 0.4, np.array([0.0, 0.3, 0.9, 1.2, 1.9, 2.3, 2.6, 3.3, 3.7, 4.1])], ids=["regular", "irregular"])
@pytest.mark.parametrize("smoothing", [dict(), dict(smooth_window_seconds=0), dict(smooth_order=None), dict(smooth_window_seconds=1.0, smooth_order=2)],
                         ids=["default", "window0", "order_none", "window1_order2"])
def test_from_masks_follows_the_reference_steps(timepoints, smoothing):
    masks = _breathing_masks(timepoints)
    got = RespiratorySignal.from_masks(masks, timepoints, **smoothing)
    want, want_dt = _from_masks_by_the_reference_steps(masks, timepoints, window=smoothing.get("smooth_window_seconds"), order=smoothing.get("smooth_order", 3))
    assert got.signal.shape == (1500,) and got.sampling_frequency == 25.0
    assert np.array_equal(got.signal, want) and np.array_equal(got.dt_signal, want_dt)
    assert got.signal.min() == -1.0 and got.signal.max() == 1.0
    other = RespiratorySignal.from_masks(masks, timepoints, target_total_seconds=20.0, target_sampling_frequency=10.0, output_range=(0, 2), **smoothing)
    want, _ = _from_masks_by_the_reference_steps(masks, timepoints, 20.0, 10.0, smoothing.get("smooth_window_seconds"), smoothing.get("smooth_order", 3), (0, 2))
    assert other.signal.shape == (200,) and np.array_equal(other.signal, want)


# ---------------------------------------------------------------------------------------------------------------- build_default
def _restatement_as_register(calls):
    def register(fixed, moving, fixed_mask=None, gpu_id=0, **parameters):
        calls.append(dict(fixed=fixed, moving=moving, fixed_mask=fixed_mask, gpu_id=gpu_id, parameters=parameters))
        u, report = R.register(fixed, moving, fixed_mask=fixed_mask, dtype=np.float32, **parameters)
        return u.astype(np.float32), report
    return register


def _phases(T=5, shape=(16, 14, 12)):
    signal = RespiratorySignal.create_cos4(total_seconds=float(T), period=5.0, sampling_frequency=1.0)
    images = np.stack([R.sphere(shape, (8, 7, 6 - 2.0 * a), radius_voxels=3.5) for a in signal.signal])
    masks = np.stack([(np.arange(shape[0])[:, None, None] < 6 + 4 * a) & np.ones(shape, dtype=bool) for a in signal.signal]).astype(np.uint8)
    return images, masks, np.stack([signal.signal, signal.dt_signal], axis=1)


def test_build_default_equals_a_loop_of_register_and_fit(monkeypatch):
    images, masks, signals = _phases()
    calls = []
    monkeypatch.setattr(reg, "register", _restatement_as_register(calls))
    parameters = dict(iterations=4, n_levels=2)
    model = CorrespondenceModel.build_default(images, signals=signals, masks=masks, reference_phase=2, gpu_id=3, **parameters)
    assert len(calls) == 5 and all(c["moving"] is images[2] or np.array_equal(c["moving"], images[2]) for c in calls)
    assert all(np.array_equal(c["fixed"], images[t]) and np.array_equal(c["fixed_mask"], masks[t]) for t, c in enumerate(calls))
    assert all(c["gpu_id"] == 3 and c["parameters"] == parameters for c in calls)
    fields = np.stack([R.register(images[t], images[2], fixed_mask=masks[t], dtype=np.float32, **parameters)[0] for t in range(5)]).astype(np.float32)
    assert not fields[2].any() and np.abs(fields[0]).max() > 0.1  # the reference phase's field is zero, the others are not
    want = CorrespondenceModel().fit(fields, signals, reference_phase=2)
    assert np.array_equal(model.mean_vector_field, want.mean_vector_field) and np.array_equal(model.coefficients, want.coefficients)
    assert model.model_hash == want.model_hash and model.reference_phase == 2 and model.timesteps == 5 and model.spatial_shape == images.shape[1:]
    # without masked registration no mask reaches the registration
    calls.clear()
    CorrespondenceModel.build_default(images, signals=signals, masks=masks, masked_registration=False, **parameters)
    assert all(c["fixed_mask"] is None for c in calls)


def test_build_default_takes_its_signals_from_the_masks(monkeypatch):
    images, masks, _ = _phases()
    timepoints = np.array([0.0, 0.9, 2.1, 3.0, 4.2])
    monkeypatch.setattr(reg, "register", _restatement_as_register([]))
    model = CorrespondenceModel.build_default(images, masks=masks, timepoints=timepoints, iterations=1, n_levels=1)
    curve = RespiratorySignal.from_masks(masks, timepoints)
    want = np.stack([np.interp(timepoints, curve.time, curve.signal), np.interp(timepoints, curve.time, curve.dt_signal)])
    assert model.signal_n_dims == 2 and model.timesteps == 5 and np.array_equal(model.signals, want)


def test_build_default_error_cases(monkeypatch):
    images, masks, signals = _phases()
    monkeypatch.setattr(reg, "register", _restatement_as_register([]))
    with pytest.raises(ValueError, match="timepoints must be given"):
        CorrespondenceModel.build_default(images, masks=masks)
    with pytest.raises(ValueError, match="Either signals or masks"):
        CorrespondenceModel.build_default(images)
    with pytest.raises(ValueError, match="reference_phase"):
        CorrespondenceModel.build_default(images, signals=signals, reference_phase=5)
    with pytest.raises(ValueError, match="signals for"):
        CorrespondenceModel.build_default(images, signals=signals[:4])
    monkeypatch.undo()  # the device call's own checks come before any device work
    with pytest.raises(ValueError, match="tau_level_decay"):
        CorrespondenceModel.build_default(images, signals=signals, tau_level_decay=0.1)
