"""Demons registration of two volumes on the MI355X: what the reference's `CorrespondenceModel.build_default`
obtains from vroc's variational registration (cbctmc/registration/correspondence.py:315-345).  vroc is not vendored in the reference
and parity with it is unpinned; what is pinned is the rule in the header of `csrc/registration.hip`, its float64 restatement
(tests/registration_ref.py) and the kernels held to that restatement.  There is no CPU fallback.

Arrays are [x, y, z] as an `MCGeometry` holds them and as `CorrespondenceModel.fit(..., frame="geometry")` takes them; the field is
[3, x, y, z] in voxels on the fixed grid, component i along axis i, with moving(x + u(x)) ~ fixed(x): it goes into `fit`,
`MCGeometry.warp` and `Context.warp_geometry` unchanged.

`invert_field` turns such a field into its inverse (csrc/field_inverse.hip, restatement
tests/field_inverse_ref.py): v with u(x + v(x)) + v(x) ~ 0, so that fixed(y + v(y)) ~ moving(y); `composition_residual` says how far
two fields are from being each other's inverse."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

MAX_LEVELS = 8
MAX_SIGMA = 4.0
STAGES = {"resize_linear": 0, "resize_nearest": 1, "warp_linear": 2, "force_step": 3, "smooth": 4}
# the reference's default_parameters that have no counterpart here, and the only value each may take
_FIXED_PARAMETERS = {"tau_level_decay": 0.0, "tau_iteration_decay": 0.0, "sigma_level_decay": 0.0, "sigma_iteration_decay": 0.0, "largest_scale_factor": 1.0}


class _RegisterOptions(C.Structure):
    """mcgpu_register_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("iterations", C.c_int), ("n_levels", C.c_int), ("device", C.c_int),
                ("out_nx", C.c_int), ("out_ny", C.c_int), ("out_nz", C.c_int), ("tau", C.c_double), ("sigma", C.c_double * 3), ("differences", C.POINTER(C.c_float))]


class _RegisterReport(C.Structure):
    """mcgpu_register_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_levels", C.c_int), ("msd_before", C.c_double * MAX_LEVELS), ("msd_after", C.c_double * MAX_LEVELS),
                ("ms_upload", C.c_double), ("ms_resize", C.c_double), ("ms_force", C.c_double), ("ms_smooth", C.c_double), ("ms_reduce", C.c_double),
                ("ms_total", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


class _InvertOptions(C.Structure):
    """mcgpu_invert_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("iterations", C.c_int), ("device", C.c_int),
                ("relaxation", C.c_double), ("initial", C.POINTER(C.c_float))]


class _InvertReport(C.Structure):
    """mcgpu_invert_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("iterations", C.c_int), ("residual_max_before", C.c_double), ("residual_rms_before", C.c_double),
                ("residual_max_after", C.c_double), ("residual_rms_after", C.c_double), ("ms_upload", C.c_double), ("ms_step", C.c_double),
                ("ms_reduce", C.c_double), ("ms_total", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


def level_shape(shape: Sequence[int], level: int) -> Tuple[int, ...]:
    """ceil(n / 2^level) per axis."""
    return tuple(-(-int(n) // (1 << level)) for n in shape)


def check_parameters(iterations, tau, sigma, n_levels, **fixed_parameters) -> Tuple[int, float, Tuple[float, float, float], int]:
    """The parameters as the device call takes them; ValueError for what the rule does not cover (a decay other than 0,
    largest_scale_factor other than 1, a sigma outside [0, 4], an unknown name)."""
    for name, value in fixed_parameters.items():
        if name not in _FIXED_PARAMETERS:
            raise ValueError(f"unknown registration parameter '{name}'")
        if float(value) != _FIXED_PARAMETERS[name]:
            raise ValueError(f"{name} = {value}: only {_FIXED_PARAMETERS[name]} is supported")
    sigma = tuple(float(s) for s in (sigma if np.ndim(sigma) else (sigma,) * 3))
    if len(sigma) != 3 or any(not (0.0 <= s <= MAX_SIGMA) for s in sigma):
        raise ValueError(f"sigma {sigma}: three values in [0, {MAX_SIGMA}] voxels (the kernels' radius int(4 sigma + 0.5) is at most 16)")
    if int(iterations) < 0:
        raise ValueError(f"iterations {iterations} is negative")
    if not 1 <= int(n_levels) <= MAX_LEVELS:
        raise ValueError(f"n_levels {n_levels} is outside 1..{MAX_LEVELS}")
    if not np.isfinite(tau):
        raise ValueError(f"tau {tau} is not finite")
    return int(iterations), float(tau), sigma, int(n_levels)


def _volume(a, name, dtype=np.float32, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 3 or a.size == 0:
        raise ValueError(f"{name} of shape {a.shape}: a volume [x, y, z]")
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{name} of shape {a.shape}, expected {tuple(shape)}")
    return a


def _library():
    from . import engine
    lib = engine.load_library()
    lib.mcgpu_register.argtypes = [C.POINTER(_RegisterOptions)] + [C.c_void_p] * 4 + [C.POINTER(_RegisterReport)]
    lib.mcgpu_register.restype = C.c_int
    lib.mcgpu_register_stage.argtypes = [C.POINTER(_RegisterOptions), C.c_int] + [C.c_void_p] * 5 + [C.POINTER(_RegisterReport)]
    lib.mcgpu_register_stage.restype = C.c_int
    lib.mcgpu_invert_field.argtypes = [C.POINTER(_InvertOptions)] + [C.c_void_p] * 2 + [C.POINTER(_InvertReport)]
    lib.mcgpu_invert_field.restype = C.c_int
    lib.mcgpu_field_residual.argtypes = [C.POINTER(_InvertOptions)] + [C.c_void_p] * 3 + [C.POINTER(_InvertReport)]
    lib.mcgpu_field_residual.restype = C.c_int
    return engine, lib


def _options(shape, iterations, tau, sigma, n_levels, gpu_id, out_shape=(0, 0, 0)):
    return _RegisterOptions(C.sizeof(_RegisterOptions), *(int(n) for n in shape), iterations, n_levels, int(gpu_id), *(int(n) for n in out_shape), tau,
                            (C.c_double * 3)(*sigma), None)


def _report_dict(rep: _RegisterReport, n_levels: int) -> dict:
    out = {name: getattr(rep, name) for name, _ in _RegisterReport._fields_ if name.startswith("ms_") or name == "peak_device_bytes"}
    out["msd_before"] = [rep.msd_before[level] for level in range(n_levels)]
    out["msd_after"] = [rep.msd_after[level] for level in range(n_levels)]
    return out


def register(fixed, moving, fixed_mask=None, iterations: int = 800, tau: float = 2.25, sigma=(1.25, 1.25, 1.25), n_levels: int = 3, gpu_id: int = 0,
             return_differences: bool = False, **fixed_parameters):
    """-> (field float32 [3, x, y, z], report dict).  The defaults are the reference's `default_parameters`; its decays and
    `largest_scale_factor` are accepted only at the values it passes (0 and 1).  Only the voxels where `fixed_mask` is non-zero are
    driven (the field still spreads into the others by the smoothing).

    report: msd_before / msd_after (lists indexed by level, 0 = finest: the mean squared difference of the warped moving image and
    the fixed one before the level's first and after its last iteration), ms_upload, ms_resize, ms_force, ms_smooth, ms_reduce,
    ms_total, peak_device_bytes; with return_differences also `differences`: per level, coarsest first, the pair of float32 volumes
    (before, after) those means were taken of."""
    iterations, tau, sigma, n_levels = check_parameters(iterations, tau, sigma, n_levels, **fixed_parameters)
    f = _volume(fixed, "fixed")
    m = _volume(moving, "moving", shape=f.shape)
    mask = None if fixed_mask is None else _volume(np.asarray(fixed_mask) != 0, "fixed_mask", np.uint8, f.shape)
    engine, lib = _library()
    o = _options(f.shape, iterations, tau, sigma, n_levels, gpu_id)
    shapes = [level_shape(f.shape, level) for level in range(n_levels - 1, -1, -1)]
    differences = None
    if return_differences:
        differences = np.zeros(2 * sum(int(np.prod(s)) for s in shapes), dtype=np.float32)
        o.differences = differences.ctypes.data_as(C.POINTER(C.c_float))
    field = np.empty((3,) + f.shape, dtype=np.float32)
    rep = _RegisterReport(C.sizeof(_RegisterReport))
    engine._check(lib.mcgpu_register(C.byref(o), f.ctypes.data, m.ctypes.data, None if mask is None else mask.ctypes.data, field.ctypes.data, C.byref(rep)))
    report = _report_dict(rep, n_levels)
    if differences is not None:
        report["differences"], at = [], 0
        for s in shapes:
            n = int(np.prod(s))
            report["differences"].append((differences[at:at + n].reshape(s), differences[at + n:at + 2 * n].reshape(s)))
            at += 2 * n
    return field, report


def register_stage(stage: str, shape=None, fixed=None, moving=None, field=None, fixed_mask=None, out_shape=None, tau: float = 2.25,
                   sigma=(1.25, 1.25, 1.25), gpu_id: int = 0):
    """One operator of the rule alone (`mcgpu_register_stage`), for tests: -> (result, report dict).

    resize_linear: moving -> float32 of `out_shape`;  resize_nearest: fixed_mask -> uint8 of `out_shape`;  warp_linear: moving, field ->
    moving(x + u);  force_step: fixed, moving, field, fixed_mask (optional) -> u + tau v;  smooth: field -> the smoothed field."""
    if stage not in STAGES:
        raise ValueError(f"stage '{stage}': one of {', '.join(STAGES)}")
    _, tau, sigma, _ = check_parameters(0, tau, sigma, 1)
    given = next(np.shape(a)[-3:] for a in (fixed, moving, field, fixed_mask) if a is not None) if shape is None else tuple(shape)
    f = None if fixed is None else _volume(fixed, "fixed", shape=given)
    m = None if moving is None else _volume(moving, "moving", shape=given)
    mask = None if fixed_mask is None else _volume(fixed_mask, "fixed_mask", np.uint8, given)
    u = None
    if field is not None:
        u = np.ascontiguousarray(field, dtype=np.float32)
        if u.shape != (3,) + tuple(given):
            raise ValueError(f"field of shape {u.shape}, expected {(3,) + tuple(given)}")
    resize = stage in ("resize_linear", "resize_nearest")
    if resize and (out_shape is None or len(out_shape) != 3 or min(out_shape) < 1):
        raise ValueError("the resize stages need out_shape = (x, y, z)")
    if stage == "resize_nearest":
        out = np.empty(tuple(out_shape), dtype=np.uint8)
    elif stage in ("resize_linear", "warp_linear"):
        out = np.empty(tuple(out_shape) if resize else given, dtype=np.float32)
    else:
        out = np.empty((3,) + tuple(given), dtype=np.float32)
    engine, lib = _library()
    o = _options(given, 0, tau, sigma, 1, gpu_id, out_shape if resize else (0, 0, 0))
    rep = _RegisterReport(C.sizeof(_RegisterReport))
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    engine._check(lib.mcgpu_register_stage(C.byref(o), STAGES[stage], ptr(f), ptr(m), ptr(u), ptr(mask), out.ctypes.data, C.byref(rep)))
    return out, _report_dict(rep, 0)


# ---- the inverse of a field (row f22)
def _field(a, name, shape=None):
    """float32 [3, x, y, z], finite; ValueError otherwise."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 4 or a.shape[0] != 3 or a.size == 0:
        raise ValueError(f"{name} of shape {a.shape}: a field [3, x, y, z]")
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{name} of shape {a.shape}, expected {tuple(shape)}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} is not finite")
    return a


def check_invert_parameters(iterations, relaxation) -> Tuple[int, float]:
    """(iterations, relaxation) as the device call takes them; ValueError for what it refuses."""
    if int(iterations) < 0:
        raise ValueError(f"iterations {iterations} is negative")
    relaxation = float(relaxation)
    if not np.isfinite(relaxation) or not 0.0 < relaxation <= 1.0:
        raise ValueError(f"relaxation {relaxation} is outside (0, 1]")
    return int(iterations), relaxation


def check_residual(report: dict, tolerance: Optional[float]) -> None:
    """RuntimeError if the inversion's `residual_max_after` exceeds `tolerance` (None: no check): how a field that folds, or a
    relaxation too large for the field's slopes, shows itself."""
    if tolerance is not None and not report["residual_max_after"] <= float(tolerance):
        raise RuntimeError(f"field inversion did not converge: max residual {report['residual_max_after']:.3g} voxel after {report['iterations']} iterations "
                           f"(before: {report['residual_max_before']:.3g}) exceeds the tolerance {float(tolerance):.3g}; "
                           "the field folds, or relaxation is too large for its slopes")


def _invert_report_dict(rep: _InvertReport) -> dict:
    return {name: getattr(rep, name) for name, _ in _InvertReport._fields_ if name != "struct_size"}


def invert_field(field, iterations: int = 40, relaxation: float = 0.5, initial=None, tolerance: Optional[float] = None, gpu_id: int = 0):
    """-> (inverse float32 [3, x, y, z], report dict).  `field` u is what `register` returns (moving(x + u(x)) ~ fixed(x)); the
    inverse v satisfies u(x + v(x)) + v(x) ~ 0, so fixed(y + v(y)) ~ moving(y).  `iterations` Jacobi steps v <- v - relaxation r,
    r(x) = v(x) + u(x + v(x)), from `initial` (default zeros); no early stop, two calls give the same bytes.

    The defaults come from the float64 restatement, not from a clinical field: relaxation 1 converges only where the field's finite
    differences stay below 1 (the demons field of the test sphere has 1.69 and stalls at a residual of 3 voxels); with 0.5 that
    field reaches 9e-5 voxel after 20 steps, 1e-6 after 30 and 1.4e-8 after 40 (float32 stops near 1e-6).

    report: iterations, residual_max_before / residual_rms_before / residual_max_after / residual_rms_after (voxels), ms_upload,
    ms_step, ms_reduce, ms_total, peak_device_bytes.  With a `tolerance`, RuntimeError if residual_max_after exceeds it: a field
    that folds has no inverse and shows itself that way.  ValueError: a shape other than [3, x, y, z], a field that is not
    finite, negative iterations, a relaxation outside (0, 1]."""
    iterations, relaxation = check_invert_parameters(iterations, relaxation)
    u = _field(field, "field")
    v0 = None if initial is None else _field(initial, "initial", u.shape)
    engine, lib = _library()
    o = _InvertOptions(C.sizeof(_InvertOptions), *(int(n) for n in u.shape[1:]), iterations, int(gpu_id), relaxation,
                       None if v0 is None else v0.ctypes.data_as(C.POINTER(C.c_float)))
    inverse = np.empty_like(u)
    rep = _InvertReport(C.sizeof(_InvertReport))
    engine._check(lib.mcgpu_invert_field(C.byref(o), u.ctypes.data, inverse.ctypes.data, C.byref(rep)))
    report = _invert_report_dict(rep)
    check_residual(report, tolerance)
    return inverse, report


def composition_residual(u, v, gpu_id: int = 0):
    """-> (residual float32 [3, x, y, z], report dict): r(x) = v(x) + u(x + v(x)) in voxels, about zero where v is the inverse of
    u and about 2 |u| where v = u.  report: residual_max, residual_rms, ms_upload, ms_reduce, ms_total, peak_device_bytes."""
    u = _field(u, "u")
    v = _field(v, "v", u.shape)
    engine, lib = _library()
    o = _InvertOptions(C.sizeof(_InvertOptions), *(int(n) for n in u.shape[1:]), 0, int(gpu_id), 1.0, None)
    residual = np.empty_like(u)
    rep = _InvertReport(C.sizeof(_InvertReport))
    engine._check(lib.mcgpu_field_residual(C.byref(o), u.ctypes.data, v.ctypes.data, residual.ctypes.data, C.byref(rep)))
    report = dict(residual_max=rep.residual_max_before, residual_rms=rep.residual_rms_before, ms_upload=rep.ms_upload, ms_reduce=rep.ms_reduce,
                  ms_total=rep.ms_total, peak_device_bytes=rep.peak_device_bytes)
    return residual, report
