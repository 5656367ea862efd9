"""Joseph forward projection on the MI355X -- the in-process stand-in for the reference's `cbctmc/forward_projection.py`
(`prepare_image_for_rtk`, `project_forward`, `create_geometry`, `save_geometry`), which runs RTK's
JosephForwardProjectionImageFilter from the `itk-rtk` wheel on the CPU.

Images are `RTKImage` objects (array in ITK order [z][y][x], spacing and origin in ITK (x, y, z) order) instead of
`itk.Image`; there is no `itk` dependency.  The arithmetic is `csrc/forward_project.hip` through `mcgpu_forward_project`
(host volume) or `mcgpu_forward_project_context` (the geometry resident in an engine context, `engine.Context.project_forward`);
there is no CPU fallback.  The scheme is restated in float64 by tests/joseph_ref.py and pinned there by analytic chords.
Parity against RTK itself is unpinned: RTK is not available to this repository, so its exact border handling could not be
checked."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import defaults
from .reconstruction import CircularGeometry, create_geometry, save_geometry  # noqa: F401  (the reference module's surface)

__all__ = ["RTKImage", "prepare_image_for_rtk", "project_forward", "create_geometry", "save_geometry", "rescale_range"]


@dataclass
class RTKImage:
    """What the reference hands to and gets from RTK as an `itk.Image`: `array` in ITK's numpy order [z][y][x],
    `spacing` and `origin` (centre of voxel 0) in ITK's (x, y, z) order, mm."""
    array: np.ndarray
    spacing: Tuple[float, float, float]
    origin: Tuple[float, float, float]

    @property
    def shape(self):
        return self.array.shape


def rescale_range(values, input_range, output_range, clip: bool = True):
    """cbctmc/utils.py: rescale_range (linear map of input_range onto output_range, clipped to output_range)."""
    if input_range and output_range and (tuple(input_range) != tuple(output_range)):
        in_min, in_max = input_range
        out_min, out_max = output_range
        values = ((values - in_min) * (out_max - out_min)) / (in_max - in_min) + out_min
        if clip:
            values = np.clip(values, out_min, out_max)
    return values


def prepare_image_for_rtk(image: np.ndarray, input_value_range: Optional[Tuple[float, float]] = (-1024, 3071),
                          output_value_range: Optional[Tuple[float, float]] = (0.0, 1.0),
                          image_spacing: Optional[Tuple[float, float, float]] = None,
                          origin_offset: Optional[Tuple[float, float, float]] = None) -> RTKImage:
    """cbctmc/forward_projection.py:18-95 for a numpy image indexed [x, y, z] (RAI: x R-L, y A-P, z I-S), e.g.
    `MCGeometry.densities`, with `image_spacing` in the same order.

    The transform is the reference's: `rot90(k=1, axes=(0, 1))`, `swapaxes(1, 2)`, flip of the middle axis, then the array is
    read as an ITK image.  Result: IEC X = MC x, IEC Y = -MC z, IEC Z = -MC y, spacing (sx, sz, sy).

    The origin follows the reference's rule (forward_projection.py:71-87) literally, half-voxel shift included:
        origin = (-NX SX / 2 + SY / 2,  -NY SZ / 2 + SZ / 2,  -NZ SY / 2 + SX / 2)
    with ITK size (NX, NY, NZ) and spacing (SX, SY, SZ).  For isotropic spacing that centres the volume at -(n - 1)/2 s.  For
    anisotropic spacing it pairs the spacings with the wrong axes (the rule permutes the spacing list before zipping it with the
    numpy-order shape); this is reproduced, not corrected, so that forward projections match the reference's."""
    if image_spacing is None:
        raise RuntimeError("Please pass image_spacing")
    arr = np.asarray(image, dtype=np.float32)
    if arr.ndim != 3:
        raise ValueError(f"expected a 3-D image, got shape {arr.shape}")
    if input_value_range and output_value_range:
        arr = rescale_range(arr, input_range=input_value_range, output_range=output_value_range)
    arr = np.rot90(arr, k=1, axes=(0, 1))
    arr = np.swapaxes(arr, 1, 2)
    arr = np.ascontiguousarray(arr[:, ::-1, :], dtype=np.float32)
    spacing, origin = rtk_frame(np.shape(image), image_spacing, origin_offset)
    return RTKImage(arr, spacing, origin)


def rtk_frame(image_shape, image_spacing, origin_offset=None):
    """(spacing, origin) in ITK (x, y, z) order that prepare_image_for_rtk gives an [x, y, z] image of this shape and spacing."""
    nx, ny, nz = (int(n) for n in image_shape)
    sx, sy, sz = (float(s) for s in image_spacing)
    spacing = (sx, sz, sy)                                # ITK (X, Y, Z)
    voxel_size = [spacing[1], spacing[2], spacing[0]]     # the reference's permutation
    origin = [-0.5 * n * v for n, v in zip((ny, nz, nx), voxel_size)]  # numpy-order shape (NZ, NY, NX) of the ITK image
    origin = [origin[2], origin[1], origin[0]]
    origin = [o + 0.5 * v for o, v in zip(origin, voxel_size)]
    if origin_offset:
        origin = [o + oo for o, oo in zip(origin, origin_offset)]
    return spacing, tuple(float(o) for o in origin)


class _FpOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("n_proj", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("du", C.c_double), ("dv", C.c_double),
                ("u0", C.c_double), ("v0", C.c_double), ("sid", C.c_double), ("sdd", C.c_double), ("gantry_deg", C.POINTER(C.c_double)),
                ("proj_offset_x", C.POINTER(C.c_double)), ("proj_offset_y", C.POINTER(C.c_double)), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int), ("sx", C.c_double), ("sy", C.c_double), ("sz", C.c_double), ("ox", C.c_double), ("oy", C.c_double),
                ("oz", C.c_double), ("device", C.c_int)]


class _FpReport(C.Structure):
    _fields_ = [("ms_kernel", C.c_double), ("ms_upload", C.c_double)]


def detector_origin(detector_size, detector_pixel_spacing) -> Tuple[float, float]:
    """Centre of pixel (0, 0): the reference's ConstantImageSource origin -0.5 n spacing (forward_projection.py:127-131).  Not
    centred: the pixel centres sit half a pixel off the -(n - 1)/2 convention, as in the reference."""
    return (-0.5 * detector_size[0] * detector_pixel_spacing[0], -0.5 * detector_size[1] * detector_pixel_spacing[1])


def _project(lib, geometry: CircularGeometry, detector_size, detector_pixel_spacing, spacing=None, origin=None, volume=None,
             context=None, gpu_id: int = 0):
    """One call of mcgpu_forward_project (volume [NZ][NY][NX]) or mcgpu_forward_project_context (context handle)."""
    from . import engine
    dp = C.POINTER(C.c_double)
    lib.mcgpu_forward_project.argtypes = [C.POINTER(_FpOptions), C.c_void_p, C.c_void_p, C.POINTER(_FpReport)]
    lib.mcgpu_forward_project_context.argtypes = [C.c_void_p, C.POINTER(_FpOptions), C.c_void_p, C.POINTER(_FpReport)]
    nu, nv = int(detector_size[0]), int(detector_size[1])
    du, dv = float(detector_pixel_spacing[0]), float(detector_pixel_spacing[1])
    u0, v0 = detector_origin((nu, nv), (du, dv))
    ang = np.ascontiguousarray(geometry.gantry_angles, dtype=np.float64)
    ox = np.ascontiguousarray(geometry.projection_offsets_x, dtype=np.float64)
    oy = np.ascontiguousarray(geometry.projection_offsets_y, dtype=np.float64)
    n = ang.size
    if n < 1:
        raise ValueError("the geometry has no projections")
    dims = (0, 0, 0) if volume is None else volume.shape[::-1]
    sp = (0.0, 0.0, 0.0) if spacing is None else tuple(float(s) for s in spacing)
    org = (float("nan"),) * 3 if origin is None else tuple(float(o) for o in origin)
    o = _FpOptions(C.sizeof(_FpOptions), n, nu, nv, du, dv, u0, v0, float(geometry.source_to_isocenter), float(geometry.source_to_detector),
                   ang.ctypes.data_as(dp), ox.ctypes.data_as(dp), oy.ctypes.data_as(dp), int(dims[0]), int(dims[1]), int(dims[2]), *sp, *org,
                   int(gpu_id))
    out = np.empty((n, nv, nu), dtype=np.float32)
    rep = _FpReport()
    if context is not None:
        engine._check(lib.mcgpu_forward_project_context(context, C.byref(o), out.ctypes.data, C.byref(rep)))
    else:
        vol = np.ascontiguousarray(volume, dtype=np.float32)
        engine._check(lib.mcgpu_forward_project(C.byref(o), vol.ctypes.data, out.ctypes.data, C.byref(rep)))
    return out, {"ms_kernel": rep.ms_kernel, "ms_upload": rep.ms_upload}


def project_forward(image: RTKImage, geometry: CircularGeometry,
                    detector_size: Tuple[int, int] = defaults.DEFAULTS.n_detector_pixels_half_fan,
                    detector_pixel_spacing: Tuple[float, float] = defaults.DEFAULTS.detector_pixel_size,
                    gpu_id: int = 0, report: Optional[dict] = None) -> RTKImage:
    """cbctmc/forward_projection.py:98-149: Joseph forward projection of `image` (an `RTKImage` in the IEC frame, as
    `prepare_image_for_rtk` returns) on `geometry`.  Returns the stack [n][nv][nu] with spacing (du, dv, 1) and origin
    (-0.5 nu du, -0.5 nv dv, 0) -- the reference's ConstantImageSource, whose pixel centres are half a pixel off centre.
    `report`, if given, receives the kernel and upload milliseconds."""
    from . import engine
    proj, rep = _project(engine.load_library(), geometry, detector_size, detector_pixel_spacing, image.spacing, image.origin,
                         volume=image.array, gpu_id=gpu_id)
    if report is not None:
        report.update(rep)
    u0, v0 = detector_origin(detector_size, detector_pixel_spacing)
    return RTKImage(proj, (float(detector_pixel_spacing[0]), float(detector_pixel_spacing[1]), 1.0), (u0, v0, 0.0))


def stack_metadata(detector_size: Sequence[int] = defaults.DEFAULTS.n_detector_pixels_half_fan,
                   detector_pixel_spacing: Sequence[float] = defaults.DEFAULTS.detector_pixel_size):
    """(spacing, origin) of a forward-projection stack (density_fp.mha, density_fp_4d.mha): what the reference sets
    (scripts/run_mc_simulations.py:535-552)."""
    u0, v0 = detector_origin(detector_size, detector_pixel_spacing)
    return (float(detector_pixel_spacing[0]), float(detector_pixel_spacing[1]), 1.0), (u0, v0, 0.0)
