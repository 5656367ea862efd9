"""Empirical water pre-correction (Sourbelle et al., "Empirical water precorrection for cone-beam computed tomography", 2005), fitted on
the MI355X: what the reference's `scripts/fit_wpc.py` does with N + 1 `rtkfdk` runs, and how its `ReconDefaults.wpc_catphan604`
came about.  The result is the `water_pre_correction` polynomial of `reconstruct_3d` / `reconstruct_4d`.

The rule (float64 restatement: tests/wpc_ref.py).  With q the normalised projections of a water cylinder,
f_n = FDK(q^n), n = 0..N, is the reconstruction `reconstruction.fdk` gives for the polynomial e_n; fbar_n is its mean over a slab of
y slices.  The coefficients minimise sum_pixels weight (sum_n c_n fbar_n - template)^2: c = inv(B) a with
B[i][j] = sum weight fbar_i fbar_j and a[i] = sum weight fbar_i template.  `csrc/wpc_fit.hip` (`mcgpu_wpc_fit`) forms fbar, B and a
in one pass over the projections without ever holding a volume; the (N + 1) x (N + 1) solve is float64 numpy, here.  There is no CPU
fallback.

Coefficients calibrate one pair of simulator and reconstructor: the reference's numbers belong to MC-GPU on CUDA plus rtkfdk, this
engine needs its own fit, and `defaults.py` carries none (a maintainer looks at images first).  Out of scope: the Catphan variant
(`fit_wpc_catphan.py`: per-material weights, `reference_mu`) and a rel_diff over the whole eroded volume."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

from . import defaults
from .materials import material_number
from .reconstruction import CircularGeometry, read_mha

MAX_ORDER = 7


class _WpcFitOptions(C.Structure):
    """mcgpu_wpc_fit_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_proj", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("du", C.c_double), ("dv", C.c_double), ("u0", C.c_double),
                ("v0", C.c_double), ("sid", C.c_double), ("sdd", C.c_double), ("gantry_deg", C.POINTER(C.c_double)), ("proj_offset_x", C.POINTER(C.c_double)),
                ("proj_offset_y", C.POINTER(C.c_double)), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("sx", C.c_double), ("sy", C.c_double),
                ("sz", C.c_double), ("ox", C.c_double), ("oy", C.c_double), ("oz", C.c_double), ("hann", C.c_double), ("hann_y", C.c_double), ("pad", C.c_double),
                ("order", C.c_int), ("y_first", C.c_int), ("y_count", C.c_int), ("device", C.c_int), ("channel_layout", C.c_int)]


class _WpcFitReport(C.Structure):
    _fields_ = [("ms_upload", C.c_double), ("ms_filter", C.c_double), ("ms_backproject", C.c_double), ("ms_reduce", C.c_double), ("ms_total", C.c_double),
                ("peak_device_bytes", C.c_ulonglong)]


@dataclass
class WPCFit:
    coefficients: np.ndarray     # [order + 1] float64: c_0 .. c_N, the water_pre_correction argument of reconstruct_3d
    B: np.ndarray                # [order + 1, order + 1] float64
    a: np.ndarray                # [order + 1] float64
    condition: float             # np.linalg.cond(B)
    residual_identity: float     # sum weight (fbar_1 - template)^2: the uncorrected image
    residual_fit: float          # sum weight (sum_n c_n fbar_n - template)^2
    basis_mean: np.ndarray       # [order + 1, nz, nx] float32: fbar_n in the FDK volume frame
    report: dict                 # ms_upload, ms_filter, ms_backproject, ms_reduce, ms_total, peak_device_bytes
    rel_diff_before: Optional[float] = None  # fit_wpc_phantom only
    rel_diff_after: Optional[float] = None


def solve(B: np.ndarray, a: np.ndarray) -> np.ndarray:
    """c = inv(B) a in float64, as scripts/fit_wpc.py:236-238 does."""
    return np.linalg.inv(np.asarray(B, dtype=np.float64)).dot(np.asarray(a, dtype=np.float64))


def residual(coefficients, basis_mean, weight, template) -> float:
    """sum_pixels weight (sum_n c_n fbar_n - template)^2 in float64."""
    c = np.asarray(coefficients, dtype=np.float64)
    image = np.tensordot(c, np.asarray(basis_mean, dtype=np.float64)[: c.size], axes=1)
    return float(np.sum(np.asarray(weight, dtype=np.float64) * (image - np.asarray(template, dtype=np.float64)) ** 2))


def normal_equations(projections: np.ndarray, geometry: CircularGeometry, pixel_spacing: Tuple[float, float], pixel_origin: Optional[Tuple[float, float]],
                     dimension: Tuple[int, int, int], spacing: Tuple[float, float, float], weight: np.ndarray, template: np.ndarray, slab: Tuple[int, int],
                     order: int = 5, origin: Optional[Tuple[float, float, float]] = None, hann: float = 1.0, hann_y: float = 1.0, pad: float = 1.0,
                     gpu_id: int = 0, channel_layout: int = 0):
    """mcgpu_wpc_fit: (B [order + 1, order + 1], a [order + 1], basis_mean [order + 1, nz, nx] float32, report dict).
    slab = (y_first, y_count).  channel_layout: 0 = the default, 1 / 2 = the two layouts of the back-projector's input
    (tools/wpc_fit_bench.py measures both; the results are the same)."""
    from . import engine
    lib = engine.load_library()
    lib.mcgpu_wpc_fit.argtypes = [C.POINTER(_WpcFitOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_WpcFitReport)]
    lib.mcgpu_wpc_fit.restype = C.c_int
    p = np.ascontiguousarray(projections, dtype=np.float32)
    if p.ndim != 3:
        raise ValueError(f"projections must be [n, nv, nu], got shape {p.shape}")
    n, nv, nu = p.shape
    if n != len(geometry.gantry_angles):
        raise ValueError(f"{n} projections but {len(geometry.gantry_angles)} geometry entries")
    nx, ny, nz = (int(d) for d in dimension)
    w = np.ascontiguousarray(weight, dtype=np.float32)
    t = np.ascontiguousarray(template, dtype=np.float32)
    if w.shape != (nz, nx) or t.shape != (nz, nx):
        raise ValueError(f"weight and template must be slab means [nz, nx] = {(nz, nx)}, got {w.shape} and {t.shape}")
    order = int(order)
    size = max(order, 0) + 1
    du, dv = float(pixel_spacing[0]), float(pixel_spacing[1])
    u0, v0 = pixel_origin if pixel_origin is not None else (-(nu - 1) / 2 * du, -(nv - 1) / 2 * dv)
    ang = np.ascontiguousarray(geometry.gantry_angles, dtype=np.float64)
    ox = np.ascontiguousarray(geometry.projection_offsets_x, dtype=np.float64)
    oy = np.ascontiguousarray(geometry.projection_offsets_y, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    o = _WpcFitOptions(C.sizeof(_WpcFitOptions), n, nu, nv, du, dv, float(u0), float(v0), float(geometry.source_to_isocenter), float(geometry.source_to_detector),
                       ang.ctypes.data_as(dp), ox.ctypes.data_as(dp), oy.ctypes.data_as(dp), nx, ny, nz, float(spacing[0]), float(spacing[1]), float(spacing[2]),
                       *(tuple(float(v) for v in origin) if origin is not None else (float("nan"),) * 3), float(hann), float(hann_y), float(pad),
                       order, int(slab[0]), int(slab[1]), int(gpu_id), int(channel_layout))
    B = np.zeros((size, size), dtype=np.float64)
    a = np.zeros(size, dtype=np.float64)
    basis = np.zeros((size, nz, nx), dtype=np.float32)
    rep = _WpcFitReport()
    engine._check(lib.mcgpu_wpc_fit(C.byref(o), p.ctypes.data, w.ctypes.data, t.ctypes.data, B.ctypes.data, a.ctypes.data, basis.ctypes.data, C.byref(rep)))
    return B, a, basis, {name: getattr(rep, name) for name, _ in _WpcFitReport._fields_}


def fit_wpc(projections: np.ndarray, geometry: CircularGeometry, pixel_spacing: Tuple[float, float], pixel_origin: Optional[Tuple[float, float]],
            dimension: Tuple[int, int, int], spacing: Tuple[float, float, float], weight: np.ndarray, template: np.ndarray, slab: Tuple[int, int],
            order: int = 5, origin: Optional[Tuple[float, float, float]] = None, hann: float = 1.0, hann_y: float = 1.0, pad: float = 1.0,
            gpu_id: int = 0) -> WPCFit:
    """Fit the water pre-correction polynomial of the given order (1..7) to normalised projections [n, nv, nu] of a water phantom.

    geometry, pixel_spacing, pixel_origin, dimension, spacing, origin, hann, hann_y, pad: as `reconstruction.fdk` takes them (the
    defaults of hann, hann_y and pad are reconstruct_3d's): fit with the settings the polynomial will be used with.
    weight, template: float images [nz, nx] in the FDK volume frame, already averaged over the slab (phantom_weight_and_template).
    slab = (y_first, y_count): the y slices of the volume whose mean the fit sees.

    B grows ill-conditioned with the order (1e9 at order 5 on an analytic cylinder): `condition` says how far the solve can be
    trusted, `residual_fit` <= `residual_identity` holds by optimality whenever it can."""
    B, a, basis, report = normal_equations(projections, geometry, pixel_spacing, pixel_origin, dimension, spacing, weight, template, slab, order, origin,
                                           hann, hann_y, pad, gpu_id)
    c = solve(B, a)
    identity = np.zeros(c.size)
    identity[1] = 1.0
    return WPCFit(coefficients=c, B=B, a=a, condition=float(np.linalg.cond(B)), residual_identity=residual(identity, basis, weight, template),
                  residual_fit=residual(c, basis, weight, template), basis_mean=basis, report=report)


def binary_erosion_cube(mask: np.ndarray, k: int) -> np.ndarray:
    """`scipy.ndimage.binary_erosion(mask, structure=np.ones((k,) * mask.ndim))` in numpy (the package does not import scipy): a voxel
    stays set when every voxel at the offsets -(k // 2) .. k - 1 - k // 2 along every axis is set; outside the array counts as 0.
    The cube is separable: one pass of k shifted ANDs per axis."""
    out = np.asarray(mask).astype(bool)
    k = int(k)
    if k <= 1:
        return out.copy()
    for axis in range(out.ndim):
        n = out.shape[axis]
        src = out
        out = np.ones_like(src)
        for off in range(-(k // 2), k - k // 2):
            shifted = np.zeros_like(src)           # shifted[i] = src[i + off], 0 outside
            lo, hi = max(0, -off), min(n, n - off)
            if hi > lo:
                dst = [slice(None)] * src.ndim
                frm = [slice(None)] * src.ndim
                dst[axis], frm[axis] = slice(lo, hi), slice(lo + off, hi + off)
                shifted[tuple(dst)] = src[tuple(frm)]
            out &= shifted
    return out


def to_fdk_frame(image_xyz: np.ndarray) -> np.ndarray:
    """An [x, y, z] image of an MCGeometry -> [nz][ny][nx] of the FDK volume, by the axis rule of
    forward_projection.prepare_image_for_rtk: IEC X = MC x, IEC Y = -MC z, IEC Z = -MC y."""
    arr = np.rot90(np.asarray(image_xyz), k=1, axes=(0, 1))
    arr = np.swapaxes(arr, 1, 2)
    return np.ascontiguousarray(arr[:, ::-1, :])


def _phantom_images(phantom, n_average_slices, edge_erosion, mu_water, mu_air):
    """(weight, template, eroded-water weight) as float32 slab means [nz, nx] in the FDK frame, and the slab (y_first, y_count)."""
    from .geometry import _cylinder
    materials = np.asarray(phantom.materials)
    shape = materials.shape
    water_mask = materials == material_number("h2o")
    air_mask = materials == material_number("air")
    water = binary_erosion_cube(water_mask, edge_erosion) if edge_erosion else water_mask
    weight = water.astype(np.float32)
    weight[air_mask] = 1
    disk, zsel = _cylinder(shape, tuple(s / 2 for s in shape), shape[0] / 2, n_average_slices)
    fov = disk[:, :, None] & zsel[None, None, :]
    weight = fov * weight
    water_weight = (fov & water).astype(np.float32)
    template = np.zeros(shape, dtype=np.float32)
    template[water_mask] = mu_water
    template[air_mask] = mu_air
    ny = shape[2]
    half = int(n_average_slices) // 2
    first, count = ny // 2 - half, 2 * half
    if first < 0 or count < 1 or first + count > ny:
        raise ValueError(f"{n_average_slices} slices do not fit the phantom's {ny}")
    # means in float64, rounded once (numpy's float32 mean rounds differently along a contiguous and a strided axis)
    means = tuple(to_fdk_frame(v)[:, first: first + count, :].mean(1, dtype=np.float64).astype(np.float32) for v in (weight, template, water_weight))
    return means + ((first, count),)


def phantom_weight_and_template(phantom, n_average_slices: int = 50, edge_erosion: int = 8, mu_water: float = defaults.MU_WATER_63KEV,
                                mu_air: float = defaults.MU_AIR_63KEV):
    """scripts/fit_wpc.py:162-200 for an MCGeometry of water in air (geometry.MCWaterPhantomGeometry): -> (weight [nz, nx], template
    [nz, nx], slab (y_first, y_count)), the arguments of fit_wpc.

    Weight 1 on the water mask eroded by a cube of `edge_erosion` voxels (edge effects stay out) and on air, both inside the
    cylindrical field of view of radius shape[0] / 2 and height `n_average_slices` about the centre; the template holds `mu_water`
    and `mu_air` on the two masks.  Both volumes go to the FDK volume frame by the axis rule of
    forward_projection.prepare_image_for_rtk and are averaged over the slab [ny // 2 - n // 2, ny // 2 + n // 2) of that frame
    (n = n_average_slices; ny = the phantom's z size).

    The script turns its reconstructions back to the phantom's frame with `moveaxis(1, -1)` and `rot90(k=-1)` because the
    reference's reconstruct_3d ends with an `iec61217_to_rsp` step.  This repository's reconstruct_3d has no such step and leaves
    the volume in RTK's IEC frame, so those two calls do NOT apply here: the phantom goes to the volume's frame instead."""
    weight, template, _, slab = _phantom_images(phantom, n_average_slices, edge_erosion, mu_water, mu_air)
    return weight, template, slab


def fit_wpc_phantom(projections_filepath, geometry_filepath, phantom, order: int = 5, n_average_slices: int = 50, edge_erosion: int = 8,
                    mu_water: float = defaults.MU_WATER_63KEV, mu_air: float = defaults.MU_AIR_63KEV, hann: float = 1.0, hann_y: float = 1.0,
                    pad: float = 1.0, gpu_id: int = 0, output_filepath=None) -> WPCFit:
    """Files in, WPCFit out: the normalised projection stack (.mha) and the RTK geometry (.xml) of a scan of `phantom` (an
    MCGeometry, e.g. MCWaterPhantomGeometry(shape=(464, 464, 250)), as scripts/fit_wpc.py simulates it).  The volume is the
    phantom's grid in the FDK frame: dimension (shape[0], shape[2], shape[1]), as the script passes it.  Writes `wpc.yaml` next to
    the projections (or `output_filepath`) with the coefficients, the condition of B, the residuals and the settings.

    rel_diff_before / rel_diff_after: (mean - mu_water) / mu_water of fbar_1 and of the corrected slab image sum_n c_n fbar_n over
    the pixels whose eroded-water weight is 1 (the script's figure over the whole eroded volume is out of scope: no volume exists)."""
    projections_filepath, geometry_filepath = Path(projections_filepath), Path(geometry_filepath)
    proj, pspacing, porigin = read_mha(projections_filepath)
    geometry = CircularGeometry.read(geometry_filepath)
    shape = np.asarray(phantom.materials).shape
    sx, sy, sz = phantom.image_spacing
    dimension, spacing = (shape[0], shape[2], shape[1]), (sx, sz, sy)
    weight, template, water_weight, slab = _phantom_images(phantom, n_average_slices, edge_erosion, mu_water, mu_air)
    fit = fit_wpc(proj, geometry, (pspacing[0], pspacing[1]), (porigin[0], porigin[1]), dimension, spacing, weight, template, slab, order,
                  None, hann, hann_y, pad, gpu_id)
    inside = water_weight == 1
    if inside.any():
        corrected = np.tensordot(fit.coefficients, fit.basis_mean.astype(np.float64), axes=1)
        fit.rel_diff_before = float((fit.basis_mean[1][inside].astype(np.float64).mean() - mu_water) / mu_water)
        fit.rel_diff_after = float((corrected[inside].mean() - mu_water) / mu_water)
    import yaml
    out = Path(output_filepath) if output_filepath else projections_filepath.parent / "wpc.yaml"
    record = dict(wpc=[float(v) for v in fit.coefficients], order=int(order), condition=fit.condition, residual_identity=fit.residual_identity,
                  residual_fit=fit.residual_fit, rel_diff_before=fit.rel_diff_before, rel_diff_after=fit.rel_diff_after,
                  projections=str(projections_filepath), geometry=str(geometry_filepath), dimension=list(int(d) for d in dimension),
                  spacing=[float(s) for s in spacing], slab=[int(slab[0]), int(slab[1])], n_average_slices=int(n_average_slices),
                  edge_erosion=int(edge_erosion), mu_water=float(mu_water), mu_air=float(mu_air), pad=float(pad), hann=float(hann), hannY=float(hann_y),
                  hardware="hip")
    with open(out, "w") as f:
        yaml.dump(record, f)
    return fit
