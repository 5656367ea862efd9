"""FDK reconstruction of projection stacks on the MI355X -- the in-process stand-in for the reference's `rtkfdk` call
(cbctmc/reconstruction/reconstruction.py:22-69 `reconstruct_3d`, reconstructors.py `FDKReconstructor`).

`reconstruct_3d` keeps the reference's signature and file contract: a normalised projection stack (`.mha`, line
integrals), an RTK circular-geometry XML file, `dimension` / `spacing` / `pad` / `hann` / `hann_y` /
`water_pre_correction`, output `recon_fdk3d.mha` + a `.yaml` with the parameters.  `create_geometry` mirrors
cbctmc/forward_projection.py:152-199 without the `itk-rtk` wheel and writes the XML RTK's geometry reader understands.
The arithmetic is `csrc/fdk.hip` through `mcgpu_fdk_reconstruct`; there is no CPU fallback.  Parity against RTK itself is
unpinned (RTK is not available to this repository); the oracle and its analytic pins are in oracle/fdk_oracle.py."""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import defaults


@dataclass
class CircularGeometry:
    """Subset of rtk::ThreeDCircularProjectionGeometry the reference uses (AddProjection(sid, sdd, angle, offx, offy))."""
    source_to_isocenter: float
    source_to_detector: float
    gantry_angles: List[float] = field(default_factory=list)       # degrees
    projection_offsets_x: List[float] = field(default_factory=list)  # mm
    projection_offsets_y: List[float] = field(default_factory=list)

    def add_projection(self, angle: float, offset_x: float = 0.0, offset_y: float = 0.0):
        self.gantry_angles.append(float(angle) % 360.0)
        self.projection_offsets_x.append(float(offset_x))
        self.projection_offsets_y.append(float(offset_y))

    def matrix(self, i: int) -> np.ndarray:
        """3x4 projection matrix of projection i (RTK: translation * magnification * rotation, zero source offsets)."""
        t = np.deg2rad(self.gantry_angles[i])
        c, s = np.cos(t), np.sin(t)
        sid, sdd = self.source_to_isocenter, self.source_to_detector
        rot = np.array([[c, 0.0, -s, 0.0], [0.0, 1.0, 0.0, 0.0], [s, 0.0, c, 0.0], [0.0, 0.0, 0.0, 1.0]])
        mag = np.array([[-sdd, 0.0, 0.0, 0.0], [0.0, -sdd, 0.0, 0.0], [0.0, 0.0, 1.0, -sid]])
        tra = np.array([[1.0, 0.0, -self.projection_offsets_x[i]], [0.0, 1.0, -self.projection_offsets_y[i]], [0.0, 0.0, 1.0]])
        return tra @ mag @ rot

    def write(self, path) -> Path:
        path = Path(path)
        L = ['<?xml version="1.0"?>', "<!DOCTYPE RTKGEOMETRY>", '<RTKThreeDCircularGeometry version="3">',
             f"  <SourceToIsocenterDistance>{self.source_to_isocenter:.17g}</SourceToIsocenterDistance>",
             f"  <SourceToDetectorDistance>{self.source_to_detector:.17g}</SourceToDetectorDistance>"]
        for i, a in enumerate(self.gantry_angles):
            L.append("  <Projection>")
            L.append(f"    <GantryAngle>{a:.17g}</GantryAngle>")
            L.append(f"    <ProjectionOffsetX>{self.projection_offsets_x[i]:.17g}</ProjectionOffsetX>")
            L.append(f"    <ProjectionOffsetY>{self.projection_offsets_y[i]:.17g}</ProjectionOffsetY>")
            m = self.matrix(i)
            L.append("    <Matrix>")
            for row in m:
                L.append("      " + " ".join(f"{v:.15g}" for v in row))
            L.append("    </Matrix>")
            L.append("  </Projection>")
        L.append("</RTKThreeDCircularGeometry>")
        path.write_text("\n".join(L) + "\n")
        return path

    @classmethod
    def read(cls, path) -> "CircularGeometry":
        text = Path(path).read_text()

        def tag(name, s, default=None):
            m = re.search(rf"<{name}>\s*([^<]+?)\s*</{name}>", s)
            return float(m.group(1)) if m else default

        head = text.split("<Projection>")[0]
        sid, sdd = tag("SourceToIsocenterDistance", head), tag("SourceToDetectorDistance", head)
        if sid is None or sdd is None:
            raise ValueError(f"{path}: not an RTK circular geometry file")
        g = cls(sid, sdd)
        gx, gy = tag("ProjectionOffsetX", head, 0.0), tag("ProjectionOffsetY", head, 0.0)  # RTK hoists values shared by all projections
        ga = tag("GantryAngle", head, 0.0)
        for block in text.split("<Projection>")[1:]:
            block = block.split("</Projection>")[0]
            g.add_projection(tag("GantryAngle", block, ga), tag("ProjectionOffsetX", block, gx), tag("ProjectionOffsetY", block, gy))
        return g


def create_geometry(n_projections: int, start_angle: float = 270.0,
                    source_to_isocenter: float = defaults.MCDefaults.source_to_isocenter_distance,
                    source_to_detector: float = defaults.MCDefaults.source_to_detector_distance,
                    detector_offset_x: float = defaults.MCDefaults.detector_lateral_displacement,
                    detector_offset_y: float = 0.0, arc: float = 360.0) -> CircularGeometry:
    """cbctmc/forward_projection.py:152-199 (same arguments and defaults)."""
    g = CircularGeometry(source_to_isocenter, source_to_detector)
    for i in range(n_projections):
        g.add_projection(start_angle + i * arc / n_projections, detector_offset_x, detector_offset_y)
    return g


def save_geometry(geometry: CircularGeometry, output_filepath) -> Path:
    """cbctmc/forward_projection.py:198-205 (`save_geometry(geometry, path)`): RTK circular-geometry XML."""
    return geometry.write(output_filepath)


_DP, _FP = C.POINTER(C.c_double), C.POINTER(C.c_float)


class _FdkOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint), ("n_proj", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("du", C.c_double), ("dv", C.c_double), ("u0", C.c_double), ("v0", C.c_double),
                ("sid", C.c_double), ("sdd", C.c_double), ("gantry_deg", C.POINTER(C.c_double)), ("proj_offset_x", C.POINTER(C.c_double)),
                ("proj_offset_y", C.POINTER(C.c_double)), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("sx", C.c_double), ("sy", C.c_double),
                ("sz", C.c_double), ("ox", C.c_double), ("oy", C.c_double), ("oz", C.c_double), ("hann", C.c_double), ("hann_y", C.c_double),
                ("wpc", C.POINTER(C.c_double)), ("n_wpc", C.c_int), ("device", C.c_int), ("pad", C.c_double)]


class _FdkReport(C.Structure):
    _fields_ = [("ms_filter", C.c_double), ("ms_backproject", C.c_double)]


_bound = None  # the library whose prototypes _library() has declared


def _library():
    """The engine's library with the prototypes of this module's entry points declared, once per loaded library."""
    global _bound
    from . import engine
    lib = engine.load_library()
    if lib is not _bound:
        P, vp, ci = C.POINTER, C.c_void_p, C.c_int
        fo, ro, rm, rr, rmr = P(_FdkOptions), P(_RoosterOptions), P(_RoosterMotion), P(_RoosterReport), P(_RoosterMotionReport)
        for name, argtypes in dict(mcgpu_fdk_reconstruct=[fo, vp, vp, P(_FdkReport)], mcgpu_fdk_reconstruct_motion=[fo, P(_FdkMotion), vp, vp, P(_FdkMotionReport)],
                                   mcgpu_rooster4d_reconstruct=[ro, vp, vp, rr], mcgpu_rooster4d_stage=[ro, ci, vp, vp, rr],
                                   mcgpu_rooster4d_reconstruct_motion=[ro, rm, vp, vp, rmr], mcgpu_rooster4d_motion_stage=[ro, rm, ci, vp, vp, rmr]).items():
            getattr(lib, name).argtypes, getattr(lib, name).restype = argtypes, ci
        _bound = lib
    return lib


def _report_dict(rep) -> dict:
    return {name: getattr(rep, name) for name, _ in rep._fields_}


def _volume(dimension, frames=None) -> np.ndarray:
    """Zeros [nz, ny, nx], or [frames, nz, ny, nx], float32."""
    shape = (int(dimension[2]), int(dimension[1]), int(dimension[0]))
    return np.zeros(shape if frames is None else (int(frames),) + shape, dtype=np.float32)


def _geometry_fields(n, nu, nv, geometry, pixel_spacing, pixel_origin, dimension, spacing, origin):
    """What mcgpu_fdk_options and mcgpu_rooster4d_options share: the 21 fields n_proj .. oz that follow struct_size, in order, and the
    arrays they point into.  No pixel origin: the detector is centred; no volume origin: NaN, which the library reads as centred."""
    if n != len(geometry.gantry_angles):
        raise ValueError(f"{n} projections but {len(geometry.gantry_angles)} geometry entries")
    du, dv = float(pixel_spacing[0]), float(pixel_spacing[1])
    u0, v0 = pixel_origin if pixel_origin is not None else (-(nu - 1) / 2 * du, -(nv - 1) / 2 * dv)
    arrays = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (geometry.gantry_angles, geometry.projection_offsets_x, geometry.projection_offsets_y))
    fields = (int(n), int(nu), int(nv), du, dv, float(u0), float(v0), float(geometry.source_to_isocenter), float(geometry.source_to_detector),
              *(a.ctypes.data_as(_DP) for a in arrays), int(dimension[0]), int(dimension[1]), int(dimension[2]),
              float(spacing[0]), float(spacing[1]), float(spacing[2]), *(tuple(float(v) for v in origin) if origin is not None else (float("nan"),) * 3))
    return fields, arrays


def fdk(projections: np.ndarray, geometry: CircularGeometry, pixel_spacing: Tuple[float, float], pixel_origin: Optional[Tuple[float, float]] = None,
        dimension: Tuple[int, int, int] = (464, 250, 464), spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0),
        origin: Optional[Tuple[float, float, float]] = None, hann: float = 0.0, hann_y: float = 0.0,
        water_pre_correction: Optional[Sequence[float]] = None, gpu_id: int = 0, pad: float = 0.0):
    """projections [n, nv, nu] (line integrals) -> (volume [nz, ny, nx] float32 in RTK's IEC frame, report dict).
    pad: rtkfdk --pad, the truncation correction of RTK's ramp filter (0 = rows are zero-padded only).  It follows the published
    heuristic only: the exact extent / weight table of RTK's FFTProjectionsConvolutionImageFilter (floor vs ceil of pad x width, the
    mirror limited by the zero extension) could not be checked against RTK here -- on a truncated half-fan scan the feathered edge
    may differ from rtkfdk's (parity unpinned)."""
    from . import engine
    lib = _library()
    p, o, keep = _fdk_options(projections, geometry, pixel_spacing, pixel_origin, dimension, spacing, origin, hann, hann_y, water_pre_correction, gpu_id, pad)
    vol, rep = _volume(dimension), _FdkReport()
    engine._check(lib.mcgpu_fdk_reconstruct(C.byref(o), p.ctypes.data, vol.ctypes.data, C.byref(rep)))
    return vol, _report_dict(rep)


def _fdk_options(projections, geometry, pixel_spacing, pixel_origin, dimension, spacing, origin, hann, hann_y, water_pre_correction, gpu_id, pad):
    """(float32 stack, mcgpu_fdk_options, the arrays it points into) of fdk() and fdk_motion()."""
    p = np.ascontiguousarray(projections, dtype=np.float32)
    n, nv, nu = p.shape
    fields, arrays = _geometry_fields(n, nu, nv, geometry, pixel_spacing, pixel_origin, dimension, spacing, origin)
    wpc = np.ascontiguousarray(water_pre_correction if water_pre_correction is not None else [], dtype=np.float64)
    o = _FdkOptions(C.sizeof(_FdkOptions), *fields, float(hann), float(hann_y), wpc.ctypes.data_as(_DP) if wpc.size else None, int(wpc.size), int(gpu_id),
                    float(pad))
    return p, o, arrays + (wpc,)


# ------------------------------------------------------------------------------------------------ motion-compensated FDK
MAX_SIGNAL_DIMS = 4


class _FdkMotion(C.Structure):
    """mcgpu_fdk_motion (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_signal_dims", C.c_int), ("mean", C.POINTER(C.c_float)), ("coefficients", C.POINTER(C.c_float)),
                ("delta", C.POINTER(C.c_double))]


class _FdkMotionReport(C.Structure):
    _fields_ = [("ms_filter", C.c_double), ("ms_backproject", C.c_double), ("ms_upload_model", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


class MotionModel:
    """A linear motion model on the FDK grid: mean [3, nz, ny, nx], coefficients [K, 3, nz, ny, nx] (both float32) and mean_signal
    [K] float64.  csrc/motion_model.inc states the layout and the displacement rule; what a displacement means is its user's
    (fdk_motion: where the material of a reference-phase voxel is; rooster4d_motion: one model each way).  dimension = (nx, ny, nz);
    spacing (mm, optional) is what from_correspondence_model derived the grid's from, and fdk_motion refuses another one."""

    def __init__(self, mean, coefficients, mean_signal, spacing=None):
        self.mean = np.ascontiguousarray(mean, dtype=np.float32)
        self.coefficients = np.ascontiguousarray(coefficients, dtype=np.float32)
        self.mean_signal = np.asarray(mean_signal, dtype=np.float64).reshape(-1)
        self.spacing = tuple(float(v) for v in spacing) if spacing is not None else None
        if self.mean.ndim != 4 or self.mean.shape[0] != 3:
            raise ValueError(f"mean of shape {self.mean.shape}, expected (3, nz, ny, nx)")
        if self.coefficients.ndim != 5 or self.coefficients.shape[1:] != self.mean.shape:
            raise ValueError(f"coefficients of shape {self.coefficients.shape}, expected (K, 3, nz, ny, nx) on the grid of mean")
        if not 1 <= self.n_signal_dims <= MAX_SIGNAL_DIMS:
            raise ValueError(f"{self.n_signal_dims} signal dimensions: 1 to {MAX_SIGNAL_DIMS} are supported")
        if self.mean_signal.size != self.n_signal_dims:
            raise ValueError(f"{self.mean_signal.size} mean signal values for {self.n_signal_dims} signal dimensions")

    @property
    def n_signal_dims(self) -> int:
        return int(self.coefficients.shape[0])

    @property
    def dimension(self) -> Tuple[int, int, int]:
        return tuple(int(n) for n in self.mean.shape[:0:-1])

    def pointers(self):
        """(mean, coefficients) as the float pointers of mcgpu_fdk_motion and mcgpu_rooster4d_motion."""
        return self.mean.ctypes.data_as(_FP), self.coefficients.ctypes.data_as(_FP)

    def check_grid(self, dimension, spacing):
        """ValueError unless (dimension, spacing) is the grid the model lives on: a model is not resampled."""
        if tuple(int(n) for n in dimension) != self.dimension:
            raise ValueError(f"the motion model lives on the grid {self.dimension}, the reconstruction on {tuple(dimension)}: resample the model first")
        if self.spacing is not None and not np.allclose(self.spacing, [float(v) for v in spacing], rtol=1e-9, atol=0.0):
            raise ValueError(f"the motion model's grid has spacing {self.spacing} mm, the reconstruction {tuple(spacing)}: resample the model first")

    def delta(self, signals) -> np.ndarray:
        """signals [n, K] -> float64 [n, K]: signal - mean_signal, what mcgpu_fdk_motion.delta takes."""
        s = np.asarray(signals, dtype=np.float64)
        if s.ndim == 1:
            s = s[:, None]
        if s.ndim != 2 or s.shape[1] != self.n_signal_dims:
            raise ValueError(f"signals of shape {np.shape(signals)}, expected (n, {self.n_signal_dims})")
        return np.ascontiguousarray(s - self.mean_signal[None, :])

    @classmethod
    def from_correspondence_model(cls, model, voxel_spacing_mm, dimension=None, spacing=None) -> "MotionModel":
        """A fitted `CorrespondenceModel` -> the model in the FDK frame.

        DIRECTION.  The model must take a voxel of the reference phase to the place of its material at a state: build it with
        `CorrespondenceModel.build_default(..., inverse=True)`.  The default `build_default` gives pull-back fields (ref(x + u_t(x))
        ~ phase_t(x)), the inverse of what is needed; such a model is NOT detected and NOT silently inverted here -- the
        reconstruction it drives is blurred more, not less.

        The model's fields are [3, gx, gy, gz] in voxel units in the MCGeometry frame, voxel_spacing_mm = (sx, sy, sz) of that
        geometry.  Arrays go through the axis rule of `water_precorrection.to_fdk_frame` (IEC X = MC x, IEC Y = -MC z, IEC Z = -MC y),
        components are permuted, signed and scaled accordingly, (ux sx, -uz sz, -uy sy), in float64, and then rounded to float32;
        the coefficients likewise.  The result lives on the grid dimension (gx, gz, gy), spacing (sx, sz, sy); with `dimension` /
        `spacing` given (the reconstruction's) anything else raises ValueError -- a model is not resampled onto another grid."""
        from .water_precorrection import to_fdk_frame
        if not model.is_fitted:
            raise RuntimeError("Correspondence model is not fitted")
        sx, sy, sz = (float(v) for v in voxel_spacing_mm)
        shape = tuple(int(n) for n in model.spatial_shape)
        k_dims = int(model.signal_n_dims)
        grid_dimension, grid_spacing = (shape[0], shape[2], shape[1]), (sx, sz, sy)
        if dimension is not None and tuple(int(n) for n in dimension) != grid_dimension:
            raise ValueError(f"the correspondence model gives the FDK grid {grid_dimension}, the reconstruction has {tuple(dimension)}: resample the model first")
        if spacing is not None and not np.allclose(grid_spacing, [float(v) for v in spacing], rtol=1e-9, atol=0.0):
            raise ValueError(f"the correspondence model gives the FDK spacing {grid_spacing} mm, the reconstruction has {tuple(spacing)}: resample the model first")

        def convert(field):  # [3, gx, gy, gz] voxels -> [3, nz, ny, nx] mm
            field = np.asarray(field, dtype=np.float64)
            return np.stack([to_fdk_frame(field[0] * sx), to_fdk_frame(-field[2] * sz), to_fdk_frame(-field[1] * sy)]).astype(np.float32)

        mean = convert(np.asarray(model.mean_vector_field).reshape(3, *shape))
        coefficients = np.asarray(model.coefficients).reshape(3, *shape, k_dims)
        coefficients = np.stack([convert(coefficients[..., k]) for k in range(k_dims)])
        return cls(mean, coefficients, np.asarray(model.mean_signal, dtype=np.float64).reshape(-1), spacing=grid_spacing)


def fdk_motion(projections: np.ndarray, geometry: CircularGeometry, pixel_spacing: Tuple[float, float], pixel_origin: Optional[Tuple[float, float]],
               motion: MotionModel, signals, dimension: Tuple[int, int, int], spacing: Tuple[float, float, float],
               origin: Optional[Tuple[float, float, float]] = None, hann: float = 0.0, hann_y: float = 0.0,
               water_pre_correction: Optional[Sequence[float]] = None, gpu_id: int = 0, pad: float = 0.0):
    """Motion-compensated FDK (Rit et al. 2009; RTK's FDKWarpBackProjectionImageFilter, `rtkfdk --signal --dvf`): fdk() with every
    projection back-projected along the trajectories `motion` predicts for its breathing state, so that all projections sharpen one
    volume at the reference phase.  projections [n, nv, nu], signals [n, K] (one row per projection) -> (volume [nz, ny, nx]
    float32, report dict: ms_filter, ms_backproject, ms_upload_model, peak_device_bytes).  The filter chain and every other argument
    are those of fdk(); the arithmetic is csrc/fdk.hip: backproject_motion_kernel, whose header states the rule.  `motion` must
    live on the reconstruction grid (ValueError otherwise) and map the reference phase forward (MotionModel.from_correspondence_model).
    Parity against RTK's warp back-projector is unpinned (RTK is absent here); tests/fdk_motion_ref.py restates the rule in float64."""
    from . import engine
    lib = _library()
    motion.check_grid(dimension, spacing)
    p, o, keep = _fdk_options(projections, geometry, pixel_spacing, pixel_origin, dimension, spacing, origin, hann, hann_y, water_pre_correction, gpu_id, pad)
    delta = motion.delta(signals)
    if delta.shape[0] != p.shape[0]:
        raise ValueError(f"{p.shape[0]} projections but {delta.shape[0]} signals")
    if not np.isfinite(delta).all():
        raise ValueError("the signals are not finite")
    m = _FdkMotion(C.sizeof(_FdkMotion), motion.n_signal_dims, *motion.pointers(), delta.ctypes.data_as(_DP))
    vol, rep = _volume(dimension), _FdkMotionReport()
    engine._check(lib.mcgpu_fdk_reconstruct_motion(C.byref(o), C.byref(m), p.ctypes.data, vol.ctypes.data, C.byref(rep)))
    return vol, _report_dict(rep)


_MHA_ELEMENT_TYPES = {"MET_FLOAT": "<f4", "MET_SHORT": "<i2", "MET_UCHAR": "u1"}


def read_mha(path):
    """(array [n2, n1, n0], spacing, origin) of an uncompressed MetaImage written by this engine or SimpleITK; a 4-D
    image gives [n3, n2, n1, n0] and 4 spacings and offsets.  MET_FLOAT gives float32 (stacks, reconstructions), MET_SHORT int16
    (CT images) and MET_UCHAR uint8 (segmentations)."""
    raw = Path(path).read_bytes()
    head_end = raw.index(b"ElementDataFile")
    head_end = raw.index(b"\n", head_end) + 1
    meta = {}
    for line in raw[:head_end].decode("latin-1").splitlines():
        if "=" in line:
            k, v = line.split("=", 1)
            meta[k.strip()] = v.strip()
    if (meta.get("ElementDataFile") != "LOCAL" or meta.get("ElementType") not in _MHA_ELEMENT_TYPES or meta.get("CompressedData", "False") == "True"
            or meta.get("BinaryDataByteOrderMSB", "False") == "True"):
        raise ValueError(f"{path}: only uncompressed little-endian MET_FLOAT / MET_SHORT / MET_UCHAR MetaImages with local data are supported")
    dims = [int(v) for v in meta["DimSize"].split()]
    spacing = [float(v) for v in meta.get("ElementSpacing", "1 1 1").split()]
    origin = [float(v) for v in meta.get("Offset", meta.get("Origin", "0 0 0")).split()]
    data = np.frombuffer(raw, dtype=_MHA_ELEMENT_TYPES[meta["ElementType"]], offset=head_end, count=int(np.prod(dims))).reshape(dims[::-1])
    return data, spacing, origin


def write_mha(path, volume: np.ndarray, spacing, origin, element_type: str = "MET_FLOAT") -> Path:
    """float32 [n2, n1, n0] -> uncompressed MetaImage (what SimpleITK.WriteImage produces for such an image).  A 4-D array
    [n3, n2, n1, n0] (e.g. the frames of reconstruct_4d) is written with NDims = 4; spacing and origin then have 4 entries.
    element_type "MET_SHORT" / "MET_UCHAR" writes int16 / uint8 elements (CT images, segmentations)."""
    path = Path(path)
    v = np.ascontiguousarray(volume, dtype=_MHA_ELEMENT_TYPES[element_type])
    d = v.shape[::-1]
    if v.ndim == 3:
        head = ("ObjectType = Image\nNDims = 3\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = False\n"
                "TransformMatrix = 1 0 0 0 1 0 0 0 1\n"
                f"Offset = {origin[0]:.15g} {origin[1]:.15g} {origin[2]:.15g}\nCenterOfRotation = 0 0 0\nAnatomicalOrientation = RAI\n"
                f"ElementSpacing = {spacing[0]:.15g} {spacing[1]:.15g} {spacing[2]:.15g}\nDimSize = {d[0]} {d[1]} {d[2]}\n"
                f"ElementType = {element_type}\nElementDataFile = LOCAL\n")
    elif v.ndim == 4:
        if len(spacing) != 4 or len(origin) != 4:
            raise ValueError("a 4-D MetaImage needs 4 spacings and 4 offsets")
        eye = " ".join("1" if i == j else "0" for i in range(4) for j in range(4))
        head = ("ObjectType = Image\nNDims = 4\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = False\n"
                f"TransformMatrix = {eye}\nOffset = {' '.join(f'{float(o):.15g}' for o in origin)}\nCenterOfRotation = 0 0 0 0\n"
                f"ElementSpacing = {' '.join(f'{float(x):.15g}' for x in spacing)}\nDimSize = {' '.join(str(n) for n in d)}\n"
                f"ElementType = {element_type}\nElementDataFile = LOCAL\n")
    else:
        raise ValueError(f"write_mha: {v.ndim}-D arrays are not supported (3 or 4)")
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(v.tobytes())
    return path


def _reconstruct_to_file(projections_filepath, geometry_filepath, output_folder, output_filename, dimension, spacing, water_pre_correction, compute, record):
    """The file flow of the four reconstruct_* functions: stack (.mha) + RTK geometry (.xml) in; compute(projections, geometry, pixel
    spacing, pixel origin) -> (volume, report); the volume out at the centred origin (a 4-D one with spacing 1 and offset 0 along
    the frames) and, next to it, a .yaml of what every flow records plus `record`.  -> (path of the volume, report)."""
    projections_filepath, geometry_filepath = Path(projections_filepath), Path(geometry_filepath)
    output_folder = Path(output_folder) if output_folder else projections_filepath.parent / "reconstructions"
    out = output_folder / output_filename
    output_folder.mkdir(parents=True, exist_ok=True)
    proj, pspacing, porigin = read_mha(projections_filepath)
    geometry = CircularGeometry.read(geometry_filepath)
    vol, report = compute(proj, geometry, (pspacing[0], pspacing[1]), (porigin[0], porigin[1]))
    origin = tuple(-(n - 1) / 2 * s for n, s in zip(dimension, spacing))
    if vol.ndim == 4:
        write_mha(out, vol, tuple(spacing) + (1.0,), origin + (0.0,))
    else:
        write_mha(out, vol, spacing, origin)
    import yaml
    with open(out.with_suffix(".yaml"), "w") as f:
        yaml.dump(dict(path=str(projections_filepath.parent), regexp=projections_filepath.name, geometry=str(geometry_filepath), hardware="hip",
                       dimension=list(dimension), spacing=list(spacing), wpc=list(water_pre_correction) if water_pre_correction is not None else None,
                       output_filepath=str(out), **record), f)
    return out, report


def reconstruct_3d(projections_filepath, geometry_filepath, output_folder=None, output_filename: Optional[str] = None,
                   dimension: Tuple[int, int, int] = (464, 250, 464), spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0), pad: float = 1.0,
                   hann: float = 1.0, hann_y: float = 1.0, water_pre_correction: Optional[Sequence[float]] = None, gpu_id: int = 0, **kwargs):
    """cbctmc/reconstruction/reconstruction.py:22-69 with `rtkfdk --hardware cuda` replaced by the in-process kernels.
    What each stage restates of `rtkfdk` with the options the reference passes (reconstruction.py:52-66): `--wpc` =
    rtk::WaterPrecorrectionImageFilter (polynomial in the line integral); displaced detector =
    rtk::DisplacedDetectorImageFilter (Wang weights + padding to a detector symmetric about the central ray); cosine and
    angular weights = rtk::FDKWeightProjectionFilter (angular gaps from the geometry file, as here); ramp =
    rtk::FFTRampImageFilter with `--hann` / `--hannY` windows; back-projection = rtk::FDKBackProjectionImageFilter
    (voxel-driven, bilinear); `--short 360` leaves rtk::ParkerShortScanImageFilter inactive for a full arc.
    `--pad` = the TruncationCorrection of rtk::FFTRampImageFilter (Ohnesorge's heuristic: rows continued by `pad` x width
    columns with the feathered point reflection of the data before the ramp; csrc/fdk.hip: extend_rows_kernel, restated in
    oracle/fdk_oracle.py: truncation_extension).  Parity against RTK itself is unpinned (RTK is absent here; DESIGN.md
    section 2): the restatement is pinned by an analytic truncated cylinder (tests/test_fdk.py)."""
    return _reconstruct_to_file(
        projections_filepath, geometry_filepath, output_folder, output_filename or "recon_fdk3d.mha", dimension, spacing, water_pre_correction,
        lambda proj, geometry, ds, org: fdk(proj, geometry, ds, org, dimension, spacing, None, hann, hann_y, water_pre_correction, gpu_id, pad=pad),
        dict(pad=pad, hann=hann, hannY=hann_y, short=360, **kwargs))


def reconstruct_3d_mc(projections_filepath, geometry_filepath, correspondence_model, signals, voxel_spacing_mm, output_folder=None,
                      output_filename: Optional[str] = None, dimension: Tuple[int, int, int] = (464, 250, 464),
                      spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0), pad: float = 1.0, hann: float = 1.0, hann_y: float = 1.0,
                      water_pre_correction: Optional[Sequence[float]] = None, gpu_id: int = 0, **kwargs):
    """reconstruct_3d with the motion of a fitted `CorrespondenceModel` compensated (fdk_motion): same defaults, same file flow.
    correspondence_model: built with `build_default(..., inverse=True)` on the reconstruction grid (see
    MotionModel.from_correspondence_model for the direction and the frame); voxel_spacing_mm: the spacing of the MCGeometry its
    fields live on; signals [n, K]: the breathing signal of every projection, in the model's units.  Writes `recon_fdk3d_mc.mha`
    and a .yaml that also records `motion` (the first 7 hex digits of the model's hash) and `signal_n_dims` (K)."""
    motion = MotionModel.from_correspondence_model(correspondence_model, voxel_spacing_mm, dimension=dimension, spacing=spacing)
    return _reconstruct_to_file(
        projections_filepath, geometry_filepath, output_folder, output_filename or "recon_fdk3d_mc.mha", dimension, spacing, water_pre_correction,
        lambda proj, geometry, ds, org: fdk_motion(proj, geometry, ds, org, motion, signals, dimension, spacing, None, hann, hann_y, water_pre_correction,
                                                   gpu_id, pad=pad),
        dict(pad=pad, hann=hann, hannY=hann_y, short=360, motion=correspondence_model.model_hash[:7], signal_n_dims=motion.n_signal_dims, **kwargs))


# ---------------------------------------------------------------------------------------------------------------- 4-D ROOSTER
class _RoosterOptions(C.Structure):
    """mcgpu_rooster4d_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_proj", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("du", C.c_double), ("dv", C.c_double),
                ("u0", C.c_double), ("v0", C.c_double), ("sid", C.c_double), ("sdd", C.c_double), ("gantry_deg", C.POINTER(C.c_double)),
                ("proj_offset_x", C.POINTER(C.c_double)), ("proj_offset_y", C.POINTER(C.c_double)), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("sx", C.c_double), ("sy", C.c_double), ("sz", C.c_double), ("ox", C.c_double), ("oy", C.c_double), ("oz", C.c_double),
                ("n_frames", C.c_int), ("phase", C.POINTER(C.c_double)), ("niter", C.c_int), ("cgiter", C.c_int), ("tviter", C.c_int),
                ("gamma_space", C.c_double), ("gamma_time", C.c_double), ("positivity", C.c_int), ("wpc", C.POINTER(C.c_double)),
                ("n_wpc", C.c_int), ("device", C.c_int), ("residuals", C.POINTER(C.c_double))]


class _RoosterReport(C.Structure):
    _fields_ = [("ms_forward", C.c_double), ("ms_back", C.c_double), ("ms_cg_vectors", C.c_double), ("ms_tv_space", C.c_double),
                ("ms_tv_time", C.c_double), ("ms_upload", C.c_double), ("ms_total", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


ROOSTER4D_STAGES = {"forward": 0, "back": 1, "tv_space": 2, "tv_time": 3}


def _rooster_call(n_proj, nu, nv, geometry, pixel_spacing, pixel_origin, phase, dimension, spacing, origin, frames, niter, cgiter, tviter,
                  gamma_time, gamma_space, water_pre_correction, positivity, gpu_id):
    """(library, options, the arrays it points into) for mcgpu_rooster4d_*."""
    lib = _library()
    fields, arrays = _geometry_fields(n_proj, nu, nv, geometry, pixel_spacing, pixel_origin, dimension, spacing, origin)
    ph = np.ascontiguousarray(phase, dtype=np.float64).ravel()
    if ph.size != n_proj:
        raise ValueError(f"{n_proj} projections but {ph.size} phase values")
    keep = dict(geometry=arrays, phase=ph, wpc=np.ascontiguousarray(water_pre_correction if water_pre_correction is not None else [], dtype=np.float64),
                residuals=np.zeros(max(int(niter), 0) * (max(int(cgiter), 0) + 1), dtype=np.float64))
    o = _RoosterOptions(C.sizeof(_RoosterOptions), *fields, int(frames), ph.ctypes.data_as(_DP), int(niter), int(cgiter), int(tviter), float(gamma_space),
                        float(gamma_time), int(bool(positivity)), keep["wpc"].ctypes.data_as(_DP) if keep["wpc"].size else None, int(keep["wpc"].size),
                        int(gpu_id), keep["residuals"].ctypes.data_as(_DP) if keep["residuals"].size else None)
    return lib, o, keep


def _rooster_result(rep, keep, niter, cgiter, **more) -> dict:
    """The report dict of a whole reconstruction: the report's fields, residuals [niter][cgiter + 1] and `more`."""
    return dict(_report_dict(rep), residuals=keep["residuals"].reshape(max(int(niter), 0), max(int(cgiter), 0) + 1).copy(), **more)


def rooster4d(projections: np.ndarray, geometry: CircularGeometry, pixel_spacing: Tuple[float, float], pixel_origin: Optional[Tuple[float, float]],
              phase: Sequence[float], dimension: Tuple[int, int, int] = (464, 250, 464), spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0),
              origin: Optional[Tuple[float, float, float]] = None, frames: int = 10, niter: int = 10, cgiter: int = 4, tviter: int = 10,
              gamma_time: float = 0.0002, gamma_space: float = 0.00007, water_pre_correction: Optional[Sequence[float]] = None,
              positivity: bool = True, gpu_id: int = 0):
    """4-D ROOSTER (csrc/rooster4d.hip, whose header spells out the algorithm; what `rtkfourdrooster` computes for the reference):
    projections [n, nv, nu] (line integrals), phase [n] in [0, 1] -> (volume [frames, nz, ny, nx] float32 in RTK's IEC frame on
    the FDK grid, report dict).

    Frame f of the result is the volume at phase f / frames; a projection at phase phi sees the linear blend of frames
    floor(phi N) mod N and the next one (periodic).  Each of `niter` main iterations runs `cgiter` conjugate-gradient steps on
    S^T B R S x = S^T B p from the current x (R = the Joseph forward projector, B = a voxel-driven back-projector weighted to be
    close to R^T, S = the phase interpolation), then x = max(x, 0) when `positivity`, then `tviter` iterations of spatial TV
    denoising (gamma_space, per frame) and of temporal TV denoising (gamma_time, per voxel, periodic).  `water_pre_correction`
    is rtkfdk's --wpc polynomial, applied to the projections first.  frames = 10 is taken to be rtkfourdrooster's --frames
    default; that could not be confirmed here (neither RTK nor its documentation is available).  Parity against RTK itself is
    unpinned; tests/rooster_ref.py restates the algorithm in float64.

    report: ms per stage (ms_forward, ms_back, ms_cg_vectors, ms_tv_space, ms_tv_time, ms_upload, ms_total), peak_device_bytes,
    and residuals [niter][cgiter + 1] (|r| at each CG restart and after each CG step)."""
    from . import engine
    p = np.ascontiguousarray(projections, dtype=np.float32)
    n, nv, nu = p.shape
    lib, o, keep = _rooster_call(n, nu, nv, geometry, pixel_spacing, pixel_origin, phase, dimension, spacing, origin, frames, niter, cgiter, tviter,
                                 gamma_time, gamma_space, water_pre_correction, positivity, gpu_id)
    vol, rep = _volume(dimension, frames), _RoosterReport()
    engine._check(lib.mcgpu_rooster4d_reconstruct(C.byref(o), p.ctypes.data, vol.ctypes.data, C.byref(rep)))
    return vol, _rooster_result(rep, keep, niter, cgiter)


def rooster4d_stage(stage: str, data: np.ndarray, geometry: CircularGeometry, detector: Tuple[int, int], pixel_spacing, pixel_origin, phase,
                    dimension, spacing, origin=None, frames: int = 10, tviter: int = 10, gamma_time: float = 0.0002, gamma_space: float = 0.00007,
                    gpu_id: int = 0):
    """One operator of rooster4d alone (mcgpu_rooster4d_stage): 'forward' (R S: [frames, nz, ny, nx] -> [n, nv, nu]), 'back'
    (S^T B: projections -> 4-D), 'tv_space' / 'tv_time' (4-D -> 4-D, `tviter` iterations).  detector = (nu, nv)."""
    from . import engine
    nu, nv = int(detector[0]), int(detector[1])
    n = len(geometry.gantry_angles)
    lib, o, keep = _rooster_call(n, nu, nv, geometry, pixel_spacing, pixel_origin, phase, dimension, spacing, origin, frames, 0, 0, tviter,
                                 gamma_time, gamma_space, None, True, gpu_id)
    shape4 = (int(frames), int(dimension[2]), int(dimension[1]), int(dimension[0]))
    code = ROOSTER4D_STAGES[stage]
    src = np.ascontiguousarray(data, dtype=np.float32)
    if src.shape != ((n, nv, nu) if stage == "back" else shape4):
        raise ValueError(f"rooster4d_stage {stage}: input shape {src.shape}")
    out, rep = np.zeros((n, nv, nu) if stage == "forward" else shape4, dtype=np.float32), _RoosterReport()
    engine._check(lib.mcgpu_rooster4d_stage(C.byref(o), code, src.ctypes.data, out.ctypes.data, C.byref(rep)))
    return out, _report_dict(rep)


def _unit_phase(amplitude_signal, phase_signal) -> np.ndarray:
    """The phase of reconstruct_4d and reconstruct_4d_mc: exactly one of the two signals is given (ValueError otherwise); an
    amplitude goes through phase.calculate_phase; the phase is min-max scaled to [0, 1]."""
    from . import phase as phase_mod
    if (amplitude_signal is None) == (phase_signal is None):
        raise ValueError("give exactly one of amplitude_signal and phase_signal")
    if phase_signal is None:
        phase_signal = np.hstack(phase_mod.calculate_phase(np.asarray(amplitude_signal)))
    ph = np.array(phase_signal, dtype=np.float64)
    ph -= ph.min()
    span = ph.max()
    if not span > 0:
        raise ValueError("the phase signal is constant: it cannot be scaled to [0, 1]")
    return ph / span


def reconstruct_4d(projections_filepath, geometry_filepath, output_folder=None, output_filename: Optional[str] = None,
                   dimension: Tuple[int, int, int] = (464, 250, 464), spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0),
                   amplitude_signal: Optional[np.ndarray] = None, phase_signal: Optional[np.ndarray] = None,
                   water_pre_correction: Optional[Sequence[float]] = None, gpu_id: int = 0, extract_signal: bool = False,
                   shroud: Optional[dict] = None, **kwargs):
    """cbctmc/reconstruction/reconstruction.py:72-125 with `rtkfourdrooster` replaced by the in-process kernels (rooster4d).
    Exactly one of `amplitude_signal` (one breathing amplitude per projection; its phase comes from phase.calculate_phase) and
    `phase_signal` is given, else ValueError.  The phase is min-max scaled to [0, 1] as the reference does before it hands the
    signal to RTK (reconstructors.py:150-151).  The reference's parameters: niter 10, cgiter 4, tviter 10, gamma_time 0.0002,
    gamma_space 0.00007 (keyword arguments override them, as do `frames` and `positivity`).  Writes `recon_rooster4d.mha`, a 4-D
    MetaImage [frames][nz][ny][nx] with spacing (sx, sy, sz, 1) and offset (ox, oy, oz, 0) in the frame of reconstruct_3d's
    output, and a .yaml of the parameters next to it (fp / bp record what ran: Joseph / VoxelBased).

    extract_signal=True takes the amplitude from the projections themselves, `shroud.extract_signal(projections, **(shroud or {}))`
    (the Amsterdam shroud; its amplitude is not calibrated, which the phase does not need), and neither signal may then be given
    (ValueError); the .yaml records `signal: shroud` and the extraction parameters under `shroud`."""
    from . import shroud as shroud_mod
    if extract_signal and (amplitude_signal is not None or phase_signal is not None):
        raise ValueError("extract_signal=True takes the signal from the projections: give neither amplitude_signal nor phase_signal")
    ph = None if extract_signal else _unit_phase(amplitude_signal, phase_signal)
    params = _rooster_parameters(kwargs)
    shroud_parameters = {"gpu_id": gpu_id, **(shroud or {})}

    def compute(proj, geometry, ds, org):
        phase = _unit_phase(shroud_mod.extract_signal(proj, **shroud_parameters), None) if extract_signal else ph
        return rooster4d(proj, geometry, ds, org, phase, dimension, spacing, None, water_pre_correction=water_pre_correction, gpu_id=gpu_id, **params)

    record = {}
    if extract_signal:  # what ran, the defaults included
        import inspect
        defaults = {k: p.default for k, p in inspect.signature(shroud_mod.extract_signal).parameters.items() if p.default is not inspect.Parameter.empty}
        unknown = set(shroud_parameters) - set(defaults)
        if unknown:
            raise ValueError(f"shroud: unknown extraction parameters {sorted(unknown)}")
        record = dict(signal="shroud", shroud={k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in {**defaults, **shroud_parameters}.items()})
    return _reconstruct_to_file(projections_filepath, geometry_filepath, output_folder, output_filename or "recon_rooster4d.mha", dimension, spacing,
                                water_pre_correction, compute, dict(fp="Joseph", bp="VoxelBased", **params, **record, **kwargs))


def _rooster_parameters(kwargs) -> dict:
    """The reference's ROOSTER parameters, each replaced by the keyword argument of its name, which is taken out of `kwargs`."""
    params = dict(niter=10, cgiter=4, tviter=10, gamma_time=0.0002, gamma_space=0.00007, frames=10, positivity=True)
    params.update({k: kwargs.pop(k) for k in list(kwargs) if k in params})
    return params


# ------------------------------------------------------------------------------------------------ motion-aware 4-D ROOSTER
class _RoosterMotion(C.Structure):
    """mcgpu_rooster4d_motion (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n_signal_dims", C.c_int), ("to_reference_mean", C.POINTER(C.c_float)),
                ("to_reference_coefficients", C.POINTER(C.c_float)), ("from_reference_mean", C.POINTER(C.c_float)),
                ("from_reference_coefficients", C.POINTER(C.c_float)), ("delta_to", C.POINTER(C.c_double)), ("delta_from", C.POINTER(C.c_double))]


class _RoosterMotionReport(C.Structure):
    _fields_ = _RoosterReport._fields_ + [("ms_warp", C.c_double), ("ms_upload_model", C.c_double)]


ROOSTER4D_MOTION_STAGES = {"warp": 0, "unwarp": 1, "tv_time_motion": 2}


def frame_signals(phase, signals, frames: int) -> np.ndarray:
    """The breathing state of every frame of a 4-D reconstruction: phase [n] in [0, 1], signals [n, K] (or [n]) -> float64 [frames, K].

    Projection k lies between frames l = floor(phase N) mod N and h = (l + 1) mod N with the weights w_h = phase N - floor(phase N),
    w_l = 1 - w_h (the S rule of rooster4d, csrc/rooster4d.hip: interpolation_weights).  The state of frame f is the mean of the
    signals of the projections that touch it, weighted by those weights.  A frame that no projection touches has no state:
    ValueError."""
    N = int(frames)
    ph = np.asarray(phase, dtype=np.float64).ravel()
    s = np.asarray(signals, dtype=np.float64)
    if s.ndim == 1:
        s = s[:, None]
    if s.ndim != 2 or s.shape[0] != ph.size:
        raise ValueError(f"{ph.size} phase values but signals of shape {np.shape(signals)}")
    t = ph * N
    ft = np.floor(t)
    l = np.mod(ft.astype(np.int64), N)
    h = (l + 1) % N
    wh = t - ft
    wl = 1.0 - wh
    total = np.zeros(N)
    acc = np.zeros((N, s.shape[1]))
    np.add.at(total, l, wl)
    np.add.at(total, h, wh)
    np.add.at(acc, l, wl[:, None] * s)
    np.add.at(acc, h, wh[:, None] * s)
    if not (total > 0).all():
        raise ValueError(f"no projection touches frame(s) {np.flatnonzero(~(total > 0)).tolist()} of {N}: they have no breathing state")
    return acc / total[:, None]


def _rooster_motion(lib, frames, dimension, spacing, motion_to_reference: MotionModel, motion_from_reference: MotionModel, states):
    """(mcgpu_rooster4d_motion, the arrays it points into) for the frame states [frames, K].  lib: what _rooster_call returned (callers
    pass it since this function declared the motion prototypes; _library() does now)."""
    motion_to_reference.check_grid(dimension, spacing)
    motion_from_reference.check_grid(dimension, spacing)
    if motion_to_reference.n_signal_dims != motion_from_reference.n_signal_dims:
        raise ValueError(f"the model to the reference has {motion_to_reference.n_signal_dims} signal dimensions, the model from it "
                         f"{motion_from_reference.n_signal_dims}")
    delta_to, delta_from = motion_to_reference.delta(states), motion_from_reference.delta(states)
    if delta_to.shape[0] != int(frames):
        raise ValueError(f"{int(frames)} frames but {delta_to.shape[0]} frame states")
    if not (np.isfinite(delta_to).all() and np.isfinite(delta_from).all()):
        raise ValueError("the signals are not finite")
    m = _RoosterMotion(C.sizeof(_RoosterMotion), motion_to_reference.n_signal_dims, *motion_to_reference.pointers(), *motion_from_reference.pointers(),
                       delta_to.ctypes.data_as(_DP), delta_from.ctypes.data_as(_DP))
    return m, (delta_to, delta_from)


def rooster4d_motion(projections: np.ndarray, geometry: CircularGeometry, pixel_spacing: Tuple[float, float], pixel_origin: Optional[Tuple[float, float]],
                     phase: Sequence[float], motion_to_reference: MotionModel, motion_from_reference: MotionModel, signals,
                     dimension: Tuple[int, int, int] = (464, 250, 464), spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0),
                     origin: Optional[Tuple[float, float, float]] = None, frames: int = 10, niter: int = 10, cgiter: int = 4, tviter: int = 10,
                     gamma_time: float = 0.0002, gamma_space: float = 0.00007, water_pre_correction: Optional[Sequence[float]] = None,
                     positivity: bool = True, gpu_id: int = 0):
    """Motion-aware 4-D ROOSTER (Mory, Janssens, Rit, PMB 2016; csrc/rooster4d.hip states the rule): rooster4d()
    with the temporal TV run along the trajectories of two motion models instead of along the time axis of every voxel, so that a
    strong `gamma_time` averages the same tissue over the frames and does not smear what moves.

    DIRECTION of the two models, both `MotionModel`s on the reconstruction grid with the same K (ValueError otherwise):
      motion_to_reference    the FORWARD model: the material of reference-phase voxel P is at P + F(P; s) at state s.
                             `MotionModel.from_correspondence_model(CorrespondenceModel.build_default(..., inverse=True), ...)`.
      motion_from_reference  the PULL-BACK model: frame_s(Q) = ref(Q + G(Q; s)).  The default `build_default(...)`, converted the
                             same way.
    Neither is derived from the other, and a swapped pair is NOT detected: it moves every frame twice the wrong way.
    signals [n, K]: the breathing signal of every projection in the models' units; frame f is given the state
    `frame_signals(phase, signals, frames)[f]`.

    Step 4 of a main iteration becomes  y = W x;  c = TVtime(y) - y;  x = x + U c  (W warps every frame to the reference phase, U
    back): the increment form, which resamples only the regulariser's correction.  RTK replaces x by U TVtime(W x), which blurs x
    whenever a displacement is no whole number of voxels -- a deliberate departure (profiles/rooster4d_motion.md has the figures).
    Everything else, the remaining arguments and the defaults are those of rooster4d().  Parity against RTK is unpinned (RTK is
    absent here); tests/rooster_motion_ref.py restates the rule in float64.

    -> (volume [frames, nz, ny, nx] float32, report dict: that of rooster4d plus ms_warp, ms_upload_model and frame_signals)."""
    from . import engine
    p = np.ascontiguousarray(projections, dtype=np.float32)
    n, nv, nu = p.shape
    lib, o, keep = _rooster_call(n, nu, nv, geometry, pixel_spacing, pixel_origin, phase, dimension, spacing, origin, frames, niter, cgiter, tviter,
                                 gamma_time, gamma_space, water_pre_correction, positivity, gpu_id)
    s = np.asarray(signals, dtype=np.float64)
    if s.shape[0] != n:
        raise ValueError(f"{n} projections but {s.shape[0]} signals")
    states = frame_signals(keep["phase"], s, frames)
    m, keep_m = _rooster_motion(lib, frames, dimension, spacing, motion_to_reference, motion_from_reference, states)
    vol, rep = _volume(dimension, frames), _RoosterMotionReport()
    engine._check(lib.mcgpu_rooster4d_reconstruct_motion(C.byref(o), C.byref(m), p.ctypes.data, vol.ctypes.data, C.byref(rep)))
    return vol, _rooster_result(rep, keep, niter, cgiter, frame_signals=states)


def rooster4d_motion_stage(stage: str, data: np.ndarray, motion_to_reference: MotionModel, motion_from_reference: MotionModel, frame_states,
                           dimension, spacing, tviter: int = 10, gamma_time: float = 0.0002, gpu_id: int = 0):
    """One operator of rooster4d_motion alone (mcgpu_rooster4d_motion_stage), [frames, nz, ny, nx] -> the same shape: 'warp' (W, every
    frame to the reference phase with motion_to_reference), 'unwarp' (U, back with motion_from_reference), 'tv_time_motion'
    (x + U (TVtime(W x) - W x) with `tviter` iterations and `gamma_time`).  frame_states [frames, K]: the state of every frame (what
    frame_signals gives).  -> (result float32, report dict)."""
    from . import engine
    src = np.ascontiguousarray(data, dtype=np.float32)
    shape4 = (src.shape[0] if src.ndim == 4 else -1, int(dimension[2]), int(dimension[1]), int(dimension[0]))
    if src.shape != shape4:
        raise ValueError(f"rooster4d_motion_stage {stage}: input shape {src.shape}")
    frames = src.shape[0]
    placeholder = CircularGeometry(1000.0, 1500.0, [0.0], [0.0], [0.0])  # the stages use no projection geometry; the options need a valid one
    lib, o, keep = _rooster_call(1, 2, 2, placeholder, (1.0, 1.0), None, [0.0], dimension, spacing, None, frames, 0, 0, tviter, gamma_time, 0.0,
                                 None, True, gpu_id)
    m, keep_m = _rooster_motion(lib, frames, dimension, spacing, motion_to_reference, motion_from_reference, frame_states)
    out, rep = np.zeros(shape4, dtype=np.float32), _RoosterMotionReport()
    engine._check(lib.mcgpu_rooster4d_motion_stage(C.byref(o), C.byref(m), ROOSTER4D_MOTION_STAGES[stage], src.ctypes.data, out.ctypes.data, C.byref(rep)))
    return out, _report_dict(rep)


def reconstruct_4d_mc(projections_filepath, geometry_filepath, model_to_reference, model_from_reference, signals, voxel_spacing_mm,
                      amplitude_signal: Optional[np.ndarray] = None, phase_signal: Optional[np.ndarray] = None, output_folder=None,
                      output_filename: Optional[str] = None, dimension: Tuple[int, int, int] = (464, 250, 464),
                      spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0), water_pre_correction: Optional[Sequence[float]] = None, gpu_id: int = 0,
                      **kwargs):
    """reconstruct_4d with the motion of two fitted `CorrespondenceModel`s followed by the temporal regulariser (rooster4d_motion):
    the signal handling and the parameters of reconstruct_4d, the file flow of reconstruct_3d_mc.
    model_to_reference: built with `build_default(..., inverse=True)` (reference-phase voxels forward to a state);
    model_from_reference: the default `build_default(...)` (pull-back fields); both on the reconstruction grid (see
    MotionModel.from_correspondence_model for the frame).  A swapped pair is not detected.  voxel_spacing_mm: the spacing of the
    MCGeometry the fields live on; signals [n, K]: the breathing signal of every projection, in the models' units.  Writes
    `recon_rooster4d_mc.mha` (4-D, as reconstruct_4d) and a .yaml that also records `motion_to_reference` / `motion_from_reference`
    (the first 7 hex digits of each model's hash), `signal_n_dims` (K) and `temporal_update: increment`."""
    ph = _unit_phase(amplitude_signal, phase_signal)
    to_reference = MotionModel.from_correspondence_model(model_to_reference, voxel_spacing_mm, dimension=dimension, spacing=spacing)
    from_reference = MotionModel.from_correspondence_model(model_from_reference, voxel_spacing_mm, dimension=dimension, spacing=spacing)
    params = _rooster_parameters(kwargs)
    return _reconstruct_to_file(
        projections_filepath, geometry_filepath, output_folder, output_filename or "recon_rooster4d_mc.mha", dimension, spacing, water_pre_correction,
        lambda proj, geometry, ds, org: rooster4d_motion(proj, geometry, ds, org, ph, to_reference, from_reference, signals, dimension, spacing, None,
                                                         water_pre_correction=water_pre_correction, gpu_id=gpu_id, **params),
        dict(fp="Joseph", bp="VoxelBased", motion_to_reference=model_to_reference.model_hash[:7], motion_from_reference=model_from_reference.model_hash[:7],
             signal_n_dims=to_reference.n_signal_dims, temporal_update="increment", **params, **kwargs))
