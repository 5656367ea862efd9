"""The CT segmentation network on the MI355X -- the in-process stand-in for the reference's `MCSegmenter`
(cbctmc/segmentation/segmenter.py; the network is the 3-D `FlexUNet` of cbctmc/speedup/models.py).

A CT image [x, y, z] in HU goes in; nine segmentations come out (eight by softmax and argmax, the lung vessels by sigmoid and 0.5),
as `MCGeometry.from_image(..., segmenter=...)` consumes them.  The arithmetic is `csrc/segment_net.hip` through `mcgpu_segment_run`:
float32 throughout (the reference runs its convolutions in float16 under autocast: this is wider, never narrower); there is no CPU
fallback.  The reference ships no trained weights: users bring the `.pth` its trainer wrote.  What is pinned is the arithmetic,
against the reference class with seeded weights (tests/test_segmentation.py, tests/test_segmentation_gpu.py); no trained weights
have ever been run here.

Departures from the reference, stated in INTEGRATION.md 5f: a `patch_overlap` whose stride is not a whole number is refused (the
reference truncates silently); the patch starts are the rule in plain integers (the reference's uint16 indices wrap under numpy 2
and collapse every patch onto one); a start the rule repeats is inferred once and stitched as often as the rule gives it."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _unet

LABELS = {0: "background", 1: "upper_body_bones", 2: "upper_body_muscles", 3: "upper_body_fat", 4: "liver", 5: "stomach", 6: "lung", 7: "other",
          8: "lung_vessels"}  # 0 .. 7: one softmax group; 8: sigmoid
N_LABELS = len(LABELS)
MAX_LEVELS = 8


def get_label_index(label_name: str) -> int:
    return list(LABELS.values()).index(label_name)


class _SegmentOptions(C.Structure):
    """mcgpu_segment_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("shape", C.c_int * 3), ("image_type", C.c_int), ("patch_shape", C.c_int * 3),
                ("patch_overlap", C.c_double), ("levels", C.c_int), ("n_filters", C.c_int * 18), ("n_classes", C.c_int), ("weights", C.c_void_p),
                ("n_weights", C.c_ulonglong), ("in_min", C.c_double), ("in_max", C.c_double), ("out_min", C.c_double), ("out_max", C.c_double),
                ("memory_limit_bytes", C.c_ulonglong)]


class _SegmentReport(C.Structure):
    """mcgpu_segment_report (include/mcgpu_amd.h)."""
    _fields_ = [("ms_upload", C.c_double), ("ms_conv", C.c_double), ("ms_norm", C.c_double), ("ms_other", C.c_double), ("ms_total", C.c_double),
                ("patches_run", C.c_ulonglong), ("patches_skipped", C.c_ulonglong), ("peak_device_bytes", C.c_ulonglong),
                ("planned_device_bytes", C.c_ulonglong)]


class _SegmentStageArgs(C.Structure):
    """mcgpu_segment_stage_args (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("upsample", C.c_int), ("c1", C.c_int), ("c2", C.c_int), ("c_out", C.c_int), ("shape", C.c_int * 3),
                ("patch_shape", C.c_int * 3), ("n_patches", C.c_int), ("starts", C.c_void_p), ("in_", C.c_void_p), ("in2", C.c_void_p),
                ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p)]


SEGMENT_STAGES = {"conv": 0, "norm_lrelu": 1, "maxpool": 2, "head": 3, "stitch": 4, "finalize": 5}
IMAGE_INT16, IMAGE_FLOAT32 = 0, 1


def _library():
    from . import engine
    lib = engine.load_library()
    lib.mcgpu_segment_run.argtypes = [C.POINTER(_SegmentOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_SegmentReport)]
    lib.mcgpu_segment_stage.argtypes = [C.POINTER(_SegmentOptions), C.c_int, C.POINTER(_SegmentStageArgs), C.POINTER(_SegmentReport)]
    return lib


# ---------------------------------------------------------------------------------------------------------------- patches
def padded_shape(array_shape: Sequence[int], patch_shape: Sequence[int]) -> Tuple[int, ...]:
    """The shape after the reference's `pad_image`: every axis at least as long as the patch."""
    return tuple(max(int(n), int(p)) for n, p in zip(array_shape, patch_shape))


def padding_left(array_shape: Sequence[int], patch_shape: Sequence[int]) -> Tuple[int, ...]:
    """Where the image starts inside the padded shape: left = pad // 2."""
    return tuple((v - int(n)) // 2 for v, n in zip(padded_shape(array_shape, patch_shape), array_shape))


def whole_stride(patch_shape: Sequence[int], patch_overlap: float) -> Tuple[int, ...]:
    """(1 - overlap) x patch axis, which must be a whole number >= 1 (the reference truncates a fraction silently)."""
    out = []
    for axis, p in enumerate(patch_shape):
        s = (1.0 - float(patch_overlap)) * int(p)
        if not s >= 1.0 or s != int(s):
            raise ValueError(f"patch_overlap {patch_overlap} gives a stride of {s} on patch axis {axis} ({p}): a whole number >= 1 is needed")
        out.append(int(s))
    return tuple(out)


def axis_starts(n: int, p: int, s: int) -> List[int]:
    """Patch starts of one axis: min(i s, N - P) for i s in range(0, N - P + s + 1, s)."""
    return [min(v, n - p) for v in range(0, n - p + s + 1, s)]


def patch_starts(array_shape: Sequence[int], patch_shape: Sequence[int], stride: Sequence[int]) -> List[Tuple[int, ...]]:
    """Every patch start of the reference's ordered extraction (`flush=True`), in its order (the last axis runs fastest), repeats
    included; `array_shape` is the padded shape, all values plain integers."""
    axes = [axis_starts(int(n), int(p), int(s)) for n, p, s in zip(array_shape, patch_shape, stride)]
    out = [()]
    for starts in axes:
        out = [t + (v,) for t in out for v in starts]
    return out


# ---------------------------------------------------------------------------------------------------------------- weights
def unet_tensors(n_filters: Sequence[int], levels: int, n_classes: int = N_LABELS, in_channels: int = 1) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the 3-D FlexUNet's state dict in its order; n_filters = [init, enc_0.., dec_{L-1}.., final] (_unet.unet_tensors)."""
    return _unet.unet_tensors(n_filters, levels, n_classes, in_channels, 3)


def _architecture(weights: Dict[str, np.ndarray]) -> Tuple[int, List[int], int]:
    """(levels, n_filters, n_classes) read from the tensor shapes: the first axis of every block's first convolution."""
    def out_channels(key):
        if key not in weights:
            raise ValueError(f"missing key {key}")
        shape = tuple(np.shape(weights[key]))
        if len(shape) != 5 or shape[2:] != (3, 3, 3):
            raise ValueError(f"{key} has shape {shape}, expected (c_out, c_in, 3, 3, 3)")
        return shape
    levels = 1 + max([int(m.group(1)) for m in (re.match(r"enc_(\d+)\.", k) for k in weights) if m], default=-1)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"{levels} encoder levels (enc_0 ..), expected 1..{MAX_LEVELS}")
    init = out_channels("init_conv.weight")
    final = out_channels("final_conv.weight")
    filters = [init[0]] + [out_channels(f"enc_{i}.convs.0.weight")[0] for i in range(levels)]
    filters += [out_channels(f"dec_{i}.convs.0.weight")[0] for i in reversed(range(levels))] + [final[1]]
    return levels, filters, final[0]


class MCSegmenter:
    """Mirror of cbctmc/segmentation/segmenter.py: MCSegmenter.  `weights` maps the names of the reference's state dict to arrays
    (where the reference takes the torch module); the number of levels and every filter count are read from the shapes."""

    def __init__(self, weights: Dict[str, np.ndarray], device: int = 0, patch_shape: Tuple[int, ...] = (128, 128, 128), patch_overlap: float = 0.0,
                 n_labels: int = N_LABELS, input_value_range: Tuple[float, float] = (-1024, 3071), output_value_range: Tuple[float, float] = (0, 1)):
        weights = dict(weights)
        self.levels, self.n_filters, self.n_classes = _architecture(weights)
        init_shape = tuple(np.shape(weights["init_conv.weight"]))
        if init_shape[1] != 1:
            raise ValueError(f"init_conv.weight has shape {init_shape}: the segmenter takes one input channel")
        self.flat = _unet.flatten(weights, unet_tensors(self.n_filters, self.levels, self.n_classes), "inconsistent weight shapes: ")
        if self.n_classes != N_LABELS or int(n_labels) != N_LABELS:
            raise ValueError(f"the final convolution has {self.n_classes} outputs and n_labels is {n_labels}: both must be {N_LABELS} "
                             "(8 softmax labels and the lung vessels)")
        if len(patch_shape) != 3:
            raise ValueError(f"patch_shape {tuple(patch_shape)}: three axes are needed")
        self.device = int(device)
        self.patch_shape = tuple(int(p) for p in patch_shape)
        self.patch_overlap = float(patch_overlap)
        self.n_labels = int(n_labels)
        self.input_value_range = tuple(input_value_range)
        self.output_value_range = tuple(output_value_range)
        self.memory_limit_bytes = 0
        self.last_report: Optional[dict] = None

    @classmethod
    def from_filepath(cls, model_filepath, device: int = 0, **kwargs) -> "MCSegmenter":
        """A `.pth` as the reference's trainer writes it or a `.npz` with the same names (_unet.read_weights)."""
        return cls(_unet.read_weights(model_filepath), device, **kwargs)

    @staticmethod
    def clear_cache():
        """The reference empties torch's CUDA cache here; every call of this class frees what it allocated."""

    def _options(self, shape, image_type) -> _SegmentOptions:
        o = _SegmentOptions(struct_size=C.sizeof(_SegmentOptions), device=self.device, image_type=int(image_type), patch_overlap=self.patch_overlap,
                            levels=self.levels, n_classes=self.n_classes, weights=self.flat.ctypes.data, n_weights=self.flat.size,
                            in_min=float(self.input_value_range[0]), in_max=float(self.input_value_range[1]),
                            out_min=float(self.output_value_range[0]), out_max=float(self.output_value_range[1]),
                            memory_limit_bytes=int(self.memory_limit_bytes))
        o.shape[:] = [int(v) for v in shape]
        o.patch_shape[:] = self.patch_shape
        o.n_filters[:len(self.n_filters)] = self.n_filters
        return o

    def segment(self, image) -> Tuple[np.ndarray, np.ndarray]:
        """(uint8 [9, padded shape], raw float32 [9, padded shape]) of a 3-D image; padded shape = max(image, patch) per axis, as the
        reference returns it.  int16 images are read as they are, anything else as float32."""
        from . import engine
        image = np.asarray(image)
        if image.ndim != 3:
            raise ValueError("Please pass a 3D image")
        image = np.ascontiguousarray(image if image.dtype == np.int16 else image.astype(np.float32, copy=False))
        out_shape = (N_LABELS,) + padded_shape(image.shape, self.patch_shape)
        labels, raw = np.zeros(out_shape, dtype=np.uint8), np.zeros(out_shape, dtype=np.float32)
        o = self._options(image.shape, IMAGE_INT16 if image.dtype == np.int16 else IMAGE_FLOAT32)
        rep = _SegmentReport()
        engine._check(_library().mcgpu_segment_run(C.byref(o), image.ctypes.data, labels.ctypes.data, raw.ctypes.data, C.byref(rep)))
        self.last_report = _unet.report_dict(rep)
        return labels, raw


def segment_stage(stage: str, data, in2=None, weight=None, bias=None, upsample: bool = False, starts=None, shape=None, device: int = 0):
    """One operator alone (mcgpu_segment_stage) -> (array, report).  'conv': data [c1, d0, d1, d2], optional in2 [c2, ...] (read
    through the x 2 nearest upsample when `upsample`), weight [c_out, c1 + c2, 3, 3, 3], bias [c_out]; 'norm_lrelu', 'maxpool': data
    [c, d0, d1, d2]; 'head': logits [9, d0, d1, d2]; 'stitch': data = patches [n, c, p0, p1, p2], starts [n, 3], shape = the volume
    -> mean [c, shape]; 'finalize': mean [9, d0, d1, d2] -> uint8 labels."""
    from . import engine
    code = SEGMENT_STAGES[stage]
    data, in2, weight, bias = map(_unet.f32, (data, in2, weight, bias))
    a = _SegmentStageArgs(struct_size=C.sizeof(_SegmentStageArgs), upsample=int(bool(upsample)))
    out_dtype = np.float32
    if stage == "stitch":
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        n, c = data.shape[:2]
        if data.ndim != 5 or starts.shape != (n, 3) or len(shape) != 3:
            raise ValueError(f"segment_stage stitch: shapes {data.shape}, {starts.shape}, {shape}")
        a.c1, a.n_patches, a.starts = int(c), int(n), starts.ctypes.data
        a.patch_shape[:] = data.shape[2:]
        vol = tuple(int(v) for v in shape)
        out_shape = (c,) + vol
    else:
        if data.ndim != 4:
            raise ValueError(f"segment_stage {stage}: data has shape {data.shape}, expected [c, d0, d1, d2]")
        vol = data.shape[1:]
        a.c1 = int(data.shape[0])
        out_shape = data.shape
        if stage == "conv":
            c2, c_out = (in2.shape[0] if in2 is not None else 0), weight.shape[0]
            want2 = tuple((v + 1) // 2 for v in vol) if upsample else vol
            if weight.shape != (c_out, a.c1 + c2, 3, 3, 3) or bias.shape != (c_out,) or (in2 is not None and in2.shape[1:] != want2):
                raise ValueError(f"segment_stage conv: shapes {data.shape}, {None if in2 is None else in2.shape}, {weight.shape}, {bias.shape}")
            a.c2, a.c_out = int(c2), int(c_out)
            out_shape = (c_out,) + vol
        elif stage == "maxpool":
            out_shape = (data.shape[0],) + tuple(v // 2 for v in vol)
        elif stage in ("head", "finalize"):
            if data.shape[0] != N_LABELS:
                raise ValueError(f"segment_stage {stage}: {data.shape[0]} channels, expected {N_LABELS}")
            out_dtype = np.uint8 if stage == "finalize" else np.float32
    a.shape[:] = vol
    out = np.zeros(out_shape, dtype=out_dtype)
    a.in_, a.in2, a.weight, a.bias, a.out = *map(_unet.ptr, (data, in2, weight, bias)), out.ctypes.data
    o = _SegmentOptions(struct_size=C.sizeof(_SegmentOptions), device=int(device))
    rep = _SegmentReport()
    engine._check(_library().mcgpu_segment_stage(C.byref(o), code, C.byref(a), C.byref(rep)))
    return out, _unet.report_dict(rep)
