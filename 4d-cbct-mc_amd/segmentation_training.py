"""Training of the CT segmentation network on the MI355X -- the in-process stand-in for the reference's `CTSegmentationTrainer`
(cbctmc/segmentation/trainer.py), its `SegmentationDataset` (cbctmc/segmentation/dataset.py), its `DiceLoss`
(cbctmc/segmentation/losses.py) as the driver's `SegmentationLoss(use_dice=True)` applies it, the `ReduceLROnPlateau` the driver
hands the trainer, and the driver's loop (scripts/train_segmentation.py).

The arithmetic is `csrc/segment_train.hip` behind a device-resident handle (`mcgpu_segment_train_*`): the forward pass of
`MCSegmenter` on one patch, the Dice loss per sample and label (softmax over labels 0 .. 7, sigmoid on the lung vessels), its
gradient and Adam; the learning rate is the host's (`ReduceLROnPlateau`, torch's rule).  There is no CPU fallback.  What the
trainer saves, `MCSegmenter.from_filepath` loads.  No weights trained on real CTs exist yet: what is pinned is the arithmetic.

Deviations from the reference, stated in INTEGRATION.md 5m: the bias of a convolution that feeds an instance norm has gradient
exactly zero and never moves; no gradient scaler (the reference's forward pass runs with autocast disabled, so both compute in
float32); `single_segmentation` and `use_dice=False` are refused; the dataset draws from a seeded `numpy.random.Generator`
instead of the global `random`, and resamples to no spacing but the file's own."""
from __future__ import annotations

import ctypes as C
import logging
from itertools import combinations
from pathlib import Path
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _unet
from ._unet_training import DeviceTrainer
from .segmentation import LABELS, N_LABELS, unet_tensors

logger = logging.getLogger(__name__)

TRAIN_STAGES = {"conv_wgrad": 0, "conv_dgrad": 1, "maxpool_backward": 2, "loss": 3}
TARGET_UINT8, TARGET_FLOAT32 = 0, 1
METRICS = ("loss",) + tuple(f"loss_label_{name}" for name in LABELS.values())
# the tissue segmentations the reference loads from files; background and other are derived, lung_vessels is an overlay
LABELS_TO_LOAD = ("body", "upper_body_bones", "upper_body_muscles", "upper_body_fat", "liver", "stomach", "lung", "lung_vessels")


class _TrainOptions(C.Structure):
    """mcgpu_segment_train_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("patch_shape", C.c_int * 3), ("max_batch", C.c_int), ("levels", C.c_int),
                ("n_filters", C.c_int * 18), ("n_classes", C.c_int), ("dry", C.c_int), ("weights", C.c_void_p), ("n_weights", C.c_ulonglong),
                ("beta1", C.c_double), ("beta2", C.c_double)]


class _TrainReport(C.Structure):
    """mcgpu_segment_train_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("n", C.c_int), ("loss", C.c_double), ("loss_label", C.c_double * 9), ("step", C.c_ulonglong),
                ("ms_forward", C.c_double), ("ms_wgrad", C.c_double), ("ms_dgrad", C.c_double), ("ms_norm", C.c_double), ("ms_optimizer", C.c_double),
                ("ms_total", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


class _TrainState(C.Structure):
    """mcgpu_segment_train_state (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("weights", C.c_void_p), ("moment1", C.c_void_p), ("moment2", C.c_void_p),
                ("n_weights", C.c_ulonglong), ("step", C.c_ulonglong), ("planned_device_bytes", C.c_ulonglong)]


class _TrainStageArgs(C.Structure):
    """mcgpu_segment_train_stage_args (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("shape", C.c_int * 3), ("upsample", C.c_int), ("c1", C.c_int), ("c2", C.c_int),
                ("c_out", C.c_int), ("in_", C.c_void_p), ("in2", C.c_void_p), ("in3", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p),
                ("values", C.c_void_p), ("n", C.c_ulonglong)]


def _library():
    from . import engine
    lib = engine.load_library()
    batch = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.mcgpu_segment_train_create.argtypes = [C.POINTER(_TrainOptions), C.POINTER(C.c_void_p)]
    lib.mcgpu_segment_train_step.argtypes = batch + [C.c_double, C.c_int, C.POINTER(_TrainReport)]
    lib.mcgpu_segment_train_gradients.argtypes = batch + [C.c_void_p, C.POINTER(_TrainReport)]
    lib.mcgpu_segment_train_predict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mcgpu_segment_train_get_state.argtypes = [C.c_void_p, C.POINTER(_TrainState)]
    lib.mcgpu_segment_train_set_state.argtypes = [C.c_void_p, C.POINTER(_TrainState)]
    lib.mcgpu_segment_train_destroy.argtypes = [C.c_void_p]
    lib.mcgpu_segment_train_stage.argtypes = [C.c_int, C.POINTER(_TrainStageArgs), C.POINTER(_TrainReport)]
    return lib


def initial_weights(seed: int = 0, n_filters: Sequence[int] = (32,) * 10, levels: int = 4) -> Dict[str, np.ndarray]:
    """A fresh state dict by the rule of a default `Conv3d`: weight and bias uniform on +-1 / sqrt(27 C_in), drawn with numpy from
    `seed` in the state dict's order (the rule, not the reference framework's random stream)."""
    rng = np.random.default_rng(seed)
    out, bound = {}, 0.0
    for name, shape in unet_tensors(n_filters, levels):
        if name.endswith(".weight"):
            bound = 1.0 / np.sqrt(27.0 * shape[1])
        out[name] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------- the scheduler
class ReduceLROnPlateau:
    """`torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min", threshold_mode="rel")` on one learning rate, in host Python; the
    defaults are the reference driver's.  `step(metric)` after every update: a metric below best x (1 - threshold) is an
    improvement; after more than `patience` steps without one the rate becomes max(lr x factor, min_lr) (where that lowers it by
    more than `eps`) and `cooldown` steps pass before bad steps count again."""

    def __init__(self, factor: float = 0.9, patience: int = 1000, threshold: float = 1e-2, cooldown: int = 1000, min_lr: float = 1e-6,
                 eps: float = 1e-8):
        if not factor < 1.0:
            raise ValueError(f"factor is {factor}: it must be < 1.0")
        self.factor, self.patience, self.threshold = float(factor), int(patience), float(threshold)
        self.cooldown, self.min_lr, self.eps = int(cooldown), float(min_lr), float(eps)
        self.best, self.num_bad_epochs, self.cooldown_counter, self.last_epoch = float("inf"), 0, 0, 0

    def step(self, metric: float, lr: float) -> float:
        """The learning rate after seeing `metric` with the rate `lr`."""
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            new_lr = max(lr * self.factor, self.min_lr)
            if lr - new_lr > self.eps:
                lr = new_lr
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        return lr

    def state_dict(self) -> dict:
        return {k: getattr(self, k) for k in ("factor", "patience", "threshold", "cooldown", "min_lr", "eps", "best", "num_bad_epochs", "cooldown_counter",
                                              "last_epoch")}

    def load_state_dict(self, state: dict):
        for k, v in state.items():
            setattr(self, k, type(getattr(self, k))(v))


# --------------------------------------------------------------------------------------------------------------- the trainer
def _images(a) -> np.ndarray:
    """[n, 1, P0, P1, P2], [n, P0, P1, P2] or one [P0, P1, P2] -> float32 [n, P0, P1, P2]."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 5 and a.shape[1] == 1:
        a = a[:, 0]
    elif a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f"image has shape {a.shape}, expected [n, 1, P0, P1, P2], [n, P0, P1, P2] or [P0, P1, P2]")
    return np.ascontiguousarray(a)


def _targets(a, images: np.ndarray) -> np.ndarray:
    """[n, 9, P0, P1, P2] or one [9, P0, P1, P2] -> uint8 as it is, anything else as float32."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim == 4:
        a = a[None]
    want = (images.shape[0], N_LABELS) + images.shape[1:]
    if a.shape != want:
        raise ValueError(f"segmentation has shape {a.shape}, expected {want} for images {images.shape}")
    return np.ascontiguousarray(a if a.dtype == np.uint8 else a.astype(np.float32, copy=False))


class CTSegmentationTrainer(DeviceTrainer):
    """Mirror of cbctmc/segmentation/trainer.py: CTSegmentationTrainer on a device-resident trainer, with the driver's loss
    (Dice, `use_dice=True`) and optimizer (Adam, lr 1e-4).  `weights`: a state dict by the reference's names, a path to one
    (`.pth` / `.npz`) or None for `initial_weights(seed, n_filters, levels)`.  `lr_scheduler`: a `ReduceLROnPlateau` of this
    module or None; it is stepped on `loss` after every update, as the reference's post-hook does."""

    ABI = "mcgpu_segment_train_"
    _library = staticmethod(_library)

    def __init__(self, weights=None, seed: int = 0, lr: float = 1e-4, lr_scheduler: Optional[ReduceLROnPlateau] = None,
                 n_filters: Sequence[int] = (32,) * 10, levels: int = 4, device: int = 0, betas=(0.9, 0.999),
                 single_segmentation: Optional[str] = None, use_dice: bool = True):
        if single_segmentation is not None:
            raise ValueError(f"single_segmentation={single_segmentation!r} is not built: MCSegmenter needs all {N_LABELS} outputs")
        if not use_dice:
            raise ValueError(f"use_dice={use_dice!r} (the cross-entropy + BCE variant of the driver's loss) is not built: only the Dice loss is")
        if not lr > 0.0:
            raise ValueError(f"lr is {lr}: it must be > 0")
        self.levels, self.n_filters = int(levels), tuple(int(v) for v in n_filters)
        self.tensors = unet_tensors(self.n_filters, self.levels)
        if weights is None:
            weights = initial_weights(seed, self.n_filters, self.levels)
        elif not isinstance(weights, dict):
            weights = _unet.read_weights(weights)
        weights = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in weights.items()}
        self._init_state(_unet.flatten(weights, self.tensors, "inconsistent weight shapes: "))
        self.device, self.betas = int(device), (float(betas[0]), float(betas[1]))
        self.lr, self.lr_scheduler = float(lr), lr_scheduler
        self.i_step = 0

    # ------------------------------------------------------------------------------------------------------------ the handle
    def _options(self, n: int, patch_shape, dry: bool = False) -> _TrainOptions:
        if len(patch_shape) != 3:
            raise ValueError(f"patch_shape {tuple(patch_shape)}: three axes are needed")
        o = _TrainOptions(struct_size=C.sizeof(_TrainOptions), device=self.device, max_batch=int(n), levels=self.levels, n_classes=N_LABELS, dry=int(dry),
                          weights=self._flat.ctypes.data, n_weights=self._flat.size, beta1=self.betas[0], beta2=self.betas[1])
        o.patch_shape[:] = [int(v) for v in patch_shape]
        o.n_filters[:len(self.n_filters)] = self.n_filters
        return o

    def _state(self, arrays: bool) -> _TrainState:
        s = _TrainState(struct_size=C.sizeof(_TrainState), n_weights=self._flat.size, step=self.i_step)
        if arrays:
            s.weights, s.moment1, s.moment2 = self._flat.ctypes.data, self._moment1.ctypes.data, self._moment2.ctypes.data
        return s

    def _read_state(self, s: _TrainState):
        self.i_step = int(s.step)

    def planned_device_bytes(self, n: int, patch_shape) -> int:
        """What a trainer for batches [n][patch] holds on the device, planned without touching it."""
        return self._planned(n, patch_shape)

    # ----------------------------------------------------------------------------------------------------------- the batches
    def _inputs(self, data: dict, need_target: bool = True):
        x = _images(data["image"])
        t = None
        if need_target:
            if data.get("segmentation") is None:
                raise ValueError("data['segmentation'] is missing")
            t = _targets(data["segmentation"], x)
        self._ensure(x.shape[0], x.shape[1:])
        return x, t

    def _metrics(self, rep: _TrainReport) -> dict:
        out = {"loss": float(rep.loss)}
        for index, name in LABELS.items():
            out[f"loss_label_{name}"] = float(rep.loss_label[index])
        return out

    def _step(self, data: dict, update: bool) -> dict:
        from . import engine
        x, t = self._inputs(data)
        rep = _TrainReport(struct_size=C.sizeof(_TrainReport))
        engine._check(_library().mcgpu_segment_train_step(self._handle, x.shape[0], x.ctypes.data, t.ctypes.data,
                                                          TARGET_UINT8 if t.dtype == np.uint8 else TARGET_FLOAT32, self.lr, int(update), C.byref(rep)))
        self.last_report = _unet.report_dict(rep)
        self.last_report["loss_label"] = list(rep.loss_label)
        return self._metrics(rep)

    def train_on_batch(self, data: dict) -> dict:
        """One update on a batch {"image", "segmentation"} -> the ten metrics and `learning_rate` (the rate the update used); then
        the scheduler sees `loss`."""
        metrics = self._step(data, True)
        self.i_step += 1
        metrics["learning_rate"] = self.lr
        if self.lr_scheduler is not None:
            self.lr = self.lr_scheduler.step(metrics["loss"], self.lr)
        return metrics

    def validate_on_batch(self, data: dict) -> dict:
        """The ten metrics of a batch; nothing changes."""
        return self._step(data, False)

    def gradients(self, data: dict) -> Dict[str, np.ndarray]:
        """The batch gradient of the loss by the state dict's names; nothing changes."""
        from . import engine
        x, t = self._inputs(data)
        flat = np.zeros_like(self._flat)
        rep = _TrainReport(struct_size=C.sizeof(_TrainReport))
        engine._check(_library().mcgpu_segment_train_gradients(self._handle, x.shape[0], x.ctypes.data, t.ctypes.data,
                                                               TARGET_UINT8 if t.dtype == np.uint8 else TARGET_FLOAT32, flat.ctypes.data, C.byref(rep)))
        self.last_report = _unet.report_dict(rep)
        return self._named(flat)

    def predict(self, data) -> np.ndarray:
        """Logits [n, 9, P0, P1, P2] of the trainer's forward pass with its present weights (a batch dict or the images)."""
        from . import engine
        x, _ = self._inputs(data if isinstance(data, dict) else {"image": data}, need_target=False)
        logits = np.zeros((x.shape[0], N_LABELS) + x.shape[1:], dtype=np.float32)
        engine._check(_library().mcgpu_segment_train_predict(self._handle, x.shape[0], x.ctypes.data, logits.ctypes.data))
        return logits

    # ------------------------------------------------------------------------------------------------------------- the files
    def state_dict(self) -> Dict[str, np.ndarray]:
        """The weights by the reference's names: what the reference's `load_state_dict` accepts."""
        self._pull()
        return self._named(self._flat)

    def save(self, path) -> Path:
        """`.npz` by the state dict's names, or `.pth` as {"model": state dict} (needs torch): both load with
        `MCSegmenter.from_filepath`."""
        return super().save(path)

    def _checkpoint_extra(self) -> dict:
        """Beside weights and moments: the step count, the learning rate, the architecture and the scheduler's state."""
        sched = self.lr_scheduler.state_dict() if self.lr_scheduler is not None else {}
        return dict(i_step=np.int64(self.i_step), lr=np.float64(self.lr), n_filters=np.asarray(self.n_filters), levels=np.int64(self.levels),
                    scheduler_keys=np.asarray(list(sched.keys()), dtype=str), scheduler_values=np.asarray(list(sched.values()), dtype=np.float64))

    def _load_checkpoint_extra(self, path, f):
        if tuple(int(v) for v in f["n_filters"]) != self.n_filters or int(f["levels"]) != self.levels:
            raise ValueError(f"{path}: architecture {tuple(f['n_filters'])} / {int(f['levels'])} levels, this trainer has {self.n_filters} / {self.levels}")
        self.i_step, self.lr = int(f["i_step"]), float(f["lr"])
        sched = dict(zip([str(k) for k in f["scheduler_keys"]], [float(v) for v in f["scheduler_values"]]))
        if sched:
            if self.lr_scheduler is None:
                self.lr_scheduler = ReduceLROnPlateau()
            self.lr_scheduler.load_state_dict(sched)


# ------------------------------------------------------------------------------------------------------------------ the data
def merge_mc_segmentations(segmentations: Dict[str, np.ndarray]) -> np.ndarray:
    """The reference's `SegmentationDataset.merge_mc_segmentations` on arrays: `segmentations` maps the names of LABELS_TO_LOAD to
    arrays of one shape -> uint8 [9, ...] in the order of LABELS.  background = body == 0; other = none of the six tissues nor
    background; lung_vessels is not in that union and stays an independent overlay."""
    missing = [k for k in LABELS_TO_LOAD if k not in segmentations]
    if missing:
        raise ValueError(f"missing segmentation {missing[0]!r}: {list(LABELS_TO_LOAD)} are needed")
    s = {k: np.asarray(v) for k, v in segmentations.items()}
    s["background"] = s["body"] == 0
    tissues = ("upper_body_bones", "upper_body_muscles", "upper_body_fat", "liver", "stomach", "lung", "background")
    s["other"] = np.logical_not(np.stack([s[k] for k in tissues]).astype(bool).any(axis=0))
    return np.stack([s[name] for name in LABELS.values()]).astype(np.uint8)


def pad_to_patch(image: Optional[np.ndarray], mask: Optional[np.ndarray], patch_shape, image_pad_value=-1000, mask_pad_value=0):
    """The reference's `crop_or_pad(no_crop=True)`: every spatial axis shorter than the patch is padded (left = pad // 2)."""
    shape = image.shape if image is not None else mask.shape[-3:]
    pad = [((p - n) // 2, (p - n) - (p - n) // 2) if n < p else (0, 0) for n, p in zip(shape, patch_shape)]
    if image is not None:
        image = np.pad(image, pad, mode="constant", constant_values=image_pad_value)
    if mask is not None:
        mask = np.pad(mask, [(0, 0)] * (mask.ndim - 3) + pad, mode="constant", constant_values=mask_pad_value)
    return image, mask


def rescale_range(values: np.ndarray, input_range=(-1024, 3071), output_range=(0, 1)) -> np.ndarray:
    """float32, operation by operation: ((v - in_min) (out_max - out_min)) / (in_max - in_min) + out_min, clipped (what
    `MCSegmenter` applies to an image); nothing when the ranges are equal or one is None."""
    v = np.asarray(values, dtype=np.float32)
    if not input_range or not output_range or tuple(input_range) == tuple(output_range):
        return v
    f = np.float32
    v = ((v - f(input_range[0])) * f(output_range[1] - output_range[0])) / f(input_range[1] - input_range[0]) + f(output_range[0])
    return np.clip(v, f(output_range[0]), f(output_range[1]))


class SegmentationDataset:
    """Mirror of cbctmc/segmentation/dataset.py: SegmentationDataset on numpy arrays or `.mha` paths.  `images[i]`: an array
    [x, y, z] in HU or a path; `segmentations[i]`: a merged array [9, x, y, z], or a dict of the names of LABELS_TO_LOAD to arrays
    or paths (merged by `merge_mc_segmentations`).  Iterating yields, per image, up to `patches_per_image` dicts with `image`
    float32 [1, P0, P1, P2] (rescaled), `segmentation` float32 [9, P0, P1, P2], `patch_slicing`, `i_patch`, `n_patches`, `image_id`,
    `labels`.  Every random draw comes from one `numpy.random.Generator` seeded with `seed` (the reference uses the global
    `random` and `numpy.random`): the same seed gives the same patches."""

    def __init__(self, images: Sequence, segmentations: Sequence, patch_shape: Sequence[int], image_spacing_range=None, random_rotation: bool = True,
                 add_noise: float = 100.0, shift_image_values: Optional[Tuple[float, float]] = (0.9, 1.1), patches_per_image=1,
                 force_balanced_sampling: bool = False, input_value_range=(-1024, 3071), output_value_range=(0, 1), seed: int = 0,
                 image_spacings: Optional[Sequence] = None):
        if len(images) != len(segmentations):
            raise ValueError(f"{len(images)} images but {len(segmentations)} segmentations")
        if len(patch_shape) != 3:
            raise ValueError(f"patch_shape {tuple(patch_shape)}: three axes are needed")
        self.images, self.segmentations = list(images), list(segmentations)
        self.patch_shape = tuple(int(p) for p in patch_shape)
        self.image_spacing_range = image_spacing_range
        self.image_spacings = list(image_spacings) if image_spacings is not None else None
        self.random_rotation, self.add_noise, self.shift_image_values = bool(random_rotation), float(add_noise or 0.0), shift_image_values
        self.patches_per_image, self.force_balanced_sampling = patches_per_image, bool(force_balanced_sampling)
        self.input_value_range, self.output_value_range = input_value_range, output_value_range
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return len(self.images)

    @staticmethod
    def _read(item):
        """(array [x, y, z], spacing or None) of an array or an `.mha` path (the file holds [z, y, x])."""
        if isinstance(item, (str, Path)):
            from . import reconstruction
            array, spacing, _ = reconstruction.read_mha(item)
            return np.transpose(array, (2, 1, 0)), tuple(float(s) for s in spacing[:3])
        return np.asarray(item), None

    def _load(self, index: int):
        image, spacing = self._read(self.images[index])
        seg = self.segmentations[index]
        if isinstance(seg, dict):
            seg = merge_mc_segmentations({k: self._read(v)[0] for k, v in seg.items()})
        else:
            seg = np.asarray(seg)
        if image.ndim != 3 or seg.shape != (N_LABELS,) + image.shape:
            raise ValueError(f"image {index} has shape {image.shape} and its segmentation {seg.shape}: expected [x, y, z] and [{N_LABELS}, x, y, z]")
        if spacing is None:
            spacing = tuple(float(s) for s in self.image_spacings[index]) if self.image_spacings is not None else (1.0, 1.0, 1.0)
        if self.image_spacing_range is not None:
            for axis, (r, s) in enumerate(zip(self.image_spacing_range, spacing)):
                if tuple(float(v) for v in r) != (s, s):
                    raise ValueError(f"image_spacing_range {tuple(r)} on axis {axis} of image {index} whose spacing is {s}: random spacing resampling is "
                                     "not built (resample with Context.resample_volume first)")
        return image, seg, spacing

    def _rotate(self, image, seg):
        planes = list(combinations(range(-3, 0), 2))
        plane = planes[int(self.rng.integers(len(planes)))]
        k = int(self.rng.integers(0, 4))
        if k:
            image, seg = np.rot90(image, k=k, axes=plane), np.rot90(seg, k=k, axes=plane)
        return image, seg

    def patch_start(self, image_shape) -> Tuple[int, ...]:
        """One random start per axis, uniform on 0 .. N - P inclusive."""
        return tuple(int(self.rng.integers(0, n - p + 1)) for n, p in zip(image_shape, self.patch_shape))

    def __iter__(self) -> Iterable[dict]:
        for index in range(len(self.images)):
            image, seg, spacing = self._load(index)
            if isinstance(self.patches_per_image, float) and 0.0 < self.patches_per_image <= 1.0:
                n_patches = max(round(image.size / int(np.prod(self.patch_shape)) * self.patches_per_image), 1)
            else:
                n_patches = int(self.patches_per_image)
            if self.random_rotation:
                image, seg = self._rotate(image, seg)
            image, rest = pad_to_patch(image, seg[1:], self.patch_shape, mask_pad_value=0)
            _, background = pad_to_patch(None, seg[:1], self.patch_shape, mask_pad_value=1)
            seg = np.concatenate([background, rest], axis=0)
            i_patch, sampled = 0, {i: 0 for i in LABELS}
            for _ in range(n_patches * 10):  # the reference's cap on attempts
                start = self.patch_start(image.shape)
                slicing = tuple(slice(s, s + p) for s, p in zip(start, self.patch_shape))
                x = image[slicing].astype(np.float32, order="C")
                t = seg[(slice(None),) + slicing].astype(np.float32, order="C")
                if self.force_balanced_sampling:
                    least = min(sampled.values())
                    candidates = [i for i, count in sampled.items() if count == least]
                    selected = candidates[int(self.rng.integers(len(candidates)))]
                    present = {i for i in LABELS if t[i].any()}
                    if selected not in present:
                        continue
                    for i in present:
                        sampled[i] += 1
                if self.add_noise:
                    std = self.rng.uniform(1.0, self.add_noise)
                    x = x + self.rng.normal(0.0, std, size=x.shape)
                if self.shift_image_values:
                    x = x * self.rng.uniform(*self.shift_image_values)
                x = rescale_range(x, self.input_value_range, self.output_value_range)
                yield {"image_id": f"{index:07d}", "patch_id": f"{index:07d}__" + "_".join(f"{s.start:03d}:{s.stop:03d}" for s in slicing),
                       "image": x[np.newaxis], "segmentation": t, "image_spacing": spacing, "full_image_shape": image.shape, "i_patch": i_patch,
                       "n_patches": n_patches, "patch_slicing": slicing, "labels": LABELS}
                i_patch += 1
                if i_patch == n_patches:
                    break


def train_segmentation(train_dataset: Iterable[dict], test_dataset: Optional[Iterable[dict]], steps: int, validation_interval: int = 1000,
                       save_interval: int = 1000, run_folder="segmentation_run", trainer: Optional[CTSegmentationTrainer] = None, **trainer_options):
    """The reference driver's loop (scripts/train_segmentation.py: batches of one patch): the training set is iterated again and
    again until `steps` updates are done; every `validation_interval` updates the test set is validated once through, every
    `save_interval` updates (and at the end) the weights are written to `<run_folder>/models/training/step_%d.npz` (and `.pth`
    where torch is importable) beside a checkpoint.  Without `trainer`, one is made with the driver's scheduler.
    -> (trainer, history: a list of {"step", "train": metrics, "validation": mean metrics or None})."""
    if trainer is None:
        trainer_options.setdefault("lr_scheduler", ReduceLROnPlateau())
        trainer = CTSegmentationTrainer(**trainer_options)
    models = Path(run_folder) / "models" / "training"
    history, done, steps = [], 0, int(steps)

    def validate():
        rows = [trainer.validate_on_batch(data) for data in (test_dataset or ())]
        return {k: float(np.mean([r[k] for r in rows])) for k in METRICS} if rows else None

    while done < steps:
        seen = 0
        for data in train_dataset:
            seen += 1
            metrics = trainer.train_on_batch(data)
            done += 1
            entry = {"step": trainer.i_step, "train": metrics, "validation": None}
            if trainer.i_step % int(validation_interval) == 0 or done == steps:
                entry["validation"] = validate()
            if trainer.i_step % int(save_interval) == 0 or done == steps:
                trainer.save(models / f"step_{trainer.i_step}.npz")
                try:
                    trainer.save(models / f"step_{trainer.i_step}.pth")
                except ImportError:
                    pass
                trainer.save_checkpoint(models / f"checkpoint_{trainer.i_step}.npz")
            history.append(entry)
            if done == steps:
                break
        if seen == 0:
            raise ValueError("the training dataset yields no patch")
    return trainer, history


# ---------------------------------------------------------------------------------------------------------------- the stages
def segment_train_stage(stage: str, data, in2=None, in3=None, upsample: bool = False, c1: int = 0, device: int = 0):
    """One backward operator alone (mcgpu_segment_train_stage) -> (outputs, report dict).
    'conv_wgrad': data [c1, d0, d1, d2], in2 [c2, ...] or None, in3 = dY [c_out, d0, d1, d2] -> (dW, db, partials);
    'conv_dgrad': data = dY [c_out, d0, d1, d2], in2 = weight [c_out, c1 + c2, 3, 3, 3], c1 = the channels of the first source
    -> (d in, d in2 or None); 'maxpool_backward': data = x, in2 = dy, in3 = what dx holds before or None -> dx;
    'loss': data = logits [n, 9, d0, d1, d2], in2 = target -> (loss, f [n, 9], d logits)."""
    from . import engine
    code = TRAIN_STAGES[stage]
    data, in2, in3 = map(_unet.f32, (data, in2, in3))
    a = _TrainStageArgs(struct_size=C.sizeof(_TrainStageArgs), device=int(device), upsample=int(bool(upsample)))
    vol = tuple(data.shape[-3:])
    a.shape[:] = vol
    if stage == "conv_wgrad":
        n1 = data.shape[0]
        c2 = in2.shape[0] if in2 is not None else 0
        co = in3.shape[0]
        dw, db = np.zeros((co, n1 + c2, 3, 3, 3), np.float32), np.zeros(co, np.float32)
        values = np.zeros(1, dtype=np.float64)
        a.c1, a.c2, a.c_out = n1, c2, co
        a.out, a.out2 = dw.ctypes.data, db.ctypes.data
        result = lambda: (dw, db, int(values[0]))  # noqa: E731
    elif stage == "conv_dgrad":
        co = data.shape[0]
        c2 = in2.shape[1] - int(c1)
        d1 = np.zeros((int(c1),) + vol, np.float32)
        d2 = np.zeros((c2,) + (tuple((v + 1) // 2 for v in vol) if upsample else vol), np.float32) if c2 else None
        values = np.zeros(1, dtype=np.float64)
        a.c1, a.c2, a.c_out = int(c1), c2, co
        a.out, a.out2 = d1.ctypes.data, _unet.ptr(d2)
        result = lambda: (d1, d2)  # noqa: E731
    elif stage == "maxpool_backward":
        dx = np.zeros_like(data)
        values = np.zeros(1, dtype=np.float64)
        a.c1 = data.shape[0]
        a.out = dx.ctypes.data
        result = lambda: dx  # noqa: E731
    else:
        if data.ndim != 5 or data.shape[1] != N_LABELS or in2 is None or in2.shape != data.shape:
            raise ValueError(f"segment_train_stage loss: shapes {data.shape}, {None if in2 is None else in2.shape}")
        n = data.shape[0]
        g = np.zeros_like(data)
        values = np.zeros(1 + N_LABELS * n, dtype=np.float64)
        a.n = n
        a.out = g.ctypes.data
        result = lambda: (float(values[0]), values[1:].reshape(n, N_LABELS).copy(), g)  # noqa: E731
    a.values = values.ctypes.data
    a.in_, a.in2, a.in3 = _unet.ptr(data), _unet.ptr(in2), _unet.ptr(in3)
    rep = _TrainReport(struct_size=C.sizeof(_TrainReport))
    engine._check(_library().mcgpu_segment_train_stage(code, C.byref(a), C.byref(rep)))
    return result(), _unet.report_dict(rep)
