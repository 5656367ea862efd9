"""Training of the speed-up network on the MI355X -- the in-process stand-in for the reference's `MCSpeedUpTrainer`
(cbctmc/speedup/trainer.py), its `MCSpeedUpDataset` (cbctmc/speedup/dataset.py) and its driver (scripts/train_speedup.py).

The arithmetic is `csrc/speedup_train.hip` behind a device-resident handle (`mcgpu_speedup_train_*`): the forward pass of
`MCSpeedup`, the L1 loss of the mean (phase "mean", the first `n_pretrain_steps` updates), then the Gaussian negative
log-likelihood of the variance with the mean net frozen (phase "variance"), their gradients and Adam with an exponentially
decaying learning rate.  There is no CPU fallback.  What the trainer saves, `MCSpeedup.from_filepath` loads.

Deviations from the reference, stated in INTEGRATION.md 5l: the bias of a convolution that feeds an instance norm has gradient
exactly zero and never moves (mathematically it is zero; autograd moves it by rounding noise, and the norm removes the effect);
everything is float32 with no gradient scaler (the reference trains under float16 autocast); the joint stage
(`n_pretrain_steps=None`) is not built."""
from __future__ import annotations

import ctypes as C
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _unet
from ._unet_training import DeviceTrainer
from .speedup import state_dict_tensors

logger = logging.getLogger(__name__)

PHASES = {"mean": 0, "variance": 1}
TRAIN_STAGES = {"conv_wgrad": 0, "conv_dgrad": 1, "norm_lrelu_backward": 2, "maxpool_backward": 3, "loss_l1": 4, "loss_nll": 5, "adam": 6}
METRICS = ("loss", "l1_loss", "gaussian_nll_loss", "psnr_before", "psnr_after")
VAR_SCALE = 0.001  # MCSpeedUpUNet.var_scale: a parameter of the reference class that its forward pass never reads


class _TrainOptions(C.Structure):
    """mcgpu_speedup_train_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("max_batch", C.c_int),
                ("mean_in_channels", C.c_int), ("mean_levels", C.c_int), ("mean_filter_base", C.c_int), ("var_in_channels", C.c_int),
                ("var_levels", C.c_int), ("var_filter_base", C.c_int), ("dry", C.c_int), ("weights", C.c_void_p), ("n_weights", C.c_ulonglong),
                ("lr", C.c_double), ("gamma", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double)]


class _TrainReport(C.Structure):
    """mcgpu_speedup_train_report (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("phase", C.c_int), ("loss", C.c_double), ("l1_loss", C.c_double), ("gaussian_nll_loss", C.c_double),
                ("psnr_before", C.c_double), ("psnr_after", C.c_double), ("step", C.c_ulonglong), ("lr", C.c_double), ("ms_forward", C.c_double),
                ("ms_wgrad", C.c_double), ("ms_dgrad", C.c_double), ("ms_norm", C.c_double), ("ms_optimizer", C.c_double), ("ms_total", C.c_double),
                ("peak_device_bytes", C.c_ulonglong)]


class _TrainState(C.Structure):
    """mcgpu_speedup_train_state (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("reserved", C.c_int), ("weights", C.c_void_p), ("moment1", C.c_void_p), ("moment2", C.c_void_p),
                ("n_weights", C.c_ulonglong), ("step_mean", C.c_ulonglong), ("step_variance", C.c_ulonglong), ("lr", C.c_double),
                ("planned_device_bytes", C.c_ulonglong)]


class _TrainStageArgs(C.Structure):
    """mcgpu_speedup_train_stage_args (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("upsample", C.c_int), ("c1", C.c_int),
                ("c2", C.c_int), ("c_out", C.c_int), ("in_", C.c_void_p), ("in2", C.c_void_p), ("in3", C.c_void_p), ("out", C.c_void_p),
                ("out2", C.c_void_p), ("out3", C.c_void_p), ("values", C.c_void_p), ("n", C.c_ulonglong), ("step", C.c_ulonglong),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double)]


def _library():
    from . import engine
    lib = engine.load_library()
    batch = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mcgpu_speedup_train_create.argtypes = [C.POINTER(_TrainOptions), C.POINTER(C.c_void_p)]
    lib.mcgpu_speedup_train_step.argtypes = batch + [C.c_int, C.POINTER(_TrainReport)]
    lib.mcgpu_speedup_train_gradients.argtypes = batch + [C.c_void_p, C.POINTER(_TrainReport)]
    lib.mcgpu_speedup_train_predict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mcgpu_speedup_train_get_state.argtypes = [C.c_void_p, C.POINTER(_TrainState)]
    lib.mcgpu_speedup_train_set_state.argtypes = [C.c_void_p, C.POINTER(_TrainState)]
    lib.mcgpu_speedup_train_destroy.argtypes = [C.c_void_p]
    lib.mcgpu_speedup_train_stage.argtypes = [C.c_int, C.POINTER(_TrainStageArgs), C.POINTER(_TrainReport)]
    return lib


def initial_weights(seed: int = 0, mean_net=(2, 4, 64), var_net=(1, 2, 16)) -> Dict[str, np.ndarray]:
    """A fresh state dict by the rule of a default `Conv2d`: weight and bias uniform on +-1 / sqrt(9 C_in), drawn with numpy from
    `seed` in the state dict's order (the rule, not the reference framework's random stream)."""
    rng = np.random.default_rng(seed)
    out, bound = {}, 0.0
    for name, shape in state_dict_tensors(mean_net, var_net):
        if name.endswith(".weight"):
            bound = 1.0 / np.sqrt(9.0 * shape[1])
        out[name] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


def adam_step(w, g, m, v, t: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """One Adam update in float64, as the device applies it per element -> (w, m, v)."""
    w, g, m, v = (np.asarray(a, dtype=np.float64) for a in (w, g, m, v))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    w = w - lr / (1.0 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return w, m, v


def _batch(a, name: str) -> Optional[np.ndarray]:
    """[n, 1, nv, nu] or [n, nv, nu] (or one [nv, nu]) -> float32 [n, nv, nu]."""
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 4 and a.shape[1] == 1:
        a = a[:, 0]
    elif a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"{name} has shape {a.shape}, expected [n, 1, nv, nu] or [n, nv, nu]")
    return np.ascontiguousarray(a)


class MCSpeedupTrainer(DeviceTrainer):
    """Mirror of cbctmc/speedup/trainer.py: MCSpeedUpTrainer on a device-resident trainer.  `weights`: a state dict by the
    reference's names (None: `initial_weights(seed, ...)`); the architecture is `mean_net` / `var_net` = (input channels, levels,
    filter base).  The phase is "mean" while `i_step < n_pretrain_steps` and "variance" afterwards; at the switch the learning
    rate goes back to `lr`, as the reference resets it."""

    ABI = "mcgpu_speedup_train_"
    _library = staticmethod(_library)

    def __init__(self, weights: Optional[Dict[str, np.ndarray]] = None, mean_net=(2, 4, 64), var_net=(1, 2, 16), device: int = 0, seed: int = 0,
                 lr: float = 1e-3, gamma: float = 0.99999, n_pretrain_steps: Optional[int] = 5000, betas=(0.9, 0.999)):
        if n_pretrain_steps is None:
            raise ValueError("n_pretrain_steps=None (the reference's joint stage of both nets) is not built: pass a step count (0: variance only)")
        self.mean_net, self.var_net = tuple(int(v) for v in mean_net), tuple(int(v) for v in var_net)
        self.tensors = state_dict_tensors(self.mean_net, self.var_net)
        if weights is None:
            weights = initial_weights(seed, self.mean_net, self.var_net)
        weights = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in weights.items() if k != "var_scale"}
        self._init_state(_unet.flatten(weights, self.tensors))
        self._steps = [0, 0]
        self.device, self.lr0, self.gamma, self.betas = int(device), float(lr), float(gamma), (float(betas[0]), float(betas[1]))
        self._lr = self.lr0
        self.n_pretrain_steps = int(n_pretrain_steps)
        self.i_step = 0

    # ------------------------------------------------------------------------------------------------------------ the handle
    @property
    def in_channels(self) -> int:
        return self.mean_net[0]

    @property
    def phase(self) -> str:
        return "mean" if self.i_step < self.n_pretrain_steps else "variance"

    def _options(self, max_batch: int, extent, dry: bool = False) -> _TrainOptions:
        nv, nu = extent
        return _TrainOptions(C.sizeof(_TrainOptions), self.device, int(nu), int(nv), int(max_batch), *self.mean_net, *self.var_net, int(dry),
                             self._flat.ctypes.data, self._flat.size, self._lr, self.gamma, *self.betas)

    def _state(self, arrays: bool) -> _TrainState:
        s = _TrainState(struct_size=C.sizeof(_TrainState), n_weights=self._flat.size, step_mean=self._steps[0], step_variance=self._steps[1], lr=self._lr)
        if arrays:
            s.weights, s.moment1, s.moment2 = self._flat.ctypes.data, self._moment1.ctypes.data, self._moment2.ctypes.data
        return s

    def _read_state(self, s: _TrainState):
        self._steps, self._lr = [int(s.step_mean), int(s.step_variance)], float(s.lr)

    def planned_device_bytes(self, n: int, nv: int, nu: int) -> int:
        """What a trainer for batches [n][nv][nu] holds on the device, planned without touching it."""
        return self._planned(n, (nv, nu))

    # ----------------------------------------------------------------------------------------------------------- the batches
    def _inputs(self, data: dict, need_target: bool = True):
        lp = _batch(data["low_photon"], "low_photon")
        fp = _batch(data.get("forward_projection"), "forward_projection") if self.in_channels == 2 else None
        if self.in_channels == 2 and fp is None:
            raise ValueError("these weights take the forward projection (in_channels = 2): data['forward_projection'] is missing")
        t = _batch(data.get("high_photon"), "high_photon") if need_target else None
        for name, a in (("forward_projection", fp), ("high_photon", t)):
            if a is not None and a.shape != lp.shape:
                raise ValueError(f"{name} has shape {a.shape}, low_photon {lp.shape}")
        if need_target and t is None:
            raise ValueError("data['high_photon'] is missing")
        self._ensure(lp.shape[0], lp.shape[1:])
        return lp, fp, t

    def _step(self, data: dict, update: bool) -> dict:
        from . import engine
        lp, fp, t = self._inputs(data)
        if update and self.i_step == self.n_pretrain_steps and self.i_step > 0:
            self._pull(arrays=False)
            self._lr = self.lr0  # the reference sets the learning rate back at the switch to the variance stage
            self._push(arrays=False)
        rep = _TrainReport(struct_size=C.sizeof(_TrainReport))
        engine._check(_library().mcgpu_speedup_train_step(self._handle, PHASES[self.phase], lp.shape[0], lp.ctypes.data, _unet.ptr(fp), t.ctypes.data,
                                                          int(update), C.byref(rep)))
        if update:
            self.i_step += 1
        self.last_report = _unet.report_dict(rep)
        return {k: float(getattr(rep, k)) for k in METRICS}

    def train_on_batch(self, data: dict) -> dict:
        """One update on a batch {"low_photon", "forward_projection", "high_photon"} -> the reference's five metrics."""
        return self._step(data, True)

    def validate_on_batch(self, data: dict) -> dict:
        """The five metrics of a batch; nothing changes."""
        return self._step(data, False)

    def gradients(self, data: dict, phase: Optional[str] = None) -> Dict[str, np.ndarray]:
        """The batch gradient of the phase's loss by the state dict's names (zero outside the phase's net); nothing changes."""
        from . import engine
        lp, fp, t = self._inputs(data)
        flat = np.zeros_like(self._flat)
        rep = _TrainReport(struct_size=C.sizeof(_TrainReport))
        engine._check(_library().mcgpu_speedup_train_gradients(self._handle, PHASES[phase or self.phase], lp.shape[0], lp.ctypes.data, _unet.ptr(fp),
                                                               t.ctypes.data, flat.ctypes.data, C.byref(rep)))
        self.last_report = _unet.report_dict(rep)
        return self._named(flat)

    def predict(self, low_photon, forward_projection=None):
        """(mean, variance) [n, nv, nu] of the trainer's forward pass with its present weights."""
        from . import engine
        lp, fp, _ = self._inputs({"low_photon": low_photon, "forward_projection": forward_projection}, need_target=False)
        mean, variance = np.zeros_like(lp), np.zeros_like(lp)
        engine._check(_library().mcgpu_speedup_train_predict(self._handle, lp.shape[0], lp.ctypes.data, _unet.ptr(fp), mean.ctypes.data,
                                                             variance.ctypes.data))
        return mean, variance

    # ------------------------------------------------------------------------------------------------------------- the files
    def state_dict(self) -> Dict[str, np.ndarray]:
        """The weights by the reference's names, `var_scale` included: what the reference's `load_state_dict` accepts."""
        self._pull()
        out = self._named(self._flat)
        out["var_scale"] = np.full((1,), VAR_SCALE, dtype=np.float32)
        return out

    def save(self, path) -> Path:
        """`.npz` by the state dict's names, or `.pth` as {"model": state dict} (needs torch): both load with
        `MCSpeedup.from_filepath`."""
        return super().save(path)

    def _checkpoint_extra(self) -> dict:
        """Beside weights and moments: the step counts, the learning rate and the architecture."""
        return dict(steps=np.asarray(self._steps, dtype=np.int64), i_step=np.int64(self.i_step), lr=np.float64(self._lr), mean_net=np.asarray(self.mean_net),
                    var_net=np.asarray(self.var_net))

    def _load_checkpoint_extra(self, path, f):
        if tuple(f["mean_net"]) != self.mean_net or tuple(f["var_net"]) != self.var_net:
            raise ValueError(f"{path}: architecture {tuple(f['mean_net'])} / {tuple(f['var_net'])}, this trainer has {self.mean_net} / {self.var_net}")
        self._steps, self.i_step, self._lr = [int(v) for v in f["steps"]], int(f["i_step"]), float(f["lr"])


# ------------------------------------------------------------------------------------------------------------------ the data
class MCSpeedUpDataset:
    """Mirror of cbctmc/speedup/dataset.py: MCSpeedUpDataset.  One folder of `.npy` projections [nv, nu] named
    `pat_%03d__phase_%02d__{mode}__proj_%03d.npy` (the low-photon scan of speed-up mode `mode`), `...__fp__...` (the forward
    projection) and `...__reference__...` (the high-photon scan).  An item is a dict with `low_photon`, `forward_projection`,
    `high_photon` as float32 [1, nv, nu] and `patient_id`, `mode`, `phase`, `projection`; a slice or index array gives a list."""

    def __init__(self, filepaths: Sequence[dict]):
        self.filepaths = list(filepaths)

    def __len__(self):
        return len(self.filepaths)

    @staticmethod
    def _load(entry: dict) -> dict:
        out = {k: entry[k] for k in ("patient_id", "mode", "phase", "projection")}
        for key in ("low_photon", "forward_projection", "high_photon"):
            out[key] = np.asarray(np.load(entry[key + "_filepath"]), dtype=np.float32)[np.newaxis]
        return out

    def __getitem__(self, item):
        if isinstance(item, np.ndarray):
            chosen = [self.filepaths[int(i)] for i in item]
        elif isinstance(item, slice):
            chosen = self.filepaths[item]
        else:
            chosen = [self.filepaths[int(item)]]
        data = [self._load(e) for e in chosen]
        return data[0] if len(data) == 1 else data

    def batch(self, indices) -> dict:
        """The items `indices` stacked: arrays [n, 1, nv, nu], the rest as lists."""
        items = [self._load(self.filepaths[int(i)]) for i in indices]
        out = {k: [it[k] for it in items] for k in ("patient_id", "mode", "phase", "projection")}
        for key in ("low_photon", "forward_projection", "high_photon"):
            out[key] = np.stack([it[key] for it in items])
        return out

    @classmethod
    def from_folder(cls, folder, modes: Sequence[str], patient_ids: Sequence[int], phases: Sequence[int] = (0,),
                    projections: Sequence[int] = range(894)) -> "MCSpeedUpDataset":
        return cls(cls.fetch_filepaths(folder, modes, patient_ids, phases, projections))

    @staticmethod
    def get_patient_ids_from_folder(folder) -> List[int]:
        return sorted({int(p.name[4:7]) for p in Path(folder).iterdir() if p.name.startswith("pat_")})

    @staticmethod
    def fetch_filepaths(root_folder, modes: Sequence[str], patient_ids: Sequence[int], phases: Sequence[int] = (0,),
                        projections: Sequence[int] = range(895)) -> List[dict]:
        """Every (patient, mode, phase, projection) whose three files exist; an incomplete triple is skipped with a warning."""
        root = Path(root_folder)
        found = []
        for patient_id in patient_ids:
            for mode in modes:
                for phase in phases:
                    for projection in projections:
                        name = lambda kind: root / f"pat_{patient_id:03d}__phase_{phase:02d}__{kind}__proj_{projection:03d}.npy"  # noqa: E731
                        entry = {"patient_id": patient_id, "phase": phase, "mode": mode, "projection": projection, "low_photon_filepath": name(mode),
                                 "forward_projection_filepath": name("fp"), "high_photon_filepath": name("reference")}
                        present = [entry[k].exists() for k in ("low_photon_filepath", "forward_projection_filepath", "high_photon_filepath")]
                        if all(present):
                            found.append(entry)
                        elif any(present):
                            logger.warning("Skipping incomplete %s", entry["low_photon_filepath"].name)
        return found


def write_speedup_dataset(simulation_folder, low_config: str, high_config: str, output_folder, patient_id: int, phase: int = 0) -> int:
    """Cuts this package's scan outputs into the dataset's layout: `<folder>/<low_config>/projections_total_normalized.mha` as
    mode `low_config`, `<folder>/<high_config>/projections_total_normalized.mha` as `reference` and `<folder>/density_fp.mha` as
    `fp`, one `.npy` [nv, nu] per projection -> the number of projections written."""
    from . import reconstruction
    folder, out = Path(simulation_folder), Path(output_folder)
    low = reconstruction.read_mha(folder / low_config / "projections_total_normalized.mha")[0]
    high = reconstruction.read_mha(folder / high_config / "projections_total_normalized.mha")[0]
    fp = reconstruction.read_mha(folder / "density_fp.mha")[0]
    if not (low.shape == high.shape == fp.shape) or low.ndim != 3:
        raise ValueError(f"stacks of shapes {low.shape}, {high.shape}, {fp.shape}: expected three equal [n, nv, nu]")
    out.mkdir(parents=True, exist_ok=True)
    for p in range(low.shape[0]):
        for kind, stack in ((low_config, low), ("reference", high), ("fp", fp)):
            np.save(out / f"pat_{patient_id:03d}__phase_{phase:02d}__{kind}__proj_{p:03d}.npy", np.asarray(stack[p], dtype=np.float32))
    return int(low.shape[0])


def train_speedup(dataset_folder, modes: Sequence[str], train_patient_ids: Sequence[int], test_patient_ids: Sequence[int], steps: int,
                  batch_size: int = 10, save_interval: int = 1000, run_folder="speedup_run", seed: int = 0, trainer: Optional[MCSpeedupTrainer] = None,
                  phases: Sequence[int] = (0,), projections: Sequence[int] = range(895), **trainer_options):
    """The reference's driver loop (scripts/train_speedup.py): batches of `batch_size` in an order shuffled from `seed`, epoch after
    epoch, for `steps` updates; every `save_interval` updates (and at the end) the test set is validated in order and the weights
    are written to `<run_folder>/models/training/step_%d.npz` (and `.pth` where torch is importable) beside a checkpoint.
    -> (trainer, history: a list of {"step", "train": metrics, "validation": mean metrics or None})."""
    train = MCSpeedUpDataset.from_folder(dataset_folder, modes, train_patient_ids, phases, projections)
    test = MCSpeedUpDataset.from_folder(dataset_folder, modes, test_patient_ids, phases, projections)
    if len(train) == 0:
        raise ValueError(f"no complete training triple in {dataset_folder} for modes {list(modes)} and patients {list(train_patient_ids)}")
    if trainer is None:
        trainer = MCSpeedupTrainer(seed=seed, **trainer_options)
    rng = np.random.default_rng(seed)
    models = Path(run_folder) / "models" / "training"
    history, order, at = [], rng.permutation(len(train)), 0

    def validate():
        if len(test) == 0:
            return None
        rows, weights = [], []
        for lo in range(0, len(test), batch_size):
            idx = range(lo, min(lo + batch_size, len(test)))
            rows.append(trainer.validate_on_batch(test.batch(idx)))
            weights.append(len(idx))
        return {k: float(np.average([r[k] for r in rows], weights=weights)) for k in METRICS}

    for _ in range(int(steps)):
        if at + batch_size > len(order) and at > 0:
            order, at = rng.permutation(len(train)), 0
        metrics = trainer.train_on_batch(train.batch(order[at:at + batch_size]))
        at += batch_size
        entry = {"step": trainer.i_step, "train": metrics, "validation": None}
        if trainer.i_step % int(save_interval) == 0 or len(history) + 1 == int(steps):
            entry["validation"] = validate()
            trainer.save(models / f"step_{trainer.i_step}.npz")
            try:
                trainer.save(models / f"step_{trainer.i_step}.pth")
            except ImportError:
                pass
            trainer.save_checkpoint(models / f"checkpoint_{trainer.i_step}.npz")
        history.append(entry)
    return trainer, history


def speedup_train_stage(stage: str, data, in2=None, in3=None, upsample: bool = False, c_out: int = 0, state=None, step: int = 1, lr: float = 1e-3,
                        betas=(0.9, 0.999), device: int = 0):
    """One backward operator alone (mcgpu_speedup_train_stage) -> (outputs, report dict).
    'conv_wgrad': data [c1, H, W], in2 [c2, H2, W2] or None, in3 = dY [c_out, H, W] -> (dW, db, partials);
    'conv_dgrad': data = dY [c_out, H, W], in2 = weight [c_out, c1 + c2, 3, 3], c_out = c1 here (the channels of the first source)
    -> (d in, d in2 or None); 'norm_lrelu_backward': data = x [c, H, W], in2 = dy -> dx; 'maxpool_backward': data = x, in2 = dy -> dx;
    'loss_l1': data = low photon [n, H, W], in2 = net output, in3 = high photon -> (loss, d net, mean); 'loss_nll': data = mean, in2 =
    net output, in3 = high photon -> (loss, d net, variance); 'adam': data = gradient [n], state = (w, m, v) -> (w, m, v)."""
    from . import engine
    code = TRAIN_STAGES[stage]
    data, in2, in3 = map(_unet.f32, (data, in2, in3))
    a = _TrainStageArgs(struct_size=C.sizeof(_TrainStageArgs), device=int(device), upsample=int(bool(upsample)), step=int(step), lr=float(lr),
                        beta1=float(betas[0]), beta2=float(betas[1]))
    values = np.zeros(4, dtype=np.float64)
    a.values = values.ctypes.data
    if stage == "adam":
        w, m, v = (np.array(s, dtype=np.float32).ravel() for s in state)
        a.n = data.size
        a.out, a.out2, a.out3 = w.ctypes.data, m.ctypes.data, v.ctypes.data
        result = lambda: (w, m, v)  # noqa: E731
    elif stage == "conv_wgrad":
        c1, H, W = data.shape
        c2 = in2.shape[0] if in2 is not None else 0
        co = in3.shape[0]
        dw, db = np.zeros((co, c1 + c2, 3, 3), np.float32), np.zeros(co, np.float32)
        a.nu, a.nv, a.c1, a.c2, a.c_out = W, H, c1, c2, co
        a.out, a.out2 = dw.ctypes.data, db.ctypes.data
        result = lambda: (dw, db, int(values[0]))  # noqa: E731
    elif stage == "conv_dgrad":
        co, H, W = data.shape
        c1 = int(c_out)
        c2 = in2.shape[1] - c1
        d1 = np.zeros((c1, H, W), np.float32)
        d2 = np.zeros((c2, (H + 1) // 2, (W + 1) // 2) if upsample else (c2, H, W), np.float32) if c2 else None
        a.nu, a.nv, a.c1, a.c2, a.c_out = W, H, c1, c2, co
        a.out, a.out2 = d1.ctypes.data, _unet.ptr(d2)
        result = lambda: (d1, d2)  # noqa: E731
    elif stage in ("norm_lrelu_backward", "maxpool_backward"):
        c, H, W = data.shape
        dx = np.zeros_like(data)
        a.nu, a.nv, a.c1 = W, H, c
        a.out = dx.ctypes.data
        result = lambda: dx  # noqa: E731
    else:
        n, H, W = data.shape
        g, head = np.zeros_like(data), np.zeros_like(data)
        a.nu, a.nv, a.n = W, H, n
        a.out, a.out2 = g.ctypes.data, head.ctypes.data
        result = lambda: (float(values[0]), g, head)  # noqa: E731
    a.in_, a.in2, a.in3 = _unet.ptr(data), _unet.ptr(in2), _unet.ptr(in3)
    rep = _TrainReport(struct_size=C.sizeof(_TrainReport))
    engine._check(_library().mcgpu_speedup_train_stage(code, C.byref(a), C.byref(rep)))
    return result(), _unet.report_dict(rep)
