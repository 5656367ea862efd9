"""The speed-up network on the MI355X -- the in-process stand-in for the reference's `MCSpeedup`
(cbctmc/speedup/inference.py; the network is cbctmc/speedup/models.py: MCSpeedUpUNet).

A low-photon projection stack and the forward projection of the density volume go in; the network's mean, its variance and one
normal sample `mean + sqrt(variance) z` come out.  The arithmetic is `csrc/speedup_net.hip` through `mcgpu_speedup_run`
(float32, as the reference runs it with autocast off); there is no CPU fallback.  The reference ships no trained weights: users
bring the `.pth` its trainer wrote.  What is pinned: the arithmetic, against the reference class with seeded weights
(tests/test_speedup.py, tests/test_speedup_gpu.py); no trained weights have ever been run here.

Deviations from the reference, both stated in INTEGRATION.md 5e: a forward-projection slice of zero variance is refused (the
reference divides by zero and returns NaN), and z comes from a counter-based generator (Philox4x32-10 keyed by `seed`), so that a
seed reproduces a sample and a stack split into several calls equals one call."""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _unet


class _SpeedupOptions(C.Structure):
    """mcgpu_speedup_options (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("device", C.c_int), ("n", C.c_int), ("nu", C.c_int), ("nv", C.c_int), ("mean_in_channels", C.c_int),
                ("mean_levels", C.c_int), ("mean_filter_base", C.c_int), ("var_in_channels", C.c_int), ("var_levels", C.c_int),
                ("var_filter_base", C.c_int), ("weights", C.c_void_p), ("n_weights", C.c_ulonglong), ("seed", C.c_ulonglong),
                ("first_projection", C.c_int)]


class _SpeedupReport(C.Structure):
    """mcgpu_speedup_report (include/mcgpu_amd.h)."""
    _fields_ = [("ms_upload", C.c_double), ("ms_preprocess", C.c_double), ("ms_conv", C.c_double), ("ms_norm", C.c_double), ("ms_other", C.c_double),
                ("ms_total", C.c_double), ("peak_device_bytes", C.c_ulonglong)]


class _SpeedupStageArgs(C.Structure):
    """mcgpu_speedup_stage_args (include/mcgpu_amd.h)."""
    _fields_ = [("struct_size", C.c_uint), ("upsample", C.c_int), ("c1", C.c_int), ("c2", C.c_int), ("c_out", C.c_int), ("in_", C.c_void_p),
                ("in2", C.c_void_p), ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p)]


SPEEDUP_STAGES = {"conv": 0, "norm_lrelu": 1, "maxpool": 2, "preprocess": 3, "normals": 4}


def _library():
    from . import engine
    lib = engine.load_library()
    lib.mcgpu_speedup_run.argtypes = [C.POINTER(_SpeedupOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_SpeedupReport)]
    lib.mcgpu_speedup_stage.argtypes = [C.POINTER(_SpeedupOptions), C.c_int, C.POINTER(_SpeedupStageArgs), C.POINTER(_SpeedupReport)]
    return lib


def unet_tensors(prefix: str, in_channels: int, levels: int, base: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of one FlexUNet's tensors in the state dict's order: init_conv, final_conv, enc_0 .. enc_{L-1},
    dec_{L-1} .. dec_0; each block holds its two convolutions as convs.0 and convs.3."""
    by_level = [base << i for i in range(levels)]
    return _unet.unet_tensors([base] + by_level + by_level[::-1] + [base], levels, 1, in_channels, 2, prefix + ".")


def state_dict_tensors(mean_net=(2, 4, 64), var_net=(1, 2, 16)) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of MCSpeedUpUNet's state dict without `var_scale`: the order of the flat weights of mcgpu_speedup_options."""
    return unet_tensors("mean_net", *mean_net) + unet_tensors("var_net", *var_net)


def _architecture(weights: Dict[str, np.ndarray], prefix: str) -> Tuple[int, int, int]:
    """(in_channels, levels, filter_base) of a FlexUNet, from the tensor shapes."""
    key = f"{prefix}.init_conv.weight"
    if key not in weights:
        raise ValueError(f"missing key {key}")
    shape = tuple(np.shape(weights[key]))
    if len(shape) != 4 or shape[2:] != (3, 3):
        raise ValueError(f"{key} has shape {shape}, expected (filter_base, in_channels, 3, 3)")
    levels = 1 + max([int(m.group(1)) for m in (re.match(rf"{prefix}\.enc_(\d+)\.", k) for k in weights) if m], default=0)
    return int(shape[1]), levels, int(shape[0])


class MCSpeedup:
    """Mirror of cbctmc/speedup/inference.py: MCSpeedup.  `weights` maps the reference's state-dict names to arrays; the
    architecture (input channels, levels, filter base of the two nets) is read from the shapes.  `var_scale` may be present: the
    forward pass never reads it."""

    def __init__(self, weights: Dict[str, np.ndarray], device: int = 0):
        weights = dict(weights)
        weights.pop("var_scale", None)
        self.mean_net = _architecture(weights, "mean_net")
        self.var_net = _architecture(weights, "var_net")
        if self.mean_net[0] not in (1, 2) or self.var_net[0] != 1:
            raise ValueError(f"mean_net.init_conv.weight / var_net.init_conv.weight: {self.mean_net[0]} / {self.var_net[0]} input channels, "
                             "expected 1 or 2 / 1")
        self.device = int(device)
        self.flat = _unet.flatten(weights, state_dict_tensors(self.mean_net, self.var_net))

    @property
    def in_channels(self) -> int:
        return self.mean_net[0]

    @classmethod
    def from_filepath(cls, model_filepath, device: int = 0) -> "MCSpeedup":
        """A `.pth` as the reference's trainer writes it or a `.npz` with the same names (_unet.read_weights)."""
        return cls(_unet.read_weights(model_filepath), device)

    # ------------------------------------------------------------------------------------------------------------------
    def _options(self, n, nv, nu, seed=0, first_projection=0) -> _SpeedupOptions:
        return _SpeedupOptions(C.sizeof(_SpeedupOptions), self.device, int(n), int(nu), int(nv), *self.mean_net, *self.var_net,
                               self.flat.ctypes.data, self.flat.size, int(seed) & (2 ** 64 - 1), int(first_projection))

    def _stack(self, a, name) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 3:
            raise ValueError(f"{name} has shape {a.shape}, expected [n, nv, nu]")
        return a

    def _inputs(self, low_photon, forward_projection):
        lp = self._stack(low_photon, "low_photon")
        if self.in_channels == 1:
            if forward_projection is not None:
                raise ValueError("these weights were trained without the forward projection (in_channels = 1): pass forward_projection=None")
            return lp, None
        if forward_projection is None:
            raise ValueError("these weights take the forward projection (in_channels = 2)")
        fp = self._stack(forward_projection, "forward_projection")
        if fp.shape != lp.shape:
            raise ValueError(f"forward_projection has shape {fp.shape}, low_photon {lp.shape}")
        return lp, fp

    def _run(self, low_photon, forward_projection, seed, first_projection, want_sample):
        from . import engine
        lp, fp = self._inputs(low_photon, forward_projection)
        mean, variance = np.zeros_like(lp), np.zeros_like(lp)
        sample = np.zeros_like(lp) if want_sample else None
        o = self._options(*lp.shape, seed=seed, first_projection=first_projection)
        rep = _SpeedupReport()
        engine._check(_library().mcgpu_speedup_run(C.byref(o), lp.ctypes.data, fp.ctypes.data if fp is not None else None, mean.ctypes.data,
                                                   variance.ctypes.data, sample.ctypes.data if want_sample else None, C.byref(rep)))
        return mean, variance, sample, _unet.report_dict(rep)

    @staticmethod
    def preprocess_inputs(low_photon, forward_projection=None):
        """(low_photon, forward_projection matched to it in mean and unbiased std per projection): the statement in numpy of what
        the device does before the network (statistics in float64, applied in float32); stacks [n, nv, nu]."""
        lp = np.asarray(low_photon, dtype=np.float32)
        if forward_projection is None:
            return lp, None
        fp = np.asarray(forward_projection, dtype=np.float32)
        if fp.shape != lp.shape or lp.ndim != 3:
            raise ValueError(f"forward_projection has shape {fp.shape}, low_photon {lp.shape}; expected two stacks [n, nv, nu]")
        stat = lambda a, f: f(a.astype(np.float64), axis=(1, 2), keepdims=True).astype(np.float32)  # noqa: E731
        std = lambda a, **kw: np.std(a, ddof=1, **kw)  # noqa: E731
        if np.any(stat(fp, std) == 0):
            raise ValueError("a forward-projection slice has zero variance: it cannot be matched to the low-photon projection")
        return lp, (fp - stat(fp, np.mean)) / stat(fp, std) * stat(lp, std) + stat(lp, np.mean)

    def predict(self, low_photon, forward_projection=None):
        """(mean, variance) of stacks [n, nv, nu]."""
        mean, variance, _, self.last_report = self._run(low_photon, forward_projection, 0, 0, False)
        return mean, variance

    def sample(self, mean, variance, seed: int, first_projection: int = 0):
        """mean + sqrt(variance) z in float32, z from the generator of the kernels (speedup_stage 'normals')."""
        mean, variance = self._stack(mean, "mean"), self._stack(variance, "variance")
        z = speedup_stage("normals", shape=mean.shape, seed=seed, first_projection=first_projection, device=self.device)[0]
        return mean + np.sqrt(variance) * z

    def execute(self, low_photon, forward_projection=None, batch_size: int = 16, seed: Optional[int] = None, output_filepath=None,
                first_projection: int = 0):
        """Arrays [n, nv, nu] -> (mean, variance, sample); paths of .mha stacks -> the sample (and, with `output_filepath`, that
        sample written with the low-photon stack's spacing and origin).  `batch_size` is accepted for the reference's signature
        and changes nothing: projections are independent.  seed=None draws one from os.urandom; the seed used is in
        `self.last_report["seed"]`."""
        from . import reconstruction
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        from_files = not isinstance(low_photon, np.ndarray)
        spacing = origin = None
        if from_files:
            low_photon, spacing, origin = reconstruction.read_mha(low_photon)
            if forward_projection is not None:
                forward_projection = reconstruction.read_mha(forward_projection)[0]
        elif output_filepath is not None:
            raise ValueError("output_filepath needs the low-photon stack as a file (its spacing and origin are written)")
        mean, variance, sample, report = self._run(low_photon, forward_projection, seed, first_projection, True)
        report["seed"] = int(seed)
        self.last_report = report
        if not from_files:
            return mean, variance, sample
        if output_filepath is not None:
            reconstruction.write_mha(output_filepath, sample, spacing, origin)
        return sample


def speedup_stage(stage: str, data=None, in2=None, weight=None, bias=None, upsample: bool = False, shape=None, seed: int = 0,
                  first_projection: int = 0, device: int = 0):
    """One operator of the network alone (mcgpu_speedup_stage) -> (array, report).  'conv': data [c1, H, W], optional in2
    [c2, H2, W2] (read through the x 2 nearest upsample when `upsample`), weight [c_out, c1 + c2, 3, 3], bias [c_out];
    'norm_lrelu' and 'maxpool': data [c, H, W]; 'preprocess': data = low photon [n, H, W], in2 = forward projection; 'normals':
    shape = (n, H, W), seed, first_projection."""
    from . import engine
    code = SPEEDUP_STAGES[stage]
    data, in2, weight, bias = map(_unet.f32, (data, in2, weight, bias))
    lead, H, W = (tuple(shape) if stage == "normals" else data.shape)
    n, c1, c2, c_out = 1, 0, 0, 0
    if stage in ("preprocess", "normals"):
        n, out_shape = lead, (lead, H, W)
        if stage == "preprocess" and in2.shape != data.shape:
            raise ValueError(f"speedup_stage preprocess: shapes {data.shape} and {in2.shape}")
    elif stage == "conv":
        c1, c2, c_out = lead, (in2.shape[0] if in2 is not None else 0), weight.shape[0]
        want2 = ((H + 1) // 2, (W + 1) // 2) if upsample else (H, W)
        if weight.shape != (c_out, c1 + c2, 3, 3) or bias.shape != (c_out,) or (in2 is not None and in2.shape[1:] != want2):
            raise ValueError(f"speedup_stage conv: shapes {data.shape}, {None if in2 is None else in2.shape}, {weight.shape}, {bias.shape}")
        out_shape = (c_out, H, W)
    else:
        c1, out_shape = lead, ((lead, H, W) if stage == "norm_lrelu" else (lead, H // 2, W // 2))
    out = np.zeros(out_shape, dtype=np.float32)
    o = _SpeedupOptions(struct_size=C.sizeof(_SpeedupOptions), device=int(device), n=int(n), nu=int(W), nv=int(H), seed=int(seed) & (2 ** 64 - 1),
                        first_projection=int(first_projection))
    a = _SpeedupStageArgs(C.sizeof(_SpeedupStageArgs), int(bool(upsample)), int(c1), int(c2), int(c_out), *map(_unet.ptr, (data, in2, weight, bias)),
                          out.ctypes.data)
    rep = _SpeedupReport()
    engine._check(_library().mcgpu_speedup_stage(C.byref(o), code, C.byref(a), C.byref(rep)))
    return out, _unet.report_dict(rep)


def speedup_simulation(simulation_folder, config_name: str, weights_filepath, gpu_id: int = 0, is_4d: bool = False, seed: Optional[int] = None):
    """The speed-up step of the reference's scan driver (scripts/run_mc_simulations.py:558-587): reads
    <folder>/<config>/projections_total_normalized.mha and <folder>/density_fp.mha (4-D: <folder>/<config>/density_fp_4d.mha),
    writes <folder>/<config>/projections_total_normalized_speedup.mha -> (its path, report dict with the seed used)."""
    folder = Path(simulation_folder)
    model = MCSpeedup.from_filepath(weights_filepath, device=gpu_id)
    forward_projection = folder / config_name / "density_fp_4d.mha" if is_4d else folder / "density_fp.mha"
    out = folder / config_name / "projections_total_normalized_speedup.mha"
    model.execute(folder / config_name / "projections_total_normalized.mha", forward_projection if model.in_channels == 2 else None, seed=seed,
                  output_filepath=out)
    return out, model.last_report
