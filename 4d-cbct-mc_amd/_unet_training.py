"""What speedup_training.py and segmentation_training.py share of a device-resident trainer (`csrc/unet_train_host.inc` is the same
on the C side): the host copy of the flat weights and both Adam moments, the handle with its hand-over of the state when a batch
needs a larger or another one, the dry plan of the device memory, and the weight and checkpoint files."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict

import numpy as np


class DeviceTrainer:
    """The handle and the files of a trainer behind `<ABI>create / get_state / set_state / destroy`.  A subclass sets `ABI` (the
    prefix of its entry points), `tensors` (the state dict's names and shapes) and gives
      `_library()`              the loaded library with its prototypes,
      `_options(n, extent, dry)` the options struct of a handle for batches [n <= max_batch][extent],
      `_state(arrays)`          its state struct with the scalar fields of this object, and the three arrays when `arrays`,
      `_read_state(s)`          the scalar fields of a state struct into this object,
      `_checkpoint_extra()`     what a checkpoint holds beside weights and moments,
      `_load_checkpoint_extra(path, f)`  the same read back (refuses a checkpoint of another architecture)."""

    ABI = ""

    def _init_state(self, flat: np.ndarray):
        self._flat = flat
        self._moment1 = self._moment2 = None
        self._handle, self._shape = None, None
        self.last_report: dict = {}

    def _call(self, name: str, *args):
        from . import engine
        engine._check(getattr(self._library(), self.ABI + name)(*args))

    def _zero_moments(self):
        if self._moment1 is None:
            self._moment1, self._moment2 = np.zeros_like(self._flat), np.zeros_like(self._flat)

    # ------------------------------------------------------------------------------------------------------------ the handle
    def _pull(self, arrays: bool = True):
        """The step counts and what else the state struct holds (with `arrays`: weights and moments too) from the device."""
        if self._handle is None:
            return
        if arrays:
            self._zero_moments()
        s = self._state(arrays)
        self._call("get_state", self._handle, C.byref(s))
        self._read_state(s)

    def _push(self, arrays: bool = True):
        if self._handle is not None:
            s = self._state(arrays and self._moment1 is not None)
            self._call("set_state", self._handle, C.byref(s))

    def _destroy(self):
        getattr(self._library(), self.ABI + "destroy")(self._handle)
        self._handle, self._shape = None, None

    def close(self):
        """Brings the state to the host and frees the device."""
        if self._handle is not None:
            self._pull()
            self._destroy()

    def __del__(self):
        try:
            if self._handle is not None:
                self._destroy()
        except Exception:
            pass

    def _ensure(self, n: int, extent):
        """A handle for [n <= max_batch][extent]; a batch of another extent or a larger one makes a new handle with the state kept."""
        extent = tuple(extent)
        if self._handle is not None and self._shape[1:] == extent and n <= self._shape[0]:
            return
        self.close()
        handle = C.c_void_p()
        self._call("create", C.byref(self._options(n, extent)), C.byref(handle))
        self._handle, self._shape = handle, (n,) + extent
        self._push()

    def _planned(self, n: int, extent) -> int:
        """What a trainer for batches [n][extent] holds on the device, planned without touching it."""
        handle, s = C.c_void_p(), self._state(False)
        self._call("create", C.byref(self._options(n, tuple(extent), dry=True)), C.byref(handle))
        try:
            self._call("get_state", handle, C.byref(s))
        finally:
            getattr(self._library(), self.ABI + "destroy")(handle)
        return int(s.planned_device_bytes)

    # ------------------------------------------------------------------------------------------------------------- the files
    def _named(self, flat: np.ndarray) -> Dict[str, np.ndarray]:
        out, at = {}, 0
        for name, shape in self.tensors:
            n = int(np.prod(shape))
            out[name] = flat[at:at + n].reshape(shape).copy()
            at += n
        return out

    def save(self, path) -> Path:
        """`.npz` by the state dict's names, or `.pth` as {"model": state dict} (needs torch)."""
        path = Path(path)
        state = self.state_dict()
        path.parent.mkdir(parents=True, exist_ok=True)
        if path.suffix == ".npz":
            np.savez(path, **state)
        elif path.suffix == ".pth":
            import torch
            torch.save({"model": {k: torch.as_tensor(v) for k, v in state.items()}}, path)
        else:
            raise ValueError(f"{path}: expected .npz or .pth")
        return path

    def save_checkpoint(self, path) -> Path:
        """Weights, both moments and the trainer's `_checkpoint_extra` (`.npz`): a run resumed from it continues bit for bit."""
        self._pull()
        self._zero_moments()
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(path, weights=self._flat, moment1=self._moment1, moment2=self._moment2, **self._checkpoint_extra())
        return path

    def load_checkpoint(self, path):
        with np.load(Path(path)) as f:
            self._load_checkpoint_extra(path, f)
            self._flat = np.ascontiguousarray(f["weights"], dtype=np.float32)
            self._moment1 = np.ascontiguousarray(f["moment1"], dtype=np.float32)
            self._moment2 = np.ascontiguousarray(f["moment2"], dtype=np.float32)
        self._push()
