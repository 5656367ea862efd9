"""What speedup.py and segmentation.py share around the reference's `FlexUNet` (cbctmc/speedup/models.py): the order and shapes of its
state dict, the reader of a weights file, the check of a state dict against the expected tensors with its flattening into the one
float32 array the C ABI takes (the order `csrc/unet_common.inc`'s NetLayers counts in), and the small ctypes helpers."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np


def unet_tensors(n_filters: Sequence[int], levels: int, n_classes: int, in_channels: int, ndim: int, prefix: str = "") -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of FlexUNet(in_channels, n_classes, levels, n_filters=[init, enc_0.., dec_{L-1}.., final]).state_dict(), in its
    order: init_conv, final_conv, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0; each block holds its two convolutions as convs.0, convs.3."""
    f = [int(v) for v in n_filters]
    if len(f) != 2 * levels + 2:
        raise ValueError(f"{len(f)} filter counts for {levels} levels, expected {2 * levels + 2}")

    def conv(name, c_in, c_out):
        return [(f"{prefix}{name}.weight", (c_out, c_in) + (3,) * ndim), (f"{prefix}{name}.bias", (c_out,))]
    skip = [f[0]] + f[1:1 + levels]
    out = conv("init_conv", in_channels, f[0]) + conv("final_conv", f[-1], n_classes)
    for i in range(levels):
        out += conv(f"enc_{i}.convs.0", skip[i], skip[i + 1]) + conv(f"enc_{i}.convs.3", skip[i + 1], skip[i + 1])
    below = skip[levels]
    for j, i in enumerate(reversed(range(levels))):
        c = f[1 + levels + j]
        out += conv(f"dec_{i}.convs.0", skip[i] + below, c) + conv(f"dec_{i}.convs.3", c, c)
        below = c
    return out


def read_weights(model_filepath) -> Dict[str, np.ndarray]:
    """A `.pth` as the reference's trainer writes it ({"model": state dict}; read with torch) or a `.npz` with the same names."""
    path = Path(model_filepath)
    if path.suffix == ".npz":
        with np.load(path) as f:
            return {k: f[k] for k in f.files}
    import torch
    state = torch.load(path, map_location="cpu")["model"]
    return {k: v.detach().cpu().numpy() for k, v in state.items()}


def flatten(weights: Dict[str, np.ndarray], expected, shape_prefix: str = "") -> np.ndarray:
    """The tensors of `expected`, in its order, as one float32 array.  Refused by name: the first missing key or wrong shape in that
    order, then the first key (sorted) that is not expected."""
    for name, shape in expected:
        if name not in weights:
            raise ValueError(f"missing key {name}")
        if tuple(np.shape(weights[name])) != shape:
            raise ValueError(f"{shape_prefix}{name} has shape {tuple(np.shape(weights[name]))}, expected {shape}")
    extra = sorted(set(weights) - {name for name, _ in expected})
    if extra:
        raise ValueError(f"unexpected key {extra[0]}")
    return np.concatenate([np.asarray(weights[name], dtype=np.float32).ravel() for name, _ in expected])


def report_dict(rep) -> dict:
    """A report struct of the C ABI as a dict of its fields."""
    return {name: getattr(rep, name) for name, _ in rep._fields_}


def f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def ptr(a):
    return None if a is None else a.ctypes.data
