"""Restatement in torch functional calls and numpy of the reference's CT segmentation (cbctmc/segmentation/segmenter.py: MCSegmenter
around the 3-D FlexUNet of cbctmc/speedup/models.py, patches and stitching of cbctmc/segmentation/patching.py), written from its
description (csrc/segment_net.hip's header), not from its source: the oracle of tests/test_segmentation.py and
tests/test_segmentation_gpu.py.  The dtype is a parameter: float64 for truth, float32 for the yardstick (what torch gives a
reference user on the CPU).  tests/golden/segment_pin.npz chains the network to the reference class itself.

FlexUNet(1, 9, L, [init, enc_0 .., dec_{L-1} .., final]): init_conv; enc_i = max-pool 2, twice [conv, instance norm,
LeakyReLU(0.01)]; dec_i = nearest upsample x 2, cat([skip_i, upsampled]), twice [conv, norm, LeakyReLU]; final_conv.  Every
convolution 3 x 3 x 3, zero padding, bias."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = Path(__file__).resolve().parent / "golden"
REFERENCE_FILTERS = (32,) * 10
PIN_SEED, PIN_PATCH = 7, (16, 16, 32)


def golden_tensors():
    """[(name, shape)] of FlexUNet(1, 9, 4, n_filters=[32] * 10).state_dict(), in its order."""
    return [(name, tuple(shape)) for name, shape in json.loads((GOLDEN / "segment_state_dict.json").read_text())]


def tensors(n_filters=REFERENCE_FILTERS, levels=4, n_classes=9):
    """[(name, shape)] of the state dict for any filter list [init, enc_0 .. enc_{L-1}, dec_{L-1} .. dec_0, final]."""
    f = list(n_filters)
    assert len(f) == 2 * levels + 2
    conv = lambda name, c_in, c_out: [(f"{name}.weight", (c_out, c_in, 3, 3, 3)), (f"{name}.bias", (c_out,))]  # noqa: E731
    skip = f[:levels + 1]
    out = conv("init_conv", 1, f[0]) + conv("final_conv", f[-1], n_classes)
    for i in range(levels):
        out += conv(f"enc_{i}.convs.0", skip[i], skip[i + 1]) + conv(f"enc_{i}.convs.3", skip[i + 1], skip[i + 1])
    below = skip[levels]
    for j, i in enumerate(reversed(range(levels))):
        c = f[levels + 1 + j]
        out += conv(f"dec_{i}.convs.0", skip[i] + below, c) + conv(f"dec_{i}.convs.3", c, c)
        below = c
    return out


def seeded_weights(seed: int, n_filters=REFERENCE_FILTERS, levels=4) -> dict:
    """Weights by name, drawn with numpy in state-dict order: every weight and bias uniform in +-1 / sqrt(27 C_in), the distribution
    torch gives a fresh Conv3d."""
    rng = np.random.default_rng(seed)
    out, bound = {}, 0.0
    for name, shape in tensors(n_filters, levels):
        if name.endswith(".weight"):
            bound = 1.0 / np.sqrt(27 * shape[1])
        out[name] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


def seeded_image(seed: int, shape, dtype=np.int16) -> np.ndarray:
    """A CT-like image in HU: smooth structure between air and bone plus noise, with a few values outside [-1024, 3071]."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij")
    smooth = np.sin(7.0 * z + 2.0 * y) * np.cos(5.0 * y - 3.0 * x) + np.sin(11.0 * x * z)
    image = 300.0 + 900.0 * smooth + rng.normal(0.0, 400.0, size=shape)
    image[rng.random(shape) < 0.01] = 3500.0
    image[rng.random(shape) < 0.01] = -1100.0
    return np.round(image).astype(dtype)


def rescale(image, input_range=(-1024, 3071), output_range=(0, 1)) -> np.ndarray:
    """Step 1 of the procedure, in float32 operation by operation: ((v - in_min) (out_max - out_min)) / (in_max - in_min) + out_min,
    clipped; nothing at all when the two ranges are equal."""
    v = np.asarray(image, dtype=np.float32)
    if tuple(input_range) == tuple(output_range):
        return v
    f = np.float32
    v = ((v - f(input_range[0])) * f(output_range[1] - output_range[0])) / f(input_range[1] - input_range[0]) + f(output_range[0])
    return np.clip(v, f(output_range[0]), f(output_range[1]))


def conv3(x, weight, bias):
    return F.conv3d(x, weight, bias, padding=1)


def norm_lrelu(x):
    return F.leaky_relu(F.instance_norm(x, eps=1e-5), 0.01)


def unet(x, w):
    """logits [1, 9, ...] of x [1, 1, d0, d1, d2]; the levels are read from the names."""
    levels = 1 + max(int(k.split(".")[0][4:]) for k in w if k.startswith("enc_"))
    skips = [conv3(x, w["init_conv.weight"], w["init_conv.bias"])]
    for i in range(levels):
        y = F.max_pool3d(skips[-1], 2)
        for j in (0, 3):
            y = norm_lrelu(conv3(y, w[f"enc_{i}.convs.{j}.weight"], w[f"enc_{i}.convs.{j}.bias"]))
        skips.append(y)
    y = skips[-1]
    for i in reversed(range(levels)):
        y = torch.cat([skips[i], F.interpolate(y, scale_factor=2, mode="nearest")], dim=1)
        for j in (0, 3):
            y = norm_lrelu(conv3(y, w[f"dec_{i}.convs.{j}.weight"], w[f"dec_{i}.convs.{j}.bias"]))
    return conv3(y, w["final_conv.weight"], w["final_conv.bias"])


def head(logits):
    """[1, 9, ...]: softmax over channels 0 .. 7, sigmoid on channel 8."""
    return torch.cat([torch.softmax(logits[:, :8], dim=1), torch.sigmoid(logits[:, 8:9])], dim=1)


def as_tensors(weights: dict, dtype):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype) for k, v in weights.items()}


def logits_of(weights: dict, patch: np.ndarray, dtype=torch.float64) -> np.ndarray:
    """[9, d0, d1, d2] of one rescaled patch."""
    with torch.no_grad():
        return unet(torch.as_tensor(patch[None, None], dtype=dtype), as_tensors(weights, dtype))[0].numpy()


# ---------------------------------------------------------------------------------------------------------------- patches
def axis_starts(n: int, p: int, s: int):
    return [min(v, n - p) for v in range(0, n - p + s + 1, s)]


def patch_starts(array_shape, patch_shape, stride):
    """All starts in the reference's order (meshgrid "ij": the last axis fastest), repeats included; plain integers."""
    axes = [axis_starts(n, p, s) for n, p, s in zip(array_shape, patch_shape, stride)]
    return [(i, j, k) for i in axes[0] for j in axes[1] for k in axes[2]]


def pad_image(image: np.ndarray, patch_shape, value=0.0) -> np.ndarray:
    pads = []
    for n, p in zip(image.shape, patch_shape):
        extra = max(p - n, 0)
        pads.append((extra // 2, extra - extra // 2))
    return np.pad(image, pads, mode="constant", constant_values=value)


class Stitcher:
    """The first value k, the sum of (value - k) and the count n per voxel; mean = k + sum / n.  float32 as the reference keeps them,
    or float64 for truth."""

    def __init__(self, shape, dtype=np.float32):
        self.k, self.sum, self.n = np.zeros(shape, dtype), np.zeros(shape, dtype), np.zeros(shape, np.uint32)

    def add(self, data, start):
        where = (slice(None),) + tuple(slice(s, s + p) for s, p in zip(start, data.shape[1:]))
        first = self.n[where] == 0
        self.k[where][first] = data[first]
        self.n[where] += 1
        self.sum[where] += (data - self.k[where]).astype(self.k.dtype)

    def mean(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.nan_to_num(self.k + self.sum / self.n.astype(self.k.dtype), nan=0.0)


def finalize(mean: np.ndarray) -> np.ndarray:
    """uint8 [9, ...]: one-hot of the argmax of channels 0 .. 7 (numpy's argmax: the first maximum), channel 8 > 0.5."""
    out = np.zeros(mean.shape, np.uint8)
    out[:8] = np.eye(8, dtype=np.uint8)[:, np.argmax(mean[:8], axis=0)]
    out[8] = mean[8] > 0.5
    return out


def segment(weights: dict, image, patch_shape, patch_overlap=0.0, dtype=torch.float64):
    """(labels uint8, raw) [9, padded shape] by the reference's procedure, every patch of the rule in its order, repeats included
    (the network is evaluated once per distinct start: it is deterministic).  float64: network, head and stitcher in float64;
    float32: all three in float32, as a reference user gets them without autocast."""
    stride = [(1.0 - patch_overlap) * p for p in patch_shape]
    assert all(s == int(s) and s >= 1 for s in stride)
    x = pad_image(rescale(image), patch_shape)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    stitcher = Stitcher((9,) + x.shape, np_dtype)
    w, cache = as_tensors(weights, dtype), {}
    with torch.no_grad():
        for start in patch_starts(x.shape, patch_shape, [int(s) for s in stride]):
            if start not in cache:
                patch = x[tuple(slice(s, s + p) for s, p in zip(start, patch_shape))]
                cache[start] = head(unet(torch.as_tensor(patch[None, None], dtype=dtype), w))[0].numpy()
            stitcher.add(cache[start], start)
    raw = stitcher.mean()
    return finalize(raw), raw
