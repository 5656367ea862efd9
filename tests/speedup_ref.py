"""Restatement in torch functional calls of the reference's speed-up network (cbctmc/speedup/models.py: MCSpeedUpUNet behind
inference.py: MCSpeedup), written from its description (csrc/speedup_net.hip's header), not from its source: the oracle of
tests/test_speedup.py and tests/test_speedup_gpu.py.  The dtype is a parameter: float64 for truth, float32 for the yardstick (what a
reference user gets from torch).  tests/golden/speedup_pin.npz chains it to the reference class itself.

FlexUNet(L levels): init_conv; enc_i = max-pool 2, twice [conv, instance norm, LeakyReLU(0.01)]; dec_i = nearest upsample x 2,
cat([skip_i, upsampled]), twice [conv, norm, LeakyReLU]; final_conv.  Every convolution 3 x 3, replicate padding, bias."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = Path(__file__).resolve().parent / "golden"


def golden_tensors():
    """[(name, shape)] of MCSpeedUpUNet(2, 2).state_dict(), in its order (var_scale included)."""
    return [(name, tuple(shape)) for name, shape in json.loads((GOLDEN / "speedup_state_dict.json").read_text())]


def seeded_weights(seed: int, tensors=None) -> dict:
    """Weights by name, drawn in golden order: convolutions N(0, 2 / (9 C_in)), biases N(0, 0.1^2), var_scale 0.001; the two final
    convolutions (weight and bias) damped (x 0.05 / x 0.25) so that neither the tanh nor the relu of the head saturates."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in (tensors if tensors is not None else golden_tensors()):
        if name == "var_scale":
            out[name] = np.full(shape, 0.001)
        elif name.endswith(".weight"):
            out[name] = rng.normal(0.0, np.sqrt(2.0 / (9 * shape[1])), size=shape)
        else:
            out[name] = rng.normal(0.0, 0.1, size=shape)
    for net, damp in (("mean_net", 0.05), ("var_net", 0.25)):  # the whole layer: its one bias alone, undamped, shifts every pixel
        for part in ("weight", "bias"):                       # by 10 tanh(N(0, 0.1)) ~ +-1 and clips 12 % of seed 7's mean to zero
            out[f"{net}.final_conv.{part}"] = out[f"{net}.final_conv.{part}"] * damp
    return {k: v.astype(np.float32) for k, v in out.items()}


def seeded_inputs(seed: int, n: int, nv: int, nu: int):
    """(low_photon, forward_projection) [n, nv, nu] float32, both uniform on [1, 4]."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(1.0, 4.0, size=(n, nv, nu)).astype(np.float32), rng.uniform(1.0, 4.0, size=(n, nv, nu)).astype(np.float32))


def conv3x3(x, weight, bias):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), weight, bias)


def norm_lrelu(x):
    return F.leaky_relu(F.instance_norm(x, eps=1e-5), 0.01)


def unet(x, w, prefix: str):
    t = lambda name: w[f"{prefix}.{name}"]  # noqa: E731
    levels = 1 + max(int(k.split(".")[1][4:]) for k in w if k.startswith(f"{prefix}.enc_"))
    skips = [conv3x3(x, t("init_conv.weight"), t("init_conv.bias"))]
    for i in range(levels):
        y = F.max_pool2d(skips[-1], 2)
        for j in (0, 3):
            y = norm_lrelu(conv3x3(y, t(f"enc_{i}.convs.{j}.weight"), t(f"enc_{i}.convs.{j}.bias")))
        skips.append(y)
    y = skips[-1]
    for i in reversed(range(levels)):
        y = torch.cat([skips[i], F.interpolate(y, scale_factor=2, mode="nearest")], dim=1)
        for j in (0, 3):
            y = norm_lrelu(conv3x3(y, t(f"dec_{i}.convs.{j}.weight"), t(f"dec_{i}.convs.{j}.bias")))
    return conv3x3(y, t("final_conv.weight"), t("final_conv.bias"))


def preprocess(low_photon, forward_projection):
    """[n, 1, H, W] tensors: the forward projection matched to the low-photon projection in mean and unbiased std, per sample."""
    d = (2, 3)
    fp = forward_projection - forward_projection.mean(dim=d, keepdim=True)
    fp = fp / forward_projection.std(dim=d, keepdim=True)
    return fp * low_photon.std(dim=d, keepdim=True) + low_photon.mean(dim=d, keepdim=True)


def predict(weights: dict, low_photon: np.ndarray, forward_projection, dtype=torch.float64, device="cpu"):
    """(mean, variance) [n, nv, nu] as numpy arrays of `dtype`; every sample runs alone, as the reference's batches of
    independent samples do."""
    w = {k: torch.as_tensor(np.asarray(v), dtype=dtype, device=device) for k, v in weights.items() if k != "var_scale"}
    means, variances = [], []
    with torch.no_grad():
        for p in range(low_photon.shape[0]):
            lp = torch.as_tensor(low_photon[p:p + 1, None], dtype=dtype, device=device)
            x = lp
            if forward_projection is not None:
                x = torch.cat([lp, preprocess(lp, torch.as_tensor(forward_projection[p:p + 1, None], dtype=dtype, device=device))], dim=1)
            mean = torch.relu(lp + 10.0 * torch.tanh(unet(x, w, "mean_net")))
            variance = mean * (0.10 * torch.sigmoid(unet(mean, w, "var_net"))) + 1e-6
            means.append(mean[0, 0].cpu().numpy())
            variances.append(variance[0, 0].cpu().numpy())
    return np.stack(means), np.stack(variances)


def normals(seed: int, n: int, nv: int, nu: int, first_projection: int = 0) -> np.ndarray:
    """z [n, nv, nu] in float64 of the sampler: Philox4x32-10, key (seed low, seed high), counter (x, y, projection, 0);
    u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1], u2 = (w1 >> 8) 2^-24, z = sqrt(-2 ln u1) cos(2 pi u2)."""
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
    import fast_rng
    p, y, x = np.meshgrid(np.arange(n, dtype=np.uint64) + np.uint64(first_projection), np.arange(nv, dtype=np.uint64), np.arange(nu, dtype=np.uint64),
                          indexing="ij")
    w = fast_rng.philox4x32([x, y, p, np.zeros_like(x)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], rounds=10)
    u1 = ((w[0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
