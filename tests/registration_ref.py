"""The demons registration of DESIGN.md row f14 restated in numpy: the rule in the header of csrc/registration.hip, operation by
operation.  Every function takes `dtype`: float64 is the reference, float32 is the same code in the kernels' precision (the smoothing
of the float32 run is what the kernels compute bit for bit; the error of the float32 run against the float64 one is the yardstick
for the other kernels).  Index tables and Gaussian weights are float64 work on the host in both runs, as the rule says.

Arrays are [x, y, z] (axes 0, 1, 2), fields [3, x, y, z] in voxels, component i along axis i: moving(x + u(x)) ~ fixed(x)."""
from __future__ import annotations

import math

import numpy as np


def level_shape(shape, level):
    return tuple(-(-int(n) // (1 << level)) for n in shape)


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def gaussian_weights(sigma, dtype=np.float64):
    """exp(-k^2 / (2 sigma^2)), k = -r .. r, divided by their sum (float64, summed from k = -r upwards), then rounded to dtype."""
    r = radius(sigma)
    e = [math.exp(-float(k * k) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)]
    total = 0.0
    for v in e:
        total += v
    return np.array([v / total for v in e], dtype=np.float64).astype(dtype)


def smooth_axis(a, axis, sigma, dtype=np.float64):
    """One pass: out[i] = sum over k = -r .. r, ascending and starting from 0, of w_k a[clamp(i + k)], in dtype."""
    if sigma == 0:
        return a
    a = np.asarray(a, dtype=dtype)
    w = gaussian_weights(sigma, dtype)
    r = radius(sigma)
    n = a.shape[axis]
    idx = np.arange(n)
    acc = np.zeros_like(a)
    for k in range(-r, r + 1):
        acc = acc + w[k + r] * np.take(a, np.clip(idx + k, 0, n - 1), axis=axis)
    return acc


def smooth(field, sigma, dtype=np.float64):
    """Step 6: every component along axis 0, then 1, then 2."""
    out = np.asarray(field, dtype=dtype)
    for axis in range(3):
        out = np.stack([smooth_axis(c, axis, sigma[axis], dtype) for c in out])
    return out


def _lerp(a, b, t):
    return a + (b - a) * t


def _blend(vol, lo, hi, t):
    """The eight taps at per-voxel (lo, hi, t) index arrays of one common (broadcast) shape: axis 2, then 1, then 0."""
    (a0, a1, a2), (b0, b1, b2), (t0, t1, t2) = lo, hi, t
    x00, x01 = _lerp(vol[a0, a1, a2], vol[a0, a1, b2], t2), _lerp(vol[a0, b1, a2], vol[a0, b1, b2], t2)
    x10, x11 = _lerp(vol[b0, a1, a2], vol[b0, a1, b2], t2), _lerp(vol[b0, b1, a2], vol[b0, b1, b2], t2)
    return _lerp(_lerp(x00, x01, t1), _lerp(x10, x11, t1), t0)


def sample(vol, coords, dtype=np.float64):
    """Trilinear `vol` at coords [3, ...] (voxel coordinates), each clamped to [0, n - 1]."""
    vol = np.asarray(vol, dtype=dtype)
    lo, hi, t = [], [], []
    for axis in range(3):
        n = vol.shape[axis]
        c = np.clip(np.asarray(coords[axis], dtype=dtype), dtype(0), dtype(n - 1))
        f = np.floor(c)
        i = f.astype(np.int64)
        lo.append(i)
        hi.append(np.minimum(i + 1, n - 1))
        t.append(c - f)
    return _blend(vol, lo, hi, t)


def _grid(shape, dtype):
    return np.meshgrid(*(np.arange(n, dtype=dtype) for n in shape), indexing="ij")


def warp(moving, u, dtype=np.float64):
    """Step 1: moving at x + u."""
    u = np.asarray(u, dtype=dtype)
    g = _grid(u.shape[1:], dtype)
    return sample(moving, [g[i] + u[i] for i in range(3)], dtype)


def resize_tables(n, s):
    """(base, fraction, nearest) of the positions linspace(0, n - 1, s), all float64 / integer work."""
    p = np.linspace(0.0, n - 1, s)
    base = np.minimum(np.floor(p), n - 1)
    return base.astype(np.int64), p - base, np.minimum(np.floor(p + 0.5), n - 1).astype(np.int64)


def resize_linear(vol, shape, dtype=np.float64):
    vol = np.asarray(vol, dtype=dtype)
    lo, hi, t = [], [], []
    for axis in range(3):
        base, frac, _ = resize_tables(vol.shape[axis], shape[axis])
        view = [1, 1, 1]
        view[axis] = -1
        lo.append(base.reshape(view))
        hi.append(np.minimum(base + 1, vol.shape[axis] - 1).reshape(view))
        t.append(frac.astype(np.float32).astype(dtype).reshape(view))  # the rule rounds the fraction to float32
    return _blend(vol, lo, hi, t)


def resize_nearest(mask, shape):
    mask = np.asarray(mask)
    i0, i1, i2 = (resize_tables(mask.shape[axis], shape[axis])[2] for axis in range(3))
    return mask[i0[:, None, None], i1[None, :, None], i2[None, None, :]]


def field_scale(s_old, s_new):
    """What component i is multiplied by when the field goes from level shape s_old to s_new."""
    return [1.0 if o == 1 else float(np.float32((n - 1) / (o - 1))) for o, n in zip(s_old, s_new)]


def resize_field(u, shape, dtype=np.float64):
    scale = field_scale(u.shape[1:], shape)
    return np.stack([resize_linear(u[i], shape, dtype) * dtype(scale[i]) for i in range(3)])


def gradient(fixed, dtype=np.float64):
    """Step 3: 0.5 (f[i + 1] - f[i - 1]) per axis, indices clamped."""
    f = np.asarray(fixed, dtype=dtype)
    out = []
    for axis in range(3):
        idx = np.arange(f.shape[axis])
        n = f.shape[axis]
        out.append(dtype(0.5) * (np.take(f, np.minimum(idx + 1, n - 1), axis=axis) - np.take(f, np.maximum(idx - 1, 0), axis=axis)))
    return out


def force_step(fixed, moving, u, tau, mask=None, dtype=np.float64):
    """Steps 1 to 5: u + tau v."""
    fixed = np.asarray(fixed, dtype=dtype)
    u = np.asarray(u, dtype=dtype)
    d = warp(moving, u, dtype) - fixed
    g = gradient(fixed, dtype)
    den = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + d * d
    active = den > dtype(1e-9)
    if mask is not None:
        active &= np.asarray(mask) != 0
    safe = np.where(active, den, dtype(1))
    return np.stack([u[i] + dtype(tau) * np.where(active, (-d * g[i]) / safe, dtype(0)) for i in range(3)])


def msd(fixed, moving, u, dtype=np.float64):
    d = (warp(moving, u, dtype) - np.asarray(fixed, dtype=dtype)).astype(np.float64)
    return float(np.mean(d * d))


def register(fixed, moving, fixed_mask=None, iterations=800, tau=2.25, sigma=(1.25, 1.25, 1.25), n_levels=3, dtype=np.float64, **_ignored):
    """-> (u [3, x, y, z] in dtype, report dict with msd_before / msd_after per level, index 0 = finest)."""
    fixed = np.asarray(fixed, dtype=dtype)
    moving = np.asarray(moving, dtype=dtype)
    if fixed.shape != moving.shape or fixed.ndim != 3:
        raise ValueError(f"fixed {fixed.shape} and moving {moving.shape}: two volumes of one shape")
    report = dict(msd_before=[0.0] * n_levels, msd_after=[0.0] * n_levels)
    u = None
    for level in range(n_levels - 1, -1, -1):
        shape = level_shape(fixed.shape, level)
        if level == 0:
            f, m, mask = fixed, moving, fixed_mask
        else:
            f, m = resize_linear(fixed, shape, dtype), resize_linear(moving, shape, dtype)
            mask = None if fixed_mask is None else resize_nearest(fixed_mask, shape)
        u = np.zeros((3,) + shape, dtype=dtype) if u is None else resize_field(u, shape, dtype)
        report["msd_before"][level] = msd(f, m, u, dtype)
        for _ in range(iterations):
            u = smooth(force_step(f, m, u, tau, mask, dtype), sigma, dtype)
        report["msd_after"][level] = msd(f, m, u, dtype)
    return u, report


def sphere(shape, centre, radius_voxels=7.0, width=1.0):
    """A sphere with a logistic edge: 1 / (1 + exp((|x - c| - R) / width))."""
    g = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    r = np.sqrt(sum((g[i] - centre[i]) ** 2 for i in range(3)))
    return (1.0 / (1.0 + np.exp((r - radius_voxels) / width))).astype(np.float32)
