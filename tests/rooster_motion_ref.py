"""Float64 numpy restatement of motion-aware 4-D ROOSTER (csrc/rooster4d.hip, whose header states the rule),
the oracle of tests/test_rooster4d_motion.py.  Everything that is not motion comes from rooster_ref.
  warp            the sampling operator Sigma(model, delta) frame by frame: displacement d = mean + sum_k coefficients[k] delta[f][k]
                  [mm]; index position i + d / spacing per axis, clamped to [0, n - 1] (the border is replicated); i0 = floor,
                  t = position - i0, i1 = min(i0 + 1, n - 1); trilinear, lerp(a, b, t) = a + t (b - a) along x, then y, then z
  motion_tv_time  x + U (TVtime(W x) - W x), W = warp with the model to the reference, U = warp with the model from it
  rooster_motion  rooster_ref.rooster with that temporal step
  frame_signals   the state of every frame: the mean of the projections' signals weighted by rooster_ref.weights
Volumes are [N][nz][ny][nx]; a model is (mean [3][nz][ny][nx], coefficients [K][3][nz][ny][nx]) in mm along IEC X, Y, Z; delta is
[N][K]."""
from __future__ import annotations

import numpy as np

import rooster_ref as rr


def warp(x4, mean, coefficients, delta, spacing, dtype=np.float64):
    """Sigma(model, delta[f]) x4[f] for every frame.  dtype: the type of the displacement and the position (float32 restates the
    kernel's coordinate arithmetic; the interpolation itself stays in float64)."""
    x4 = np.asarray(x4, dtype=np.float64)
    N, nz, ny, nx = x4.shape
    mean = np.asarray(mean, dtype=dtype)
    coefficients = np.asarray(coefficients, dtype=dtype)
    delta = np.asarray(delta, dtype=dtype).reshape(N, -1)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = np.empty_like(x4)
    for f in range(N):
        d = mean.copy()
        for k in range(coefficients.shape[0]):
            d = d + coefficients[k] * delta[f, k]
        cell = []
        for comp, idx, n in ((0, ix, nx), (1, iy, ny), (2, iz, nz)):
            inv = dtype(1.0 / spacing[comp])
            pos = d[comp] * inv + idx.astype(dtype)
            pos = np.where(np.isnan(pos), 0.0, pos)          # fmaxf(NaN, 0) = 0
            pos = np.minimum(np.maximum(pos, 0), n - 1).astype(dtype)
            i0 = np.floor(pos).astype(np.int64)
            cell.append((i0, np.minimum(i0 + 1, n - 1), (pos - i0).astype(np.float64)))
        (x0, x1, tx), (y0, y1, ty), (z0, z1, tz) = cell
        v = x4[f]
        lerp = lambda a, b, t: a + t * (b - a)  # noqa: E731
        a00, a01 = lerp(v[z0, y0, x0], v[z0, y0, x1], tx), lerp(v[z0, y1, x0], v[z0, y1, x1], tx)
        a10, a11 = lerp(v[z1, y0, x0], v[z1, y0, x1], tx), lerp(v[z1, y1, x0], v[z1, y1, x1], tx)
        out[f] = lerp(lerp(a00, a01, ty), lerp(a10, a11, ty), tz)
    return out


def motion_tv_time(x4, to_reference, from_reference, delta_to, delta_from, spacing, iters, gamma):
    """x + U (TVtime(W x) - W x).  to_reference / from_reference: (mean, coefficients)."""
    x4 = np.asarray(x4, dtype=np.float64)
    y = warp(x4, *to_reference, delta_to, spacing)
    return x4 + warp(rr.tv_time(y, iters, gamma) - y, *from_reference, delta_from, spacing)


def rooster_motion(g: rr.Geometry, projections, niter, cgiter, tviter, gamma_space, gamma_time, to_reference, from_reference, delta_to, delta_from,
                   positivity=True, residuals=None, wpc=None):
    """rooster_ref.rooster with step 4 run along the models' trajectories."""
    if wpc is not None and len(wpc) > 0:
        projections = rr.water_precorrection(projections, wpc)
    b = rr.back(g, projections)
    A = lambda v: rr.back(g, rr.forward(g, v))  # noqa: E731
    x = np.zeros(g.shape4())
    for _ in range(niter):
        x = rr.cg(A, b, x, cgiter, residuals)
        if positivity:
            x = np.maximum(x, 0.0)
        if tviter > 0:
            x = np.stack([rr.tv_space(x[f], tviter, gamma_space) for f in range(g.N)])
            x = motion_tv_time(x, to_reference, from_reference, delta_to, delta_from, g.sp, tviter, gamma_time)
    return x


def frame_signals(phase, signals, N):
    """[N][K]: per frame the mean of the signals of the projections that touch it, weighted by the S rule's weights."""
    s = np.asarray(signals, dtype=np.float64)
    s = s[:, None] if s.ndim == 1 else s
    l, h, wl, wh = rr.weights(phase, N)
    out = np.zeros((N, s.shape[1]))
    for f in range(N):
        w = wl * (l == f) + wh * (h == f)
        if not w.sum() > 0:
            raise ValueError(f"no projection touches frame {f}")
        out[f] = (w[:, None] * s).sum(axis=0) / w.sum()
    return out
