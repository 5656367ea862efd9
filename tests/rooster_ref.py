"""Float64 numpy restatement of 4-D ROOSTER (csrc/rooster4d.hip; its header spells out the algorithm), the oracle of
tests/test_rooster4d.py and tests/test_rooster4d_configs.py.  R is joseph_ref.project on the phase blend of two frames; everything
else is restated here:
  weights   phase -> (l, h, w_l, w_h):  t = phi N, l = floor(t) mod N, h = (l + 1) mod N, w_h = t - floor(t), w_l = 1 - w_h
  back      S^T B: voxel-driven bilinear gather (a sample counts only with both detector columns and both rows inside), weight
            (sdd / U)^2 sx sy sz / (du dv), U = sid - z_rot, distributed into frames l and h with w_l and w_h
  tv_*      min 1/2 |u - f|^2 + gamma TV(u) by tviter dual projected-gradient steps from p = 0, tau = 1 / (4 d)
  rooster   optional water pre-correction p <- sum_j c_j p^j, then niter x (cgiter CG steps restarted from x, positivity,
            spatial TV per frame, temporal TV per voxel)
Vectors are [N][nz][ny][nx]; projections [n][nv][nu]."""
from __future__ import annotations

import numpy as np

import joseph_ref as jr


def weights(phase, N):
    t = np.asarray(phase, dtype=np.float64) * N
    ft = np.floor(t)
    l = np.mod(ft.astype(np.int64), N)
    return l, (l + 1) % N, 1.0 - (t - ft), t - ft


class Geometry:
    """Circular cone-beam geometry and grids of one problem (origin None = centred on the isocentre)."""

    def __init__(self, angles, sid, sdd, nu, nv, du, dv, dimension, spacing, phase, frames, offsets_x=None, offsets_y=None, u0=None, v0=None,
                 origin=None):
        self.angles = np.asarray(angles, float)
        n = len(self.angles)
        self.offx = np.zeros(n) if offsets_x is None else np.asarray(offsets_x, float)
        self.offy = np.zeros(n) if offsets_y is None else np.asarray(offsets_y, float)
        self.sid, self.sdd, self.nu, self.nv, self.du, self.dv = sid, sdd, nu, nv, du, dv
        self.u0 = -(nu - 1) / 2 * du if u0 is None else u0
        self.v0 = -(nv - 1) / 2 * dv if v0 is None else v0
        self.dim = tuple(int(d) for d in dimension)       # (nx, ny, nz)
        self.sp = np.asarray(spacing, float)
        self.org = -(np.array(self.dim) - 1) / 2 * self.sp if origin is None else np.asarray(origin, float)
        self.N = int(frames)
        self.l, self.h, self.wl, self.wh = weights(phase, self.N)

    def shape4(self):
        return (self.N, self.dim[2], self.dim[1], self.dim[0])


def forward(g: Geometry, x4):
    """R S: projections [n][nv][nu]."""
    out = np.zeros((len(g.angles), g.nv, g.nu))
    for k, a in enumerate(g.angles):
        blend = g.wl[k] * x4[g.l[k]] + g.wh[k] * x4[g.h[k]]
        out[k] = jr.project(blend, g.sp, g.org, [a], [g.offx[k]], [g.offy[k]], g.sid, g.sdd, g.nu, g.nv, g.du, g.dv, g.u0, g.v0)[0]
    return out


def back(g: Geometry, q):
    """S^T B: 4-D volume."""
    nx, ny, nz = g.dim
    X = g.org[0] + g.sp[0] * np.arange(nx)
    Y = g.org[1] + g.sp[1] * np.arange(ny)
    Z = g.org[2] + g.sp[2] * np.arange(nz)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    K = g.sp.prod() / (g.du * g.dv)
    out = np.zeros(g.shape4())
    for k, a in enumerate(g.angles):
        t = np.deg2rad(a)
        c, s = np.cos(t), np.sin(t)
        xr, zr = xx * c - zz * s, xx * s + zz * c
        U = g.sid - zr
        mag = g.sdd / U
        fu = (mag * xr - g.offx[k] - g.u0) / g.du
        fv = (mag * yy - g.offy[k] - g.v0) / g.dv
        iu, iv = np.floor(fu).astype(int), np.floor(fv).astype(int)
        ok = (U > 0) & (iu >= 0) & (iu < g.nu - 1) & (iv >= 0) & (iv < g.nv - 1)
        iu, iv = np.where(ok, iu, 0), np.where(ok, iv, 0)
        au, av = fu - np.floor(fu), fv - np.floor(fv)
        P = q[k]
        top = P[iv, iu] + au * (P[iv, iu + 1] - P[iv, iu])
        bot = P[iv + 1, iu] + au * (P[iv + 1, iu + 1] - P[iv + 1, iu])
        val = np.where(ok, (top + av * (bot - top)) * mag * mag * K, 0.0)
        out[g.l[k]] += g.wl[k] * val
        out[g.h[k]] += g.wh[k] * val
    return out


# ---- TV ----------------------------------------------------------------------------------------------------------------------
def grad_space(u):
    """Forward differences along x, y, z of u [nz][ny][nx]; the last difference of each axis is 0 (Neumann)."""
    gx, gy, gz = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    gx[:, :, :-1] = u[:, :, 1:] - u[:, :, :-1]
    gy[:, :-1, :] = u[:, 1:, :] - u[:, :-1, :]
    gz[:-1, :, :] = u[1:, :, :] - u[:-1, :, :]
    return gx, gy, gz


def div_space(px, py, pz):
    """-grad^T (px, py, pz)."""
    d = np.zeros_like(px)
    for p, ax in ((px, 2), (py, 1), (pz, 0)):
        n = p.shape[ax]
        sl = lambda a, b: tuple(slice(a, b) if i == ax else slice(None) for i in range(3))  # noqa: E731
        d[sl(0, n - 1)] += p[sl(0, n - 1)]
        d[sl(1, n)] -= p[sl(0, n - 1)]
    return d


def grad_time(u4):
    return np.roll(u4, -1, axis=0) - u4


def div_time(p4):
    return p4 - np.roll(p4, 1, axis=0)


def tv_space(f, iters, gamma):
    """One frame [nz][ny][nx]."""
    p = [np.zeros_like(f) for _ in range(3)]
    for _ in range(iters):
        u = f + div_space(*p)
        q = [pi + gi / 12.0 for pi, gi in zip(p, grad_space(u))]
        nrm = np.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
        s = np.where(nrm > gamma, gamma / np.where(nrm > 0, nrm, 1.0), 1.0)
        p = [qi * s for qi in q]
    return f + div_space(*p)


def tv_time(f4, iters, gamma):
    p = np.zeros_like(f4)
    for _ in range(iters):
        u = f4 + div_time(p)
        p = np.clip(p + 0.25 * grad_time(u), -gamma, gamma)
    return f4 + div_time(p)


def total_variation_space(u):
    g = grad_space(u)
    return float(np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2).sum())


# ---- CG and the main loop ----------------------------------------------------------------------------------------------------
def cg(apply_A, b, x, iters, residuals=None):
    """iters conjugate-gradient steps on A x = b from x (restarted: r = b - A x, d = r)."""
    r = b - apply_A(x)
    d = r.copy()
    rr = float((r * r).sum())
    if residuals is not None:
        residuals.append(np.sqrt(rr))
    for _ in range(iters):
        if rr > 0:
            Ad = apply_A(d)
            dAd = float((d * Ad).sum())
            if dAd > 0:
                alpha = rr / dAd
                x = x + alpha * d
                r = r - alpha * Ad
                rr_new = float((r * r).sum())
                d = r + (rr_new / rr) * d
                rr = rr_new
        if residuals is not None:
            residuals.append(np.sqrt(rr))
    return x


def water_precorrection(p, wpc):
    """sum_j c_j p^j (rtkfdk --wpc), in float64."""
    p = np.asarray(p, dtype=np.float64)
    return sum(c * p ** j for j, c in enumerate(wpc))


def rooster(g: Geometry, projections, niter, cgiter, tviter, gamma_space, gamma_time, positivity=True, residuals=None, wpc=None):
    if wpc is not None and len(wpc) > 0:  # applied to the projections before b, as the kernel does
        projections = water_precorrection(projections, wpc)
    b = back(g, projections)
    A = lambda v: back(g, forward(g, v))  # noqa: E731
    x = np.zeros(g.shape4())
    for _ in range(niter):
        x = cg(A, b, x, cgiter, residuals)
        if positivity:
            x = np.maximum(x, 0.0)
        if tviter > 0:
            x = np.stack([tv_space(x[f], tviter, gamma_space) for f in range(g.N)])
            x = tv_time(x, tviter, gamma_time)
    return x
