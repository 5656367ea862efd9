"""Float64 numpy restatement of the Joseph forward projector (csrc/forward_project.hip), the oracle of tests/test_forward_projection.py and
tests/test_forward_projection_configs.py (`project`: whole stacks; `project_rays`: a chosen set of rays of a large stack).

Geometry (RTK circular, as CircularGeometry.matrix): source at Ry(angle) (0, 0, sid); pixel (u, v) at rotated-frame position
(u + offset_x, v + offset_y, sid - sdd).  Volume [nz][ny][nx] in the IEC frame, voxel (0,0,0) centred at `origin`; it spans half a
voxel beyond its outer voxel centres and is 0 outside.  Scheme as RTK documents it:
  - main axis = the largest component of the ray direction in index coordinates (first of equal components);
  - samples where the ray crosses the voxel-centre planes ns..fs of the main axis (ns, fs = the planes nearest to where the
    clipped ray enters and leaves), each a bilinear interpolation in the other two axes with taps outside the volume at 0;
  - the first and last steps weighted by the fraction of a step the clipped ray covers (one sample: the whole clipped length);
  - the sum scaled by the length in mm of one main-axis step.
"""
from __future__ import annotations

import numpy as np


def ray_endpoints(angle_deg, offset_x, offset_y, sid, sdd, u, v):
    """Source (3,) and pixel positions (..., 3) in world coordinates for detector coordinates u, v (broadcast)."""
    t = np.deg2rad(angle_deg)
    c, s = np.cos(t), np.sin(t)
    xr, yr = np.asarray(u, float) + offset_x, np.asarray(v, float) + offset_y
    xr, yr = np.broadcast_arrays(xr, yr)
    zr = sid - sdd
    P = np.stack([c * xr + s * zr, yr, -s * xr + c * zr], axis=-1)
    S = np.array([s * sid, 0.0, c * sid])
    return S, P


def project(vol, spacing, origin, angles, offsets_x, offsets_y, sid, sdd, nu, nv, du, dv, u0, v0):
    """vol [nz][ny][nx] -> projections [n][nv][nu] (float64)."""
    vol = np.asarray(vol, dtype=np.float64)
    N = np.array(vol.shape[::-1])  # (nx, ny, nz)
    sp, org = np.asarray(spacing, float), np.asarray(origin, float)
    uu, vv = np.meshgrid(u0 + du * np.arange(nu), v0 + dv * np.arange(nv))
    out = np.zeros((len(angles), nv, nu))
    for p, a in enumerate(angles):
        S, P = ray_endpoints(a, offsets_x[p], offsets_y[p], sid, sdd, uu.ravel(), vv.ravel())
        D = P - S
        Si, Di = (S - org) / sp, D / sp
        out[p] = _trace(vol, N, Si, Di, np.linalg.norm(D, axis=1)).reshape(nv, nu)
    return out


def project_rays(vol, spacing, origin, angles, offsets_x, offsets_y, sid, sdd, du, dv, u0, v0, p, iu, iv):
    """Line integrals (float64, 1-D) of the rays (projection p[i], pixel column iu[i], row iv[i]) only: the same entries of
    `project`, bit for bit, without tracing the rest of the stack.  `vol` is read as it is (a float32 volume is converted voxel by
    voxel inside the gather, never as a whole)."""
    vol = np.asarray(vol)
    N = np.array(vol.shape[::-1])
    sp, org = np.asarray(spacing, float), np.asarray(origin, float)
    p, iu, iv = (np.asarray(v, dtype=np.int64).ravel() for v in (p, iu, iv))
    out = np.zeros(p.size)
    for q in np.unique(p):
        sel = np.flatnonzero(p == q)
        S, P = ray_endpoints(angles[q], offsets_x[q], offsets_y[q], sid, sdd, u0 + du * iu[sel], v0 + dv * iv[sel])
        D = P - S
        out[sel] = _trace(vol, N, (S - org) / sp, D / sp, np.linalg.norm(D, axis=1))
    return out


def _trace(vol, N, Si, Di, dlen):
    R = Di.shape[0]
    t0, t1 = np.zeros(R), np.ones(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            lo, hi = -0.5, N[a] - 0.5
            ta, tb = (lo - Si[a]) / Di[:, a], (hi - Si[a]) / Di[:, a]
            tmin, tmax = np.minimum(ta, tb), np.maximum(ta, tb)
            par = Di[:, a] == 0
            inside = (Si[a] >= lo) & (Si[a] <= hi)
            tmin = np.where(par, np.where(inside, -np.inf, np.inf), tmin)
            tmax = np.where(par, np.where(inside, np.inf, -np.inf), tmax)
            t0, t1 = np.maximum(t0, tmin), np.minimum(t1, tmax)
    m = np.argmax(np.abs(Di), axis=1)
    r = np.arange(R)
    a1 = np.where(m == 0, 1, 0)
    a2 = np.where(m == 2, 1, 2)
    Sm, Dm = Si[m], Di[r, m]
    S1, D1, S2, D2 = Si[a1], Di[r, a1], Si[a2], Di[r, a2]
    e0, e1 = Sm + t0 * Dm, Sm + t1 * Dm
    lo, hi = np.minimum(e0, e1), np.maximum(e0, e1)
    hit = t0 < t1
    ns = np.maximum(np.floor(lo + 0.5), 0).astype(int)
    fs = np.minimum(np.floor(hi + 0.5), N[m] - 1).astype(int)
    hit &= ns <= fs
    r1, r2 = D1 / Dm, D2 / Dm
    w_first = np.where(ns == fs, hi - lo, ns + 0.5 - lo)
    w_last = hi - fs + 0.5
    na, nb = N[a1], N[a2]
    acc = np.zeros(R)
    for k in range(int(N.max())):
        act = hit & (k >= ns) & (k <= fs)
        if not act.any():
            continue
        A = S1 + (k - Sm) * r1
        B = S2 + (k - Sm) * r2
        ia, ib = np.floor(A).astype(int), np.floor(B).astype(int)
        fa, fb = A - ia, B - ib
        val = np.zeros(R)
        for da, db, w in ((0, 0, (1 - fa) * (1 - fb)), (1, 0, fa * (1 - fb)), (0, 1, (1 - fa) * fb), (1, 1, fa * fb)):
            qa, qb = ia + da, ib + db
            ok = act & (qa >= 0) & (qa < na) & (qb >= 0) & (qb < nb) & (k < N[m])
            x = np.where(m == 0, k, qa)
            y = np.where(m == 1, k, np.where(m == 0, qa, qb))
            z = np.where(m == 2, k, qb)
            x, y, z = np.clip(x, 0, N[0] - 1), np.clip(y, 0, N[1] - 1), np.clip(z, 0, N[2] - 1)
            val += np.where(ok, w * vol[z, y, x], 0.0)
        wk = np.where(k == ns, w_first, np.where(k == fs, w_last, 1.0))
        acc += np.where(act, wk * val, 0.0)
    return np.where(hit, acc * dlen / np.abs(Dm), 0.0)


def ambiguous_main_axis(angles, offsets_x, offsets_y, sid, sdd, nu, nv, du, dv, u0, v0, spacing, rel=1e-5):
    """[n][nv][nu] mask of rays whose two largest index-space direction components are within `rel`: float32 and float64 may
    pick different main axes there (both are valid Joseph samplings, but not the same sum)."""
    uu, vv = np.meshgrid(u0 + du * np.arange(nu), v0 + dv * np.arange(nv))
    out = np.zeros((len(angles), nv, nu), dtype=bool)
    for p, a in enumerate(angles):
        S, P = ray_endpoints(a, offsets_x[p], offsets_y[p], sid, sdd, uu.ravel(), vv.ravel())
        d = np.sort(np.abs((P - S) / np.asarray(spacing, float)), axis=1)
        out[p] = (d[:, 2] - d[:, 1] <= rel * d[:, 2]).reshape(nv, nu)
    return out


def ambiguous_main_axis_rays(angles, offsets_x, offsets_y, sid, sdd, du, dv, u0, v0, p, iu, iv, spacing, rel=1e-5):
    """`ambiguous_main_axis` of the rays (p[i], iu[i], iv[i]) only (1-D bool)."""
    p, iu, iv = (np.asarray(v, dtype=np.int64).ravel() for v in (p, iu, iv))
    out = np.zeros(p.size, dtype=bool)
    for q in np.unique(p):
        sel = np.flatnonzero(p == q)
        S, P = ray_endpoints(angles[q], offsets_x[q], offsets_y[q], sid, sdd, u0 + du * iu[sel], v0 + dv * iv[sel])
        d = np.sort(np.abs((P - S) / np.asarray(spacing, float)), axis=1)
        out[sel] = d[:, 2] - d[:, 1] <= rel * d[:, 2]
    return out
