"""Float64 restatement of motion-compensated FDK (the rule stands above backproject_motion_kernel in
csrc/fdk.hip), built from the pieces of oracle/fdk_oracle.py.  TEST INFRASTRUCTURE.

The grid is the FDK grid [nz][ny][nx] in RTK's IEC frame.  A motion model on it: mean [3][nz][ny][nx] (mm, along IEC X, Y, Z),
coefficients [K][3][nz][ny][nx] (mm per signal unit), delta [n][K] = signal_i - mean_signal (rounded once to float32, as the device
does).  For the voxel at P and projection i:  P' = P + mean + sum_k coefficients[k] delta[i][k], and the projection gives the voxel
what plain FDK gives at P':  xr = X'c - Z's, zr = X's + Z'c, U = sid - zr, mag = sdd / U, fu = (mag xr - off_x - u0_p) / du,
fv = (mag Y' - off_y - v0) / dv, weight gap_i (sid / U)^2, bilinear sample of the filtered, padded rows.  A sample counts only when
U > 0, columns iu, iu + 1 lie inside the padded detector and rows iv, iv + 1 inside the detector.  The filter chain (weights,
padding, --pad extension, ramp, hannY, water pre-correction) is fdk_oracle.reconstruct's, from the same functions."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import fdk_oracle as fo  # noqa: E402


def filtered_rows(proj, du, dv, u0, v0, sid, sdd, off_x, off_y, hann=0.0, hann_y=0.0, wpc=None, pad=0.0, ramp="direct"):
    """The rows the back-projector samples: (q [n][nv][nu_p] float64, nu_p, u0_p), step by step what fdk_oracle.reconstruct does to
    a projection before it back-projects it."""
    proj = np.asarray(proj)
    n, nv, nu = proj.shape
    pad_l, pad_r = fo.symmetric_padding(nu, du, u0, float(off_x.min()), float(off_x.max()))
    nu_p, u0_p = nu + pad_l + pad_r, u0 - pad_l * du
    nxt = int(min(np.ceil(pad * nu_p), nu_p - 1)) if pad > 0 else 0
    h = fo.ramp_kernel(nu_p + 2 * nxt - 1, hann)
    ky = fo.hann_y_kernel(hann_y)
    out = np.empty((n, nv, nu_p), dtype=np.float64)
    for k in range(n):
        pk = proj[k].astype(np.float64)
        if wpc is not None and len(wpc):
            acc, pw = np.zeros_like(pk), np.ones_like(pk)
            for c in wpc:
                acc += c * pw
                pw *= pk
            pk = acc
        up = u0 + du * np.arange(nu) + off_x[k]
        vp = v0 + dv * np.arange(nv) + off_y[k]
        w_cos = sdd / np.sqrt(sdd * sdd + up[None, :] ** 2 + vp[:, None] ** 2)
        p = np.pad(pk * w_cos * fo.displaced_weights(up, sdd)[None, :], ((0, 0), (pad_l, pad_r)))
        p, _ = fo.truncation_extension(p, pad)
        q = fo.ramp_rows(p, h, nxt, nu_p, ramp)
        q *= (sdd / sid) / du
        if ky.size > 1:
            hk = ky.size // 2
            qp = np.pad(q, ((hk, hk), (0, 0)), mode="edge")
            q = sum(ky[j] * qp[j: j + nv] for j in range(ky.size))
        out[k] = q
    return out, nu_p, u0_p


def _displaced(mean, coefficients, delta_k, dim, spacing, origin):
    """P' = P + mean + sum_k coefficients[k] delta[k] for every voxel: X', Y', Z' [nz][ny][nx] in float64 (delta through float32)."""
    X, Y, Z = fo.volume_axes(dim, spacing, origin)
    d = np.asarray(mean, dtype=np.float64).copy()
    for k, c in enumerate(np.asarray(coefficients)):
        d += np.asarray(c, dtype=np.float64) * np.float64(np.float32(delta_k[k]))
    return X[None, None, :] + d[0], Y[None, :, None] + d[1], Z[:, None, None] + d[2]


def _detector_point(Xp, Yp, Zp, gantry_deg, sid, sdd, off_x, off_y, u0_p, v0, du, dv):
    t = np.deg2rad(gantry_deg)
    c, s = np.cos(t), np.sin(t)
    xr, zr = Xp * c - Zp * s, Xp * s + Zp * c
    U = sid - zr
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = sdd / U
        return (mag * xr - off_x - u0_p) / du, (mag * Yp - off_y - v0) / dv, U


def reconstruct(proj, du, dv, u0, v0, sid, sdd, gantry_deg, off_x, off_y, mean, coefficients, delta, dim, spacing, origin=None, hann=0.0,
                hann_y=0.0, wpc=None, pad=0.0, ramp="direct", stats=None):
    """proj [n][nv][nu] -> volume [nz][ny][nx] float64 by the rule of the header.  stats (a dict) receives how many (voxel,
    projection) samples the range test refused along u and along v."""
    proj = np.asarray(proj)
    n, nv, nu = proj.shape
    off_x = np.broadcast_to(np.asarray(off_x, dtype=np.float64), (n,))
    off_y = np.broadcast_to(np.asarray(off_y, dtype=np.float64), (n,))
    delta = np.asarray(delta, dtype=np.float64).reshape(n, -1)
    q_all, nu_p, u0_p = filtered_rows(proj, du, dv, u0, v0, sid, sdd, off_x, off_y, hann, hann_y, wpc, pad, ramp)
    dbeta = fo.angular_gaps(gantry_deg)
    vol = np.zeros((dim[2], dim[1], dim[0]), dtype=np.float64)
    out_u = out_v = 0
    for k in range(n):
        q = q_all[k]
        Xp, Yp, Zp = _displaced(mean, coefficients, delta[k], dim, spacing, origin)
        fu, fv, U = _detector_point(Xp, Yp, Zp, gantry_deg[k], sid, sdd, off_x[k], off_y[k], u0_p, v0, du, dv)
        ok_U = U > 0
        fu, fv = np.where(ok_U, fu, -1.0), np.where(ok_U, fv, -1.0)
        iu, iv = np.floor(fu).astype(np.int64), np.floor(fv).astype(np.int64)
        au, av = fu - iu, fv - iv
        ok_u, ok_v = (iu >= 0) & (iu < nu_p - 1), (iv >= 0) & (iv < nv - 1)
        out_u += int(np.count_nonzero(~ok_u))
        out_v += int(np.count_nonzero(~ok_v))
        iu_c, iv_c = np.clip(iu, 0, nu_p - 2), np.clip(iv, 0, nv - 2)
        val = ((1 - av) * ((1 - au) * q[iv_c, iu_c] + au * q[iv_c, iu_c + 1]) + av * ((1 - au) * q[iv_c + 1, iu_c] + au * q[iv_c + 1, iu_c + 1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            wgt = dbeta[k] * (sid / U) ** 2
        vol += np.where(ok_U & ok_u & ok_v, wgt * val, 0.0)
    if stats is not None:
        stats.update(refused_u=out_u, refused_v=out_v)
    return vol


def ambiguous_voxels(nu, nv, du, dv, u0, v0, sid, sdd, gantry_deg, off_x, off_y, mean, coefficients, delta, dim, spacing, origin=None, tol=1e-3):
    """[nz][ny][nx] mask like fdk_oracle.ambiguous_voxels, at the displaced point: voxels for which some projection puts fu or fv
    within `tol` pixel of an inclusion limit (fu at 0 or nu_p - 1, fv at 0 or nv - 1) with the other coordinate inside its range
    (or as close to it).  There the float32 kernel and this restatement may disagree about whether a whole contribution counts."""
    n = len(gantry_deg)
    off_x = np.broadcast_to(np.asarray(off_x, dtype=np.float64), (n,))
    off_y = np.broadcast_to(np.asarray(off_y, dtype=np.float64), (n,))
    delta = np.asarray(delta, dtype=np.float64).reshape(n, -1)
    pad_l, pad_r = fo.symmetric_padding(nu, du, u0, float(off_x.min()), float(off_x.max()))
    nu_p, u0_p = nu + pad_l + pad_r, u0 - pad_l * du
    out = np.zeros((dim[2], dim[1], dim[0]), dtype=bool)
    for k in range(n):
        Xp, Yp, Zp = _displaced(mean, coefficients, delta[k], dim, spacing, origin)
        fu, fv, U = _detector_point(Xp, Yp, Zp, gantry_deg[k], sid, sdd, off_x[k], off_y[k], u0_p, v0, du, dv)
        u_edge = (np.abs(fu) < tol) | (np.abs(fu - (nu_p - 1)) < tol)
        u_wide = (fu > -tol) & (fu < nu_p - 1 + tol)
        v_edge = (np.abs(fv) < tol) | (np.abs(fv - (nv - 1)) < tol)
        v_wide = (fv > -tol) & (fv < nv - 1 + tol)
        out |= (U > 0) & ((u_edge & v_wide) | (v_edge & u_wide))
    return out


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------
def breathing(n, cycles=4.3):
    """(s [n], ds [n]): a cos^4 breathing curve over the scan (Lujan et al. 1999), scaled to [-1, 1], and its derivative scaled to
    the same range (max |8 cos^3 sin| = 3 sqrt(3) / 2)."""
    ph = np.pi * cycles * np.arange(n, dtype=np.float64) / n
    s = 1.0 - 2.0 * np.cos(ph) ** 4
    ds = 8.0 * np.cos(ph) ** 3 * np.sin(ph) / (1.5 * np.sqrt(3.0))
    return s, ds


def signal_columns(n, k_dims):
    """delta [n][K] of the tests: the breathing curve, its derivative, and their products for K > 2 (all within [-1, 1])."""
    s, ds = breathing(n)
    return np.stack([s, ds, s * s - 0.5, s * ds][:k_dims], axis=1)


def smooth_model(dim, spacing, k_dims, amplitude_mm, seed=3, offset_mm=(0.0, 0.0, 0.0)):
    """(mean [3][nz][ny][nx], coefficients [K][3][nz][ny][nx]) float32: a few low-order sinusoids per component, each field bounded by
    amplitude_mm (plus the constant offset_mm on the mean)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dim
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")

    def field():
        out = np.zeros((3, nz, ny, nx))
        for c in range(3):
            for _ in range(3):
                f = rng.integers(0, 3, size=3)
                ph = rng.uniform(0, 2 * np.pi, size=3)
                out[c] += rng.uniform(-1, 1) * np.cos(np.pi * f[0] * x + ph[0]) * np.cos(np.pi * f[1] * y + ph[1]) * np.cos(np.pi * f[2] * z + ph[2])
            out[c] *= amplitude_mm[c] / max(np.abs(out[c]).max(), 1e-30)
        return out

    mean = field() * 0.5 + np.asarray(offset_mm, dtype=np.float64)[:, None, None, None]
    coefficients = np.stack([field() * (0.5 / k_dims) for _ in range(k_dims)])
    return mean.astype(np.float32), coefficients.astype(np.float32)


def sphere_masks(dim, sp, centre, radius, margin, outer):
    """(interior r < radius - margin, shell radius + margin < r < radius + outer) of the voxel centres."""
    X, Y, Z = fo.volume_axes(dim, sp)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    r = np.sqrt((xx - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (zz - centre[2]) ** 2)
    return r < radius - margin, (r > radius + margin) & (r < radius + outer)
