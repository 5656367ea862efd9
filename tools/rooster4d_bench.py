"""Time the 4-D ROOSTER reconstruction (csrc/rooster4d.hip) at the reference's size: 894 half-fan projections of 1024 x 768 pixels
(0.388 mm, lateral offset -159.856 mm, start angle 270 degrees), 10 frames of 464 x 250 x 464 voxels of 1 mm, the reference's
parameters (reconstruction.py: reconstruct_4d -- niter 10, cgiter 4, tviter 10, gamma_time 0.0002, gamma_space 0.00007).

The projections are the Joseph forward projection (mcgpu_rooster4d_stage FORWARD) of a synthetic 4-D phantom: a water cylinder
(radius 120 mm, axis Y) with a sphere of radius 15 mm that moves 20 mm along Z with the phase of a sin^4 breathing curve (period
4 s, 15 projections/s; phase.calculate_phase).  Prints the per-stage ms, the wall time and the peak device memory; for the TV and
CG-vector kernels also bytes moved / time against the achievable HBM rate (6.3 TB/s, a float4 copy on MI355X).  The bytes are
counted from what each kernel reads and writes (neighbour reads of the TV kernels counted once: they hit the cache).  Final line:
JSON.  Usage: python tools/rooster4d_bench.py [--n-proj 894] [--frames 10] [--niter 10]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

HBM_TBPS = 6.3


def phantom(dim, spacing, frames):
    nx, ny, nz = dim
    X = ((np.arange(nx) - (nx - 1) / 2) * spacing[0]).astype(np.float32)
    Y = ((np.arange(ny) - (ny - 1) / 2) * spacing[1]).astype(np.float32)
    Z = ((np.arange(nz) - (nz - 1) / 2) * spacing[2]).astype(np.float32)
    cyl = (Z[:, None] ** 2 + X[None, :] ** 2 <= 120.0 ** 2).astype(np.float32)  # [nz][nx]
    out = np.empty((frames, nz, ny, nx), np.float32)
    for f in range(frames):
        cz = 10.0 * np.cos(2 * np.pi * f / frames)
        sph = ((Z[:, None, None] - cz) ** 2 + Y[None, :, None] ** 2 + X[None, None, :] ** 2) <= 15.0 ** 2
        out[f] = cyl[:, None, :] + 0.5 * sph
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-proj", type=int, default=894)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--niter", type=int, default=10)
    args = ap.parse_args()
    pkg = load_package()
    recon, d = pkg.reconstruction, pkg.defaults.DEFAULTS
    pkg.engine.load_library()
    dim, spacing = (464, 250, 464), (1.0, 1.0, 1.0)
    (nu, nv), pix = d.n_detector_pixels_half_fan, d.detector_pixel_size
    params = dict(niter=args.niter, cgiter=4, tviter=10, gamma_time=0.0002, gamma_space=0.00007)
    geo = recon.create_geometry(args.n_proj)
    amp = pkg.respiratory.RespiratorySignal.create_sin4(total_seconds=args.n_proj / 15.0, period=4.0, sampling_frequency=15.0).signal
    ph = np.hstack(pkg.phase.calculate_phase(amp)).astype(np.float64)
    ph = (ph - ph.min()) / (ph.max() - ph.min())
    t0 = time.perf_counter()
    x4 = phantom(dim, spacing, args.frames)
    print(f"phantom : {time.perf_counter() - t0:.1f} s", flush=True)
    proj, rep_fp = recon.rooster4d_stage("forward", x4, geo, (nu, nv), pix, None, ph, dim, spacing, frames=args.frames)
    del x4
    print(f"fp      : {rep_fp['ms_forward']:.1f} ms for {args.n_proj} projections (one R S)", flush=True)
    t0 = time.perf_counter()
    vol, rep = recon.rooster4d(proj, geo, pix, None, ph, dim, spacing, frames=args.frames, **params)
    wall = time.perf_counter() - t0
    nvox = dim[0] * dim[1] * dim[2]
    vec = 4.0 * nvox * args.frames
    niter, cg, tv = params["niter"], params["cgiter"], params["tviter"]
    # CG vectors: restart 4 (+1 memset of A d in the first iteration), per step dot 2 + update 6 + direction 3, positivity 2
    cg_bytes = vec * (niter * (4 + 11 * cg + 2) + 1)
    tvs_bytes = 4.0 * nvox * niter * args.frames * (3 + 12 * tv + 5)  # memset of the dual, 12 frames per iteration, final u
    tvt_bytes = 2.0 * vec * niter
    applications = 1 + niter * (cg + 1) - 1  # b, then cgiter + 1 per main iteration, the first restart at x = 0 needs none
    res = dict(n_proj=args.n_proj, detector=[nu, nv], dimension=list(dim), frames=args.frames, params=params, s_wall=wall,
               **{k: v for k, v in rep.items() if k != "residuals"}, fp_applications=applications - 1, bp_applications=applications,
               ms_per_forward=rep["ms_forward"] / max(applications - 1, 1), ms_per_back=rep["ms_back"] / applications,
               hbm_cg_vectors_tbps=cg_bytes / (rep["ms_cg_vectors"] * 1e-3) / 1e12, hbm_tv_space_tbps=tvs_bytes / (rep["ms_tv_space"] * 1e-3) / 1e12,
               hbm_tv_time_tbps=tvt_bytes / (rep["ms_tv_time"] * 1e-3) / 1e12, residual_first_last=[float(rep["residuals"][0, 0]), float(rep["residuals"][-1, -1])],
               volume_mean=float(vol.mean()), volume_max=float(vol.max()))
    print(f"forward : {rep['ms_forward']:.0f} ms ({res['ms_per_forward']:.1f} ms x {applications - 1})", flush=True)
    print(f"back    : {rep['ms_back']:.0f} ms ({res['ms_per_back']:.1f} ms x {applications})", flush=True)
    for name, key, b in (("cg vec ", "ms_cg_vectors", cg_bytes), ("tv space", "ms_tv_space", tvs_bytes), ("tv time", "ms_tv_time", tvt_bytes)):
        tb = b / (rep[key] * 1e-3) / 1e12
        print(f"{name} : {rep[key]:.0f} ms, {b / 1e9:.1f} GB moved, {tb:.2f} TB/s = {100 * tb / HBM_TBPS:.0f} % of {HBM_TBPS} TB/s", flush=True)
    print(f"upload  : {rep['ms_upload']:.0f} ms; total {rep['ms_total'] / 1e3:.1f} s, wall {wall:.1f} s, peak device memory "
          f"{rep['peak_device_bytes'] / 2**30:.2f} GiB", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
