"""Time motion-aware 4-D ROOSTER (csrc/rooster4d.hip: warp4_kernel; reconstruction.rooster4d_motion) at the
reference's size: tools/rooster4d_bench.py's scan (894 half-fan projections of 1024 x 768 pixels, 10 frames of 464 x 250 x 464
voxels of 1 mm, niter 10, cgiter 4, tviter 10, gamma_time 0.0002, gamma_space 0.00007) and phantom, with a synthetic K = 2 pair of
motion models on the reconstruction grid.

The phantom's sphere moves by 10 cos(2 pi f / frames) mm along Z; the projections' signals are (cos, sin)(2 pi phase).  The model
to the reference moves a smooth bump (radius about 60 mm around the isocentre) by +10 mm along Z per unit of signal 0 and by +2 mm
along X per unit of signal 1; the model from the reference is its negative (an inverse to first order).  Prints the per-stage ms,
the warps' share of the total, the bytes the warp step moves against the achievable HBM rate (6.3 TB/s) and the peak device
memory.  --plain also runs rooster4d on the same projections (the same process, after the motion-aware run).  Final line: JSON.
Usage: python tools/rooster4d_motion_bench.py [--n-proj 894] [--frames 10] [--niter 10] [--gamma-time 0.0002] [--plain]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from __graft_entry__ import load_package  # noqa: E402
from rooster4d_bench import HBM_TBPS, phantom  # noqa: E402

K = 2


def models(recon, dim, spacing):
    """(to_reference, from_reference): MotionModels of K = 2 on the grid."""
    nx, ny, nz = dim
    X = ((np.arange(nx) - (nx - 1) / 2) * spacing[0]).astype(np.float32)
    Y = ((np.arange(ny) - (ny - 1) / 2) * spacing[1]).astype(np.float32)
    Z = ((np.arange(nz) - (nz - 1) / 2) * spacing[2]).astype(np.float32)
    bump = np.exp(-(Z[:, None, None] ** 2 + Y[None, :, None] ** 2 + X[None, None, :] ** 2) / np.float32(2 * 60.0 ** 2)).astype(np.float32)
    mean = np.zeros((3, nz, ny, nx), np.float32)
    coef = np.zeros((K, 3, nz, ny, nx), np.float32)
    coef[0, 2] = 10.0 * bump
    coef[1, 0] = 2.0 * bump
    return recon.MotionModel(mean, coef, np.zeros(K), spacing=spacing), recon.MotionModel(mean, -coef, np.zeros(K), spacing=spacing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-proj", type=int, default=894)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--gamma-time", type=float, default=0.0002)
    ap.add_argument("--plain", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    recon, d = pkg.reconstruction, pkg.defaults.DEFAULTS
    pkg.engine.load_library()
    dim, spacing = (464, 250, 464), (1.0, 1.0, 1.0)
    (nu, nv), pix = d.n_detector_pixels_half_fan, d.detector_pixel_size
    params = dict(niter=args.niter, cgiter=4, tviter=10, gamma_time=args.gamma_time, gamma_space=0.00007)
    geo = recon.create_geometry(args.n_proj)
    amp = pkg.respiratory.RespiratorySignal.create_sin4(total_seconds=args.n_proj / 15.0, period=4.0, sampling_frequency=15.0).signal
    ph = np.hstack(pkg.phase.calculate_phase(amp)).astype(np.float64)
    ph = (ph - ph.min()) / (ph.max() - ph.min())
    signals = np.stack([np.cos(2 * np.pi * ph), np.sin(2 * np.pi * ph)], axis=1)
    t0 = time.perf_counter()
    x4 = phantom(dim, spacing, args.frames)
    to_reference, from_reference = models(recon, dim, spacing)
    print(f"phantom and models : {time.perf_counter() - t0:.1f} s", flush=True)
    proj, _ = recon.rooster4d_stage("forward", x4, geo, (nu, nv), pix, None, ph, dim, spacing, frames=args.frames)
    del x4
    t0 = time.perf_counter()
    vol, rep = recon.rooster4d_motion(proj, geo, pix, None, ph, to_reference, from_reference, signals, dim, spacing, frames=args.frames, **params)
    wall = time.perf_counter() - t0
    nvox = dim[0] * dim[1] * dim[2]
    vec = 4.0 * nvox * args.frames
    model = 4.0 * nvox * 3 * (K + 1)
    # per main iteration: W reads x and the model and writes y twice; the subtraction reads two vectors and writes one; U reads c and the
    # model and reads and writes x (the 8 gathers of a voxel counted once: neighbours share them through the cache)
    warp_bytes = params["niter"] * ((3 * vec + model) + 3 * vec + (3 * vec + model))
    tb = warp_bytes / (rep["ms_warp"] * 1e-3) / 1e12
    res = dict(n_proj=args.n_proj, detector=[nu, nv], dimension=list(dim), frames=args.frames, n_signal_dims=K, params=params, s_wall=wall,
               **{k: v for k, v in rep.items() if k not in ("residuals", "frame_signals")}, warp_share_of_total=rep["ms_warp"] / rep["ms_total"],
               warp_gb_moved=warp_bytes / 1e9, hbm_warp_tbps=tb, residual_first_last=[float(rep["residuals"][0, 0]), float(rep["residuals"][-1, -1])],
               volume_mean=float(vol.mean()), volume_max=float(vol.max()))
    for key in ("ms_forward", "ms_back", "ms_cg_vectors", "ms_tv_space", "ms_tv_time", "ms_warp", "ms_upload", "ms_upload_model"):
        print(f"{key:16s}: {rep[key]:.0f} ms", flush=True)
    print(f"warp step : {rep['ms_warp']:.0f} ms = {100 * res['warp_share_of_total']:.2f} % of {rep['ms_total'] / 1e3:.1f} s; {warp_bytes / 1e9:.1f} GB moved, "
          f"{tb:.2f} TB/s = {100 * tb / HBM_TBPS:.0f} % of {HBM_TBPS} TB/s; peak device memory {rep['peak_device_bytes'] / 2**30:.2f} GiB, wall {wall:.1f} s", flush=True)
    if args.plain:
        del vol
        t0 = time.perf_counter()
        _, plain = recon.rooster4d(proj, geo, pix, None, ph, dim, spacing, frames=args.frames, **params)
        res["plain"] = dict(s_wall=time.perf_counter() - t0, **{k: v for k, v in plain.items() if k != "residuals"})
        print(f"plain rooster4d : total {plain['ms_total'] / 1e3:.1f} s, tv time {plain['ms_tv_time']:.0f} ms, peak device memory "
              f"{plain['peak_device_bytes'] / 2**30:.2f} GiB", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
