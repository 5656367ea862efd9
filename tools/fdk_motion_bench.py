"""Time motion-compensated FDK (csrc/fdk.hip: backproject_motion_kernel) beside plain FDK at the reference's size: 894 half-fan
projections of 1024 x 768 pixels (0.388 mm, lateral offset -159.856 mm, start angle 270 degrees) into 464 x 250 x 464 voxels of
1 mm, pad / hann / hannY = 1 as reconstruct_3d passes them; K = 2 and a synthetic smooth model (low-order sinusoids, up to 10 mm) on a
cos^4 breathing curve and its derivative.

One warm-up round, then `--runs` rounds; a round runs plain `fdk` (the yardstick: the column kernel) and `fdk_motion` once each, in
turn, in this process on one card.  Prints the median ms_backproject and ms_filter of both, their ratio, the model's upload time and
the peak device bytes.  Final line: JSON.  Usage: python tools/fdk_motion_bench.py [--n-proj 894] [--runs 5] [--k 2]"""
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


def smooth_model(dim, k_dims, amplitude_mm=10.0, seed=3):
    """(mean [3][nz][ny][nx], coefficients [K][3][nz][ny][nx]) float32: one separable low-order sinusoid per field and component."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dim
    axes = [np.linspace(0.0, 1.0, n, dtype=np.float32) for n in (nz, ny, nx)]
    out = np.empty((k_dims + 1, 3, nz, ny, nx), np.float32)
    for f in range(k_dims + 1):
        for c in range(3):
            freq, ph = rng.integers(1, 3, size=3), rng.uniform(0, 2 * np.pi, size=3)
            z, y, x = (np.cos(np.pi * freq[a] * axes[a] + ph[a]).astype(np.float32) for a in range(3))
            np.multiply(z[:, None, None] * y[None, :, None], x[None, None, :] * np.float32(0.5 * amplitude_mm / (1 if f == 0 else k_dims)), out=out[f, c])
    return out[0], out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-proj", type=int, default=894)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--dimension", default="464,250,464")
    args = ap.parse_args()
    pkg = load_package()
    recon, d = pkg.reconstruction, pkg.defaults.DEFAULTS
    pkg.engine.load_library()
    dim, spacing, k_dims = tuple(int(v) for v in args.dimension.split(",")), (1.0, 1.0, 1.0), args.k
    (nu, nv), pix = d.n_detector_pixels_half_fan, d.detector_pixel_size
    n = args.n_proj
    geo = recon.create_geometry(n)
    t0 = time.perf_counter()
    proj = np.random.default_rng(1).random((n, nv, nu), dtype=np.float32)
    proj += np.float32(2.0)
    mean, coefficients = smooth_model(dim, k_dims)
    motion = recon.MotionModel(mean, coefficients, np.zeros(k_dims), spacing=spacing)
    ph = np.pi * (n / 60.0) * np.arange(n) / n                     # 15 projections / s, 4 s period
    s, ds = 1.0 - 2.0 * np.cos(ph) ** 4, 8.0 * np.cos(ph) ** 3 * np.sin(ph) / (1.5 * np.sqrt(3.0))
    signals = np.stack([s, ds, s * s - 0.5, s * ds][:k_dims], axis=1)
    model_bytes = mean.nbytes + coefficients.nbytes
    print(f"inputs  : {time.perf_counter() - t0:.1f} s; projections {proj.nbytes / 1e9:.2f} GB, model {model_bytes / 1e9:.2f} GB", flush=True)
    common = dict(hann=1.0, hann_y=1.0, pad=1.0)
    results = {"plain": [], "motion": []}
    for r in range(args.runs + 1):  # round 0 warms both shapes up
        for name in results:
            t0 = time.perf_counter()
            if name == "plain":
                vol, rep = recon.fdk(proj, geo, pix, None, dim, spacing, **common)
            else:
                vol, rep = recon.fdk_motion(proj, geo, pix, None, motion, signals, dim, spacing, **common)
            rep["s_wall"] = time.perf_counter() - t0
            if r > 0:
                results[name].append(rep)
            print(f"round {r} {name:7s}: backproject {rep['ms_backproject']:8.1f} ms, filter {rep['ms_filter']:7.1f} ms, wall {rep['s_wall']:.2f} s", flush=True)
            del vol
    med = {name: {k: float(np.median([rep[k] for rep in reps])) for k in reps[0]} for name, reps in results.items()}
    spread = {name: [float(min(rep["ms_backproject"] for rep in reps)), float(max(rep["ms_backproject"] for rep in reps))] for name, reps in results.items()}
    plain, moving = med["plain"], med["motion"]
    print(f"plain   : backproject {plain['ms_backproject']:.1f} ms {spread['plain']}, filter {plain['ms_filter']:.1f} ms", flush=True)
    print(f"motion  : backproject {moving['ms_backproject']:.1f} ms {spread['motion']} = {moving['ms_backproject'] / plain['ms_backproject']:.2f} x plain, "
          f"filter {moving['ms_filter']:.1f} ms, model upload {moving['ms_upload_model']:.0f} ms, peak device memory {moving['peak_device_bytes'] / 2**30:.2f} GiB", flush=True)
    print(json.dumps(dict(n_proj=n, detector=[nu, nv], dimension=list(dim), k=k_dims, runs=args.runs, model_bytes=model_bytes, median=med,
                          ms_backproject_min_max=spread, ratio=moving["ms_backproject"] / plain["ms_backproject"])))


if __name__ == "__main__":
    main()
