"""Time the ray-traced primary (csrc/primary_project.hip) on bench.py's own workloads at the reference's size -- the Catphan604 in 512^3
voxels of 1 mm and the CIRS phantom, 1848 x 768 pixel detector cropped to the 1024 half-fan columns -- next to the FAST launch of the same
projection, and measure what the analytic plane replaces: the history count at which the Monte Carlo unscattered plane's median
relative sigma (per-pixel variance) falls to 1 %.

Per workload, for `--projections` projections spread over the trajectory:
  primary   : kernel ms per projection at 1 x 1 and 2 x 2 sub-points (HIP events around the launches, mcgpu_primary_report.ms_kernel),
              after one warm-up call; the host tables' time beside it
  fast      : kernel ms of the FAST launch of `--histories` histories of the same projections (mcgpu_run_projection's kernel time)
  sigma     : median over the lit pixels of sqrt(variance) / value of the unscattered plane of a second launch that also tallies the
              squared weights, and N(1 %) = histories x
              (median / 0.01)^2
Prints one line per measurement and a final JSON line.  Usage: python tools/primary_bench.py [--workloads catphan cirs]
[--projections 4] [--histories 1e8] [--n-vox 512]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["catphan", "cirs"])
    ap.add_argument("--projections", type=int, default=4)
    ap.add_argument("--histories", type=float, default=1e8)
    ap.add_argument("--n-vox", type=int, default=512)
    ap.add_argument("--n-proj", type=int, default=894)
    args = ap.parse_args()
    pkg = load_package()
    eng, wl, d = pkg.engine, pkg.workloads, pkg.defaults.DEFAULTS
    eng.load_library()
    crop = d.n_detector_pixels_half_fan[0]
    n_hist = int(args.histories)
    result = {"histories": n_hist, "crop_nx": crop}
    for workload in args.workloads:
        workdir = wl.workload_dir(workload, args.n_vox, args.n_proj)
        inp = workdir / "input.in"
        if not inp.exists():
            t0 = time.perf_counter()
            inp = wl.build_workload(workdir, workload, n_hist, args.n_proj, engine=eng, n_vox=args.n_vox)
            print(f"{workload}: inputs built in {time.perf_counter() - t0:.1f} s", flush=True)
        with eng.create(str(inp), device=0) as ctx:
            nz, nx = ctx.detector_shape
            which = [int(p) for p in np.linspace(0, ctx.num_projections, args.projections, endpoint=False)]
            row = {"detector": [nx, nz], "volume_kind": ctx.geti("volume_kind"), "voxels": [ctx.geti(f"num_voxels_{a}") for a in "xyz"], "projections": which}
            ctx.primary_projection(which[0], crop_nx=crop)                      # code object, allocator
            for ss in ((1, 1), (2, 2)):
                ms, tables = [], []
                for p in which:
                    plane, rep = ctx.primary_projection(p, subsamples=ss, crop_nx=crop)
                    ms.append(rep["ms_kernel"])
                    tables.append(rep["ms_tables"])
                row[f"primary_{ss[0]}x{ss[1]}"] = dict(ms_kernel=float(np.mean(ms)), ms_kernel_min=float(np.min(ms)), ms_kernel_max=float(np.max(ms)),
                                                       ms_tables=float(np.mean(tables)), n_materials=rep["n_materials"], n_energy_points=rep["n_energy_points"])
                print(f"{workload}: primary {ss[0]} x {ss[1]}: {np.mean(ms):.2f} ms per projection (min {np.min(ms):.2f}, max {np.max(ms):.2f}), "
                      f"tables {np.mean(tables):.2f} ms, {rep['n_materials']} materials, {rep['n_energy_points']} energy points", flush=True)
            ctx.run_projection(which[0], 1_000_000)                              # warm-up of the tracking kernel
            fast_ms, rel = [], []
            for p in which:
                fast_ms.append(1e3 * ctx.run_projection(p, n_hist, mode="fast")[1])
                image, w2, _, done = ctx.run_projection_with_variance(p, n_hist, mode="fast")
                w = image[0, :, :crop].astype(np.float64)
                var = np.maximum(w2[0, :, :crop].astype(np.float64) * 1048576.0 - w * w / done, 0.0)
                lit = w > 0
                rel.append(float(np.median(np.sqrt(var[lit]) / w[lit])))
            med = float(np.mean(rel))
            row["fast"] = dict(ms_kernel=float(np.mean(fast_ms)), median_relative_sigma=med, histories_for_one_percent=n_hist * (med / 0.01) ** 2)
            print(f"{workload}: FAST launch {np.mean(fast_ms):.1f} ms per projection of {n_hist:.1e} histories; unscattered plane: median "
                  f"relative sigma {med:.4f} -> {row['fast']['histories_for_one_percent']:.2e} histories for 1 %", flush=True)
        result[workload] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
