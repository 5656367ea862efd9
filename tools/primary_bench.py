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
  noise     : `--noise-rounds R` (default 0: off) rounds of primary_scan, primary_moments_scan and primary_noisy_scan of the same
              projections at 1 x 1 sub-points, alternated call by call (and, with `--parent-lib PATH`, the primary_scan of another build
              of the library -- the parent commit's -- on a context of its own in the same process, alternated with them): kernel ms per
              projection of each, min / median / max over the rounds, and the sampler's ms (`profiles/primary_ab.md`)
Prints one line per measurement and a final JSON line.  Usage: python tools/primary_bench.py [--workloads catphan cirs]
[--projections 4] [--histories 1e8] [--n-vox 512] [--noise-rounds 5] [--parent-lib build/ab/parent.so] [--skip-fast]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402


class OtherBuild:
    """primary_scan of another build of the library (one that may lack the newer entry points), on a context of its own."""

    def __init__(self, eng, path, input_path, device=0):
        self.eng, self.lib = eng, C.CDLL(str(path))
        self.lib.mcgpu_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.mcgpu_destroy.argtypes = [C.c_void_p]
        self.lib.mcgpu_destroy.restype = None
        self.lib.mcgpu_primary_project.argtypes = [C.c_void_p, C.POINTER(eng.PrimaryOptions), C.c_void_p, C.POINTER(eng.PrimaryReport)]
        self.h = C.c_void_p()
        if self.lib.mcgpu_create(str(input_path).encode(), device, C.byref(self.h)) != 0:
            raise RuntimeError(f"{path}: mcgpu_create failed")

    def primary_ms(self, p, shape, crop):
        o = self.eng.PrimaryOptions(C.sizeof(self.eng.PrimaryOptions), int(p), 1, 1, 1, 2, int(crop))
        r = self.eng.PrimaryReport(C.sizeof(self.eng.PrimaryReport))
        out = np.zeros(shape, dtype=np.float32)
        if self.lib.mcgpu_primary_project(self.h, C.byref(o), out.ctypes.data, C.byref(r)) != 0:
            raise RuntimeError("mcgpu_primary_project of the other build failed")
        return r.ms_kernel, out

    def close(self):
        self.lib.mcgpu_destroy(self.h)


def noise_rounds(eng, ctx, inp, which, crop, rounds, parent_lib, histories):
    """Kernel ms per projection of primary_scan, primary_moments_scan and primary_noisy_scan (and the other build's primary_scan),
    alternated call by call; every call is one projection."""
    other = OtherBuild(eng, parent_lib, inp) if parent_lib else None
    ms = {"primary": [], "moments": [], "noisy": [], "noisy_sample": []}
    if other:
        ms["parent_primary"] = []
    try:
        for r in range(rounds + 1):                                             # round 0 warms every code object up and is dropped
            acc = {k: [] for k in ms}
            for p in which:
                if other:
                    t, theirs = other.primary_ms(p, (ctx.detector_shape[0], crop), crop)
                    acc["parent_primary"].append(t)
                plane, rep = ctx.primary_projection(p, crop_nx=crop)
                acc["primary"].append(rep["ms_kernel"])
                if other and r == 0:
                    assert theirs.tobytes() == plane.tobytes(), "the two builds disagree on primary_projection"
                acc["moments"].append(ctx.primary_moments(p, crop_nx=crop)[1]["ms_kernel"])
                rep = ctx.primary_noisy_projection(p, histories, seed=1 + r, crop_nx=crop)[1]
                acc["noisy"].append(rep["ms_kernel"])
                acc["noisy_sample"].append(rep["ms_sample"])
            if r:
                for k in ms:
                    ms[k].append(float(np.mean(acc[k])))
    finally:
        if other:
            other.close()
    return {k: dict(min=float(np.min(v)), median=float(np.median(v)), max=float(np.max(v)), rounds=v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["catphan", "cirs"])
    ap.add_argument("--projections", type=int, default=4)
    ap.add_argument("--histories", type=float, default=1e8)
    ap.add_argument("--n-vox", type=int, default=512)
    ap.add_argument("--n-proj", type=int, default=894)
    ap.add_argument("--noise-rounds", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-fast", action="store_true", help="leave out the FAST launches and the sigma measurement")
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
            if args.noise_rounds > 0:
                row["noise"] = noise_rounds(eng, ctx, inp, which, crop, args.noise_rounds, args.parent_lib, float(n_hist))
                for k, v in row["noise"].items():
                    print(f"{workload}: {k}: {v['median']:.3f} ms per projection (min {v['min']:.3f}, max {v['max']:.3f} over {args.noise_rounds} rounds)",
                          flush=True)
            if args.skip_fast:
                result[workload] = row
                continue
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
