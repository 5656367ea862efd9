#!/usr/bin/env python3
"""Dev measurement (GPU): the shape of the END of a FAST launch.  One launch of the diagnostic build (libmcgpu_amd_stats.so, mode
"stats") leaves the first and last constant-rate clock (100 MHz) of every wave in the wave trace; this prints how long before the
last wave the others ended (p10, p50, p90, max of `last end - own end`, in microseconds), per wave and per workgroup, and the
launch's span.  The diagnostic build is slower than the product: the figures describe the shape of the end, not a headline time.
The last clock is taken behind the kernel's final barrier, which only a staged launch (or one with a material dose) has, so the
per-wave figures want the direct tally (the default here; --staged keeps the engine's own choice).
Usage: python tools/launch_end.py [workload] [--histories N] [--projection P] [--staged] [--repeat K]"""
import argparse, ctypes as C, json, os, sys, tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="catphan")
ap.add_argument("--histories", type=float, default=1e8)
ap.add_argument("--projection", type=int, default=0)
ap.add_argument("--staged", action="store_true")
ap.add_argument("--repeat", type=int, default=3)
args = ap.parse_args()
os.environ.setdefault("MCGPU_AMD_LIB", str(ROOT / "4d-cbct-mc_amd" / "libmcgpu_amd_stats.so"))  # the diagnostic build (stats mode)
if not args.staged:
    os.environ["MCGPU_TALLY_STAGE"] = "0"
import numpy as np  # noqa: E402
import bench, cases  # noqa: E402

eng = cases.pkg.engine
NS, NT, WAVES_PER_WG = 32, 32 + 3 * 16384, 16  # device_model.hpp: kNumStats, kWaveTrace, kPoolBlockThreads / 64
wd = Path(tempfile.gettempdir()) / f"mcgpu_bench_{args.workload}_512_894"
if not (wd / "input.in").exists():
    wd.mkdir(parents=True, exist_ok=True)
    bench.build_workload(wd, args.workload, 100_000_000, 894, eng)
n = int(args.histories)


def quantiles(lag_us):
    return {k: round(float(np.percentile(lag_us, q)), 1) for k, q in (("p10", 10), ("p50", 50), ("p90", 90), ("max", 100))}


with eng.create(str(wd / "input.in"), device=0) as ctx:
    out = (C.c_ulonglong * NT)()
    ctx.run_projection(args.projection, n, mode="stats", seed=42)  # one-off costs
    for rep in range(args.repeat):
        eng._check(ctx.lib.mcgpu_scheduler_stats_ex(ctx.h, out, NT, 1))
        ctx.run_projection(args.projection, n, mode="stats", seed=42)
        eng._check(ctx.lib.mcgpu_scheduler_stats_ex(ctx.h, out, NT, 0))
        t = np.frombuffer(out, dtype=np.uint64)[NS:].reshape(-1, 3)
        t = t[t[:, 1] != 0]
        first, last = t[:, 1].astype(np.int64), t[:, 2].astype(np.int64)
        lag = (last.max() - last) / 100.0  # 100 MHz ticks -> us
        wg = lag[: len(lag) // WAVES_PER_WG * WAVES_PER_WG].reshape(-1, WAVES_PER_WG)
        print(json.dumps({"workload": args.workload, "histories": n, "staged": bool(args.staged), "run": rep, "waves": int(len(t)),
                          "launch_span_us": round((last.max() - first.min()) / 100.0, 1),
                          "wave_end_before_last_us": quantiles(lag), "mean_us": round(float(lag.mean()), 1),
                          "workgroup_end_before_last_us": quantiles(wg.min(axis=1)),
                          "spread_inside_a_workgroup_us": quantiles(wg.max(axis=1) - wg.min(axis=1))}), flush=True)
