#!/usr/bin/env python3
"""Write gpurun_out/fast_pin.json (GPU): SHA-256 of the FAST kernel's integer tallies on small cases.  Copy the file to
tests/golden/fast_pin.json after a DELIBERATE change of the FAST arithmetic or random-number use; the test
test_fast_kernel_tallies_are_pinned then fails whenever a build changes a single tally word by accident (compiler, flags)."""
import hashlib, json, sys
from pathlib import Path
import tempfile
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import cases
PIN_CASES = [("catphan64_ct", 1, 600_000, 11), ("tissue22", 0, 400_000, 12), ("cirs76", 2, 400_000, 13), ("air", 0, 200_000, 14)]


def compute(mode="fast"):
    eng = cases.pkg.engine
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, p, n, seed in PIN_CASES:
            with eng.create(cases.build_case(name, Path(tmp) / name), device=0) as ctx:
                img, _, done = ctx.run_projection(p, n, mode=mode, seed=seed)
                out[name] = {"projection": p, "histories": n, "seed": seed, "sum": int(img.sum()), "sha256": hashlib.sha256(img.tobytes()).hexdigest()}
    return out


STATS_CASES = ("catphan64_ct", "tissue22")
# sums over histories of events that each history's own stream decides: the same under every schedule
SCHEDULE_FREE = ("lanes_taking_a_step", "flying_lanes", "compton_angle_lanes", "compton_shell_lanes", "compton_done_lanes", "voxel_load_lanes")


def compute_stats():
    """The diagnostic build (MCGPU_AMD_LIB = libmcgpu_amd_stats.so, set before this process imports the engine) on STATS_CASES under both
    schedulers: {case: {scheduler: {"sum", "sha256", "stats": scheduler_stats()}}}.  `--stats` prints it; `--stats-pin` prints what
    tests/golden/fast_stats_pin.json holds, the SCHEDULE_FREE counters per case -- written from the build BEFORE a change of the kernel."""
    import os
    eng = cases.pkg.engine
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, p, n, seed in PIN_CASES:
            if name not in STATS_CASES:
                continue
            out[name] = {}
            for sched in (0, 1):
                os.environ["MCGPU_FAST_SCHED"] = str(sched)  # read when the model is uploaded
                with eng.create(cases.build_case(name, Path(tmp) / f"{name}_{sched}"), device=0) as ctx:
                    assert ctx.geti("fast_scheduler") == sched
                    img, _, done = ctx.run_projection(p, n, mode="stats", seed=seed)
                    out[name][str(sched)] = {"sum": int(img.sum()), "sha256": hashlib.sha256(img.tobytes()).hexdigest(), "stats": ctx.scheduler_stats()}
    return out


if __name__ == "__main__":
    if sys.argv[1:] in (["--stats"], ["--stats-pin"]):
        got = compute_stats()
        if sys.argv[1] == "--stats-pin":
            for name, runs in got.items():
                assert all(runs["0"]["stats"][k] == runs["1"]["stats"][k] for k in SCHEDULE_FREE), (name, runs)
            got = {name: {k: runs["0"]["stats"][k] for k in SCHEDULE_FREE} for name, runs in got.items()}
        print(json.dumps(got))
        sys.exit(0)
    (ROOT / "gpurun_out").mkdir(exist_ok=True)
    for mode in ("fast", "fast64"):
        (ROOT / "gpurun_out" / f"{mode}_pin.json").write_text(json.dumps(compute(mode), indent=1))
        print(mode, json.dumps(compute(mode), indent=1))
