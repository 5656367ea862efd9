"""Time a FAST launch that tallies squared weights (mcgpu_launch_projection_w2) against the plain launch of the same histories, on a
benchmark workload (workloads.build_workload: catphan, cirs, thorax), 1e8 histories per launch by default.

Three kinds of launch alternate in one process after a warm-up round, each timed by the HIP events the engine records around the
launch (track kernel + folds, mcgpu_last_kernel_ms):

  plain            no w2: the default route of the workload (staged by the exterior rule, or the direct atomics)
  w2               with w2, default route: staged wherever the detector has a plan, the fold's squares pass over the same records
  w2_direct        with w2 and MCGPU_TALLY_STAGE=0: two 64-bit atomics per hit

Per kind: median and [min, max] over the rounds; the last line is one JSON object.  The w2 of the two w2 routes and the images of all
three are compared word for word at the end (a mismatch is an error, not a figure).
Usage: python tools/variance_cost.py [--workload catphan] [--histories 1e8] [--rounds 5] [--workdir DIR]"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="catphan")
    ap.add_argument("--histories", type=float, default=1e8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workdir", default=None, help="inputs are kept here and reused (default: the workload's scratch directory)")
    args = ap.parse_args()
    import torch  # before the engine library brings up HIP
    if not torch.cuda.is_available():
        raise SystemExit("variance_cost.py needs a GPU (the engine has no CPU fallback)")
    pkg = load_package()
    eng = pkg.engine
    eng.load_library()
    n = int(args.histories)
    workdir = Path(args.workdir) if args.workdir else pkg.workloads.workload_dir(args.workload)
    inp = workdir / "input.in"
    if not (inp.exists() and (workdir / "geometry.voxbin").exists()):
        workdir.mkdir(parents=True, exist_ok=True)
        pkg.workloads.build_workload(workdir, args.workload, n, 894, eng)
    for k in ("MCGPU_TALLY_STAGE", "MCGPU_TALLY_STAGE_CAP", "MCGPU_TALLY_STAGE_MAX_HISTORIES"):
        os.environ.pop(k, None)
    kinds = {"plain": (False, None), "w2": (True, None), "w2_direct": (True, "0")}
    ms = {k: [] for k in kinds}
    tallies = {}
    with eng.create(inp, device=0) as ctx:
        img = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        w2 = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        staged_by_default = ctx.geti("tally_stage_bins") > 0
        for rnd in range(args.rounds + 1):  # round 0 warms every kind up
            for kind, (with_w2, stage) in kinds.items():
                if stage is None:
                    os.environ.pop("MCGPU_TALLY_STAGE", None)
                else:
                    os.environ["MCGPU_TALLY_STAGE"] = stage
                ctx.reload_env_knobs()
                img.zero_()
                w2.zero_()
                torch.cuda.synchronize()
                ctx.launch(rnd % ctx.num_projections, img.data_ptr(), n, mode="fast", w2_dev_ptr=w2.data_ptr() if with_w2 else 0)
                t = ctx.last_kernel_ms()
                if rnd > 0:
                    ms[kind].append(t)
                if rnd == args.rounds:
                    tallies[kind] = (ctx.download_image(img.data_ptr()), ctx.download_image(w2.data_ptr()))
        os.environ.pop("MCGPU_TALLY_STAGE", None)
    assert np.array_equal(tallies["plain"][0], tallies["w2"][0]) and np.array_equal(tallies["plain"][0], tallies["w2_direct"][0]), "images differ"
    assert np.array_equal(tallies["w2"][1], tallies["w2_direct"][1]) and int(tallies["w2"][1].sum()) > 0, "w2 differs between the routes"
    out = {"workload": args.workload, "histories": n, "rounds": args.rounds, "plain_is_staged": staged_by_default,
           "detected_hits_words": int(np.count_nonzero(tallies["plain"][0]))}
    for kind, v in ms.items():
        out[kind] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
        print(f"{args.workload:8s} {kind:10s} median {np.median(v):8.3f} ms  [{np.min(v):.3f}, {np.max(v):.3f}]  runs {np.round(v, 3).tolist()}")
    for kind in ("w2", "w2_direct"):
        out[kind]["over_plain"] = out[kind]["median_ms"] / out["plain"]["median_ms"] - 1.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
