"""Time the field inversion (csrc/field_inverse.hip) at the size of a clinical grid, 464 x 464 x 250, on a smooth
synthetic field:

  1. ms per step of `invert_step_kernel` (device events around the chunk of launches, `ms_step` of the report over the iterations) and
     the effective GB/s over the 24 B per voxel of v traffic (three reads, three writes; the taps of u are not counted);
  2. the same loop composed from torch: `torch.nn.functional.grid_sample(u, grid(x + v), mode="bilinear", padding_mode="border",
     align_corners=True)` and v <- v - w (v + sample), timed by events, and the largest difference of the two results;
  3. end to end, `CorrespondenceModel.build_pair` against the two `build_default` sweeps it replaces (inverse=False and inverse=True), on
     --phases phase images of a sphere that follows the breathing amplitude, at the registration's default parameters, with the wall
     time of each part (registrations, inversions, the host's predictions and fits).

Prints the numbers, writes profiles/field_inverse.md (or --out) unless --no-write.  Final line: JSON.
Usage: python tools/field_inverse_bench.py [--shape 464 464 250] [--iterations 40] [--repeats 5] [--phases 5] [--skip-pair]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402  -- before the engine brings up HIP

from __graft_entry__ import load_package  # noqa: E402


def smooth_field(shape, amplitude=4.0):
    """[3, x, y, z] float32: products of one sine period per axis, `amplitude` voxels, slopes of at most 2 pi amplitude / n."""
    g = [np.arange(n, dtype=np.float32) / np.float32(max(n - 1, 1)) for n in shape]
    s = [np.sin(2 * np.pi * a).astype(np.float32) for a in g]
    c = [np.cos(2 * np.pi * a).astype(np.float32) for a in g]
    u = np.empty((3,) + tuple(shape), dtype=np.float32)
    u[0] = amplitude * s[0][:, None, None] * c[1][None, :, None] * c[2][None, None, :]
    u[1] = -0.5 * amplitude * c[0][:, None, None] * s[1][None, :, None] * c[2][None, None, :]
    u[2] = 0.75 * amplitude * c[0][:, None, None] * c[1][None, :, None] * s[2][None, None, :]
    return u


def torch_loop(u, iterations, relaxation):
    """The rule composed from torch operations on the device: -> (v [3, x, y, z], ms per step)."""
    dev = torch.device("cuda:0")
    shape = u.shape[1:]
    ut = torch.from_numpy(u).to(dev)[None]                                    # [1, 3, D, H, W]
    axes = [torch.arange(n, device=dev, dtype=torch.float32) for n in shape]
    base = torch.stack(torch.meshgrid(*axes, indexing="ij"))                  # [3, D, H, W]
    scale = torch.tensor([2.0 / max(n - 1, 1) for n in shape], device=dev, dtype=torch.float32)[:, None, None, None]

    def run(steps):
        v = torch.zeros_like(base)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            grid = ((base + v) * scale - 1.0).flip(0).permute(1, 2, 3, 0)[None]  # the last axis is (W, H, D)
            sampled = torch.nn.functional.grid_sample(ut, grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
            v = v - relaxation * (v + sampled)
        e1.record()
        torch.cuda.synchronize()
        return v, e0.elapsed_time(e1) / max(steps, 1)

    run(2)  # warm-up
    v, ms = run(iterations)
    return v.cpu().numpy(), ms


def phase_images(shape, amplitudes, travel):
    """A sphere with a logistic edge at z = centre + travel (0.5 - a), radius a quarter of the shortest axis."""
    g = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in shape), indexing="ij", sparse=True)
    radius = 0.25 * min(shape)
    out = []
    for a in amplitudes:
        centre = (0.5 * (shape[0] - 1), 0.5 * (shape[1] - 1), 0.5 * (shape[2] - 1) + travel * (0.5 - a))
        r = np.sqrt((g[0] - centre[0]) ** 2 + (g[1] - centre[1]) ** 2 + (g[2] - centre[2]) ** 2)
        out.append((1.0 / (1.0 + np.exp(np.clip((r - radius) / 2.0, -30, 30)))).astype(np.float32))
    return np.stack(out)


class Clock:
    """Wall seconds spent inside the wrapped functions, by name."""
    def __init__(self):
        self.seconds = {}

    def wrap(self, name, fn):
        def timed(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return fn(*args, **kwargs)
            finally:
                self.seconds[name] = self.seconds.get(name, 0.0) + time.perf_counter() - t0
        return timed


def time_pair(pkg, shape, phases, travel):
    """-> dict: wall seconds of build_pair and of the two build_default sweeps, and of their parts."""
    reg, Model = pkg.registration, pkg.correspondence.CorrespondenceModel
    amplitudes = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(phases) / phases)
    rates = np.gradient(amplitudes)
    signals = np.stack([amplitudes, rates], axis=1)
    images = phase_images(shape, amplitudes, travel)
    reference_phase = int(np.argmax(amplitudes))
    plain = dict(register=reg.register, invert_field=reg.invert_field, fit=Model.fit, predict=Model.predict_field32)
    out = {}
    try:
        for name in ("build_pair", "two_build_default"):
            clock = Clock()
            reg.register, reg.invert_field = clock.wrap("register", plain["register"]), clock.wrap("invert", plain["invert_field"])
            Model.fit, Model.predict_field32 = clock.wrap("fit", plain["fit"]), clock.wrap("predict", plain["predict"])
            t0 = time.perf_counter()
            if name == "build_pair":
                a, b = Model.build_pair(images, signals=signals, reference_phase=reference_phase)
                out["inversion_residual_max"] = max(r["residual_max_after"] for r in b.inversion_reports)
                out["inversion_ms_step"] = sum(r["ms_step"] for r in b.inversion_reports)
            else:
                a = Model.build_default(images, signals=signals, reference_phase=reference_phase)
                b = Model.build_default(images, signals=signals, reference_phase=reference_phase, inverse=True)
            out[name + "_s"] = time.perf_counter() - t0
            out[name + "_parts_s"] = dict(clock.seconds)
            Model.fit, Model.predict_field32 = plain["fit"], plain["predict"]
            out[name + "_pair_rms"] = [a.pair_residual(b, s)["rms"] for s in signals]
            del a, b
    finally:
        reg.register, reg.invert_field, Model.fit, Model.predict_field32 = plain["register"], plain["invert_field"], plain["fit"], plain["predict"]
    out.update(phases=phases, reference_phase=reference_phase, travel_voxels=travel)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(464, 464, 250))
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--relaxation", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--phases", type=int, default=5)
    ap.add_argument("--travel", type=float, default=8.0, help="voxels the sphere moves between the end states")
    ap.add_argument("--skip-pair", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "field_inverse.md")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("field_inverse_bench.py needs the GPU: there is nothing to time without it")
    pkg = load_package()
    reg = pkg.registration
    shape, k, w = tuple(args.shape), args.iterations, args.relaxation
    n = int(np.prod(shape))
    u = smooth_field(shape)
    res = dict(shape=shape, voxels=n, iterations=k, relaxation=w, repeats=args.repeats, device=torch.cuda.get_device_name(0))

    step_ms, reduce_ms, total_ms, v, report = [], [], [], None, None
    for i in range(1 + args.repeats):  # the first call warms up
        v, report = reg.invert_field(u, iterations=k, relaxation=w)
        if i:
            step_ms.append(report["ms_step"] / k)
            reduce_ms.append(report["ms_reduce"] / 2)
            total_ms.append(report["ms_total"])
    step = statistics.median(step_ms)
    res.update(step_ms_median=step, step_ms_min=min(step_ms), step_ms_max=max(step_ms), step_gb_per_s=24.0 * n / (step * 1e-3) / 1e9,
               residual_ms_median=statistics.median(reduce_ms), call_ms_median=statistics.median(total_ms), residual_max_before=report["residual_max_before"],
               residual_max_after=report["residual_max_after"], peak_device_bytes=report["peak_device_bytes"])
    print(f"step     : {step:.3f} ms (min {min(step_ms):.3f}, max {max(step_ms):.3f}), {res['step_gb_per_s']:.0f} GB/s over 24 B per voxel", flush=True)
    print(f"residual : {res['residual_ms_median']:.3f} ms a pass; the whole call with its copies {res['call_ms_median']:.0f} ms; residual max "
          f"{report['residual_max_before']:.3g} -> {report['residual_max_after']:.3g}", flush=True)
    if not args.skip_torch:
        vt, torch_ms = torch_loop(u, k, w)
        res.update(torch_step_ms=torch_ms, torch_over_kernel=torch_ms / step, torch_max_abs_difference=float(np.abs(vt - v).max()))
        print(f"torch    : {torch_ms:.3f} ms a step, {torch_ms / step:.1f} x the kernel; results differ by at most {res['torch_max_abs_difference']:.3g}", flush=True)
        del vt
        torch.cuda.empty_cache()
    del u, v
    if not args.skip_pair:
        res["pair"] = time_pair(pkg, shape, args.phases, args.travel)
        p = res["pair"]
        print(f"pair     : build_pair {p['build_pair_s']:.1f} s {p['build_pair_parts_s']}; two build_default {p['two_build_default_s']:.1f} s "
              f"{p['two_build_default_parts_s']}", flush=True)
    if not args.no_write:
        args.out.write_text(markdown(res, args))
        print(f"wrote {args.out}", flush=True)
    print(json.dumps(res))


def markdown(res, args):
    shape = " x ".join(map(str, res["shape"]))
    text = ("# Field inversion: the step kernel, the torch composition and build_pair end to end\n\n"
            f"`python tools/field_inverse_bench.py --shape {' '.join(map(str, res['shape']))} --iterations {res['iterations']} --relaxation {res['relaxation']} "
            f"--repeats {res['repeats']} --phases {args.phases}` on {res['device']}; a smooth synthetic field (products of one sine period per axis, up to 4 voxels) on "
            f"{shape} = {res['voxels'] / 1e6:.1f} M voxels.  Kernel times come from device events around the chunk of {res['iterations']} launches (`ms_step` of the report), "
            f"medians over {res['repeats']} calls after one warm-up call (min .. max); the torch loop is timed by events over {res['iterations']} steps after 2 warm-up steps.\n\n"
            "| what | ms per step | GB/s over 24 B per voxel |\n|---|---|---|\n"
            f"| `invert_step_kernel` | {res['step_ms_median']:.3f} ({res['step_ms_min']:.3f} .. {res['step_ms_max']:.3f}) | {res['step_gb_per_s']:.0f} |\n")
    if "torch_step_ms" in res:
        text += (f"| torch: `grid_sample(align_corners=True, padding_mode=\"border\")` + the update | {res['torch_step_ms']:.3f} | "
                 f"{24.0 * res['voxels'] / (res['torch_step_ms'] * 1e-3) / 1e9:.0f} |\n\n"
                 f"The composition takes {res['torch_over_kernel']:.1f} x the kernel's time; the two results differ by at most {res['torch_max_abs_difference']:.3g} voxel "
                 f"after {res['iterations']} steps.\n")
    floor_ms = 36.0 * res["voxels"] / 6.3e12 * 1e3
    text += (f"\nThe GB/s figure counts the three reads and three writes of v only; the 24 taps of u per voxel are served by the caches where v is smooth and are not counted.  "
             f"At least 36 B per voxel must move (v in and out, u in once): {36.0 * res['voxels'] / 1e9:.2f} GB, {floor_ms:.2f} ms at the 6.3 TB/s a streaming kernel reaches on this "
             f"device.  The step takes {res['step_ms_median'] / floor_ms:.1f} x that, so HBM does not bound it; presumably the 24 four-byte gathers per voxel do (no counters were collected; pairing the two "
             f"taps of a row into one load has not been tried).  The fixed grid of 256 blocks leaves `field_residual_kernel` one block per compute unit, which is why a pass costs more "
             f"than a step.  One pass of `field_residual_kernel` takes {res['residual_ms_median']:.3f} ms; it runs twice per call, so fusing it into the step could save at most "
             f"{2 * res['residual_ms_median']:.2f} ms of {res['iterations'] * res['step_ms_median'] + 2 * res['residual_ms_median']:.2f} ms of kernel time while adding a reduction to "
             f"every step: no fused variant was built and no A/B of one was run.  The whole call, with the upload of u and the download of v, takes "
             f"{res['call_ms_median']:.0f} ms; the residual max went from {res['residual_max_before']:.3g} to {res['residual_max_after']:.3g} voxel; peak device memory "
             f"{res['peak_device_bytes'] / 1e9:.2f} GB.\n")
    if "pair" in res:
        p = res["pair"]
        parts = lambda d: ", ".join(f"{k} {v:.1f}" for k, v in sorted(d.items()))  # noqa: E731
        text += ("\n## End to end\n\n"
                 f"{p['phases']} phase images of a sphere that moves {p['travel_voxels']:g} voxels along z, signals [amplitude, rate], reference phase {p['reference_phase']}, the "
                 "registration's default parameters (3 levels x 800 iterations), no engine context (the fits and the predictions run on the host in numpy).  Wall seconds, one run "
                 "each, in this order in one process.\n\n"
                 "| what | s | of which (s) |\n|---|---|---|\n"
                 f"| `build_pair` | {p['build_pair_s']:.1f} | {parts(p['build_pair_parts_s'])} |\n"
                 f"| `build_default` + `build_default(inverse=True)` | {p['two_build_default_s']:.1f} | {parts(p['two_build_default_parts_s'])} |\n\n"
                 f"`build_pair` takes {p['build_pair_s'] / p['two_build_default_s']:.2f} x the time of the two sweeps.  The {p['phases']} inversions spend "
                 f"{p['inversion_ms_step'] / 1e3:.2f} s in the step kernel and end with a residual of at most {p['inversion_residual_max']:.3g} voxel.  Pair residual (rms, voxels) per "
                 f"training state: derived pair {', '.join(f'{v:.3f}' for v in p['build_pair_pair_rms'])}; the two registered models "
                 f"{', '.join(f'{v:.3f}' for v in p['two_build_default_pair_rms'])}.\n")
    return text


if __name__ == "__main__":
    main()
