"""Time the demons registration at the reference's size, beside the same loop written with torch ops on the same GPU.

  level    : one level at 500 x 500 x 300 (the CIRS phantom with its insert, padded as scripts/create_cirs_phantom_4d.py pads it, phase 0
             against phase 2): registration.register(n_levels=1) with --level-iterations iterations; per iteration, the report's force and
             smoothing milliseconds and the bytes of the rule's traffic model (100 B per voxel: 28 for the force step, 24 per pass) over
             that time; the torch loop with the same number of iterations, timed with the device synchronised
  build    : what CorrespondenceModel.build_default does on --phases CIRS phases (MCCIRSPhantomGeometry.place_insert shifts along z by the
             cos^4 curve of the script, amplitude 20, minus 10): the registrations of every phase against phase 2 with --iterations
             iterations on each of --levels levels, wall time over --rounds rounds; the torch loop on the same pairs with
             --torch-iterations iterations (default: the same number; when it differs the kernels are timed at that number too) over
             --torch-rounds rounds; then one whole build_default, the host fit included

The torch loop (torch_register) is the rule with library operators: trilinear interpolate(align_corners=True) for the levels,
grid_sample(border, align_corners=True) for the warp, slices of a replicate-padded volume for the gradient (computed once per level, which
favours it), three conv3d over a replicate-padded field for the Gaussian.  Its field is compared with the kernels' (max difference).
One warm-up, then --rounds rounds (at least 5 for a figure that is to be quoted); median [min, max].  Prints the tables, optionally
writes them (--out), and ends with one JSON line.
Usage: python tools/registration_bench.py [--rounds 5] [--level-iterations 20] [--phases 10] [--iterations 800] [--levels 3]
       [--torch-iterations N] [--torch-rounds N] [--skip-level] [--skip-build] [--skip-torch] [--out FILE.md]"""
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

SHAPE = (500, 500, 300)
BYTES_PER_VOXEL = {"force": 28, "smooth": 72}


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def fmt(s, unit="ms", digits=1):
    return f"{s['median']:.{digits}f} [{s['min']:.{digits}f}, {s['max']:.{digits}f}] {unit}"


def cirs_phases(pkg, n_phases, shape=SHAPE):
    """(images [T, x, y, z] float32 densities, signals [T, 2]) as scripts/create_cirs_phantom_4d.py makes them."""
    RespiratorySignal = pkg.respiratory.RespiratorySignal
    period = 5.0
    curve = RespiratorySignal.create_cos4(total_seconds=period, amplitude=20.0, sampling_frequency=25.0).resample(n_phases / period)
    base = pkg.geometry.MCCIRSPhantomGeometry.from_base_geometry()
    images = np.stack([base.place_insert(shift=(0, 0, -(float(a) - 10.0))).pad_to_shape(shape).densities for a in curve.signal]).astype(np.float32)
    return images, np.stack([curve.signal, curve.dt_signal], axis=-1)


def torch_register(fixed, moving, mask=None, iterations=800, tau=2.25, sigma=(1.25, 1.25, 1.25), n_levels=3, device="cuda"):
    """The rule with torch operators, float32 on `device`: -> field float32 [3, x, y, z] (numpy)."""
    import torch
    import torch.nn.functional as F
    lib = load_package().registration
    full = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=device)[None, None] for a in (fixed, moving)]
    full_mask = None if mask is None else torch.as_tensor(np.ascontiguousarray(mask != 0, dtype=np.float32), device=device)[None, None]
    kernels = []
    for axis in range(3):
        if sigma[axis] == 0:
            kernels.append(None)
            continue
        r = int(4.0 * sigma[axis] + 0.5)
        k = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma[axis] ** 2))
        view = [1, 1, 1, 1, 1]
        view[2 + axis] = -1
        kernels.append((r, torch.as_tensor((k / k.sum()).astype(np.float32), device=device).reshape(view)))
    u = None
    for level in range(n_levels - 1, -1, -1):
        shape = lib.level_shape(fixed.shape, level)
        if level:
            f, m = (F.interpolate(a, size=shape, mode="trilinear", align_corners=True) for a in full)
            w_mask = None if full_mask is None else F.interpolate(full_mask, size=shape, mode="nearest")
        else:
            (f, m), w_mask = full, full_mask
        if u is None:
            u = torch.zeros((1, 3) + shape, dtype=torch.float32, device=device)
        else:
            scale = [1.0 if o == 1 else (n - 1) / (o - 1) for o, n in zip(u.shape[2:], shape)]
            u = F.interpolate(u, size=shape, mode="trilinear", align_corners=True) * torch.tensor(scale, dtype=torch.float32, device=device).view(1, 3, 1, 1, 1)
        ident = torch.stack(torch.meshgrid(*(torch.arange(n, dtype=torch.float32, device=device) for n in shape), indexing="ij"))[None]
        norm = torch.tensor([2.0 / max(n - 1, 1) for n in shape], dtype=torch.float32, device=device).view(1, 3, 1, 1, 1)
        p = F.pad(f, (1, 1, 1, 1, 1, 1), mode="replicate")
        g = torch.cat([0.5 * (p[:, :, 2:, 1:-1, 1:-1] - p[:, :, :-2, 1:-1, 1:-1]), 0.5 * (p[:, :, 1:-1, 2:, 1:-1] - p[:, :, 1:-1, :-2, 1:-1]),
                       0.5 * (p[:, :, 1:-1, 1:-1, 2:] - p[:, :, 1:-1, 1:-1, :-2])], dim=1)
        g2 = (g * g).sum(dim=1, keepdim=True)
        del p
        for _ in range(iterations):
            grid = ((ident + u) * norm - 1.0).flip(1).permute(0, 2, 3, 4, 1)  # grid_sample wants (z, y, x) of its (D, H, W) input last
            d = F.grid_sample(m, grid, mode="bilinear", padding_mode="border", align_corners=True) - f
            den = g2 + d * d
            v = torch.where(den > 1e-9, -d * g / den, torch.zeros((), dtype=torch.float32, device=device))
            if w_mask is not None:
                v = v * w_mask
            u = u + tau * v
            c = u.permute(1, 0, 2, 3, 4)
            for axis, kernel in enumerate(kernels):
                if kernel is None:
                    continue
                pad = [0, 0, 0, 0, 0, 0]
                pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = kernel[0]
                c = F.conv3d(F.pad(c, pad, mode="replicate"), kernel[1])
            u = c.permute(1, 0, 2, 3, 4)
    torch.cuda.synchronize()
    return u[0].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--level-iterations", type=int, default=20)
    ap.add_argument("--phases", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=800)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--torch-iterations", type=int, default=None)
    ap.add_argument("--torch-rounds", type=int, default=None)
    ap.add_argument("--shape", type=int, nargs=3, default=list(SHAPE))
    ap.add_argument("--skip-level", action="store_true")
    ap.add_argument("--skip-build", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the engine library brings up HIP
    pkg = load_package()
    reg, Model = pkg.registration, pkg.correspondence.CorrespondenceModel
    pkg.engine.load_library()
    shape = tuple(args.shape)
    images, signals = cirs_phases(pkg, args.phases, shape)
    reference = min(2, args.phases - 1)
    voxels = int(np.prod(shape))
    lines, out = [], dict(shape=list(shape), rounds=args.rounds, phases=args.phases, gpu=torch.cuda.get_device_name(0))
    t = {}

    if not args.skip_level:
        n = args.level_iterations
        kw = dict(iterations=n, n_levels=1)
        hip_field = torch_field = None
        for i in range(args.rounds + 1):  # round 0 warms up
            t0 = time.perf_counter()
            hip_field, rep = reg.register(images[0], images[reference], **kw)
            wall = (time.perf_counter() - t0) * 1e3
            if i:
                for key, value in (("hip_wall", wall), ("hip_force", rep["ms_force"] / n), ("hip_smooth", rep["ms_smooth"] / n), ("hip_upload", rep["ms_upload"])):
                    t.setdefault(key, []).append(value)
            if not args.skip_torch:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                torch_field = torch_register(images[0], images[reference], **kw)
                if i:
                    t.setdefault("torch_wall", []).append((time.perf_counter() - t0) * 1e3)
        s = {k: stats(v) for k, v in t.items()}
        out["peak_device_bytes"] = int(rep["peak_device_bytes"])
        lines += [f"One level at {shape[0]} x {shape[1]} x {shape[2]} ({voxels / 1e6:.0f} M voxels), {n} iterations, {args.rounds} rounds after one warm-up; "
                  f"peak device memory {rep['peak_device_bytes'] / 1e9:.2f} GB", "",
                  "| route | per iteration | force step | smoothing (3 passes) | whole call (wall, copies included) |", "|---|---|---|---|---|"]
        per_iteration = stats(np.asarray(t["hip_force"]) + np.asarray(t["hip_smooth"]))
        s["hip_iteration"] = per_iteration
        lines.append(f"| HIP kernels | {fmt(per_iteration, digits=2)} | {fmt(s['hip_force'], digits=2)} | {fmt(s['hip_smooth'], digits=2)} | {fmt(s['hip_wall'], digits=0)} |")
        for key in ("force", "smooth"):
            out[f"{key}_model_TBps"] = BYTES_PER_VOXEL[key] * voxels / (s[f"hip_{key}"]["median"] * 1e-3) / 1e12
        lines.append(f"| traffic model over time | | {out['force_model_TBps']:.2f} TB/s (28 B per voxel) | {out['smooth_model_TBps']:.2f} TB/s (72 B per voxel) | |")
        if not args.skip_torch:
            # the torch call's wall time holds its uploads too; its loop alone = wall - the kernels' route's copies is not known, so the whole calls are compared
            lines.append(f"| torch loop | {s['torch_wall']['median'] / n:.2f} ms (whole call / iterations) | | | {fmt(s['torch_wall'], digits=0)} |")
            out["level_field_max_difference"] = float(np.abs(hip_field - torch_field).max())
            out["level_speedup_whole_call"] = s["torch_wall"]["median"] / s["hip_wall"]["median"]
            lines += ["", f"- whole call, torch / HIP: {out['level_speedup_whole_call']:.2f} x; max |field difference| {out['level_field_max_difference']:.3g} voxel "
                          f"(max |field| {float(np.abs(hip_field).max()):.3g})"]
        # every operator alone, through the stage entry point (kernel time of the stage's report)
        alone = {}
        field = hip_field
        for i in range(args.rounds + 1):
            for name, sigma in (("smooth_x", (1.25, 0, 0)), ("smooth_y", (0, 1.25, 0)), ("smooth_z", (0, 0, 1.25))):
                rep_stage = reg.register_stage("smooth", field=field, sigma=sigma)[1]
                if i:
                    alone.setdefault(name, []).append(rep_stage["ms_smooth"])
            rep_stage = reg.register_stage("force_step", fixed=images[0], moving=images[reference], field=field)[1]
            if i:
                alone.setdefault("force_step", []).append(rep_stage["ms_force"])
        lines += ["", "Every kernel alone on the field of that call (`register_stage`, kernel time):", "", "| kernel | time | traffic model over time |", "|---|---|---|"]
        for name, v in alone.items():
            s[name] = stats(v)
            model_bytes = (28 if name == "force_step" else 24) * voxels
            lines.append(f"| {name} | {fmt(s[name], digits=3)} | {model_bytes / (s[name]['median'] * 1e-3) / 1e12:.2f} TB/s |")
        lines.append("")
        out["level_ms"] = s

    if not args.skip_build:
        kw = dict(iterations=args.iterations, n_levels=args.levels)
        n_torch = args.iterations if args.torch_iterations is None else args.torch_iterations
        torch_rounds = args.rounds if args.torch_rounds is None else args.torch_rounds
        pairs = lambda f, **k: np.stack([f(images[p], images[reference], **k) for p in range(args.phases)])  # noqa: E731
        hip = lambda fixed, moving, **k: reg.register(fixed, moving, **k)[0]  # noqa: E731
        runs = [("hip", hip, args.iterations, args.rounds)]
        if not args.skip_torch:
            if n_torch != args.iterations:
                runs.append(("hip_short", hip, n_torch, torch_rounds))
            runs.append(("torch", torch_register, n_torch, torch_rounds))
        seconds, fields = {}, {}
        for name, f, iterations, rounds in runs:
            for i in range(rounds + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fields[name] = pairs(f, iterations=iterations, n_levels=args.levels)
                if i:
                    seconds.setdefault(name, []).append(time.perf_counter() - t0)
        s_build = {name: stats(v) for name, v in seconds.items()}
        out["register_pairs_s"] = s_build
        lines += [f"The {args.phases} registrations of build_default on CIRS phases of {shape[0]} x {shape[1]} x {shape[2]} (moving = phase {reference}), {args.levels} levels, "
                  f"one warm-up round each; wall time with the copies to and from the host", "", "| route | iterations per level | rounds | wall |", "|---|---|---|---|"]
        labels = dict(hip="HIP kernels", hip_short="HIP kernels", torch="torch loop")
        for name, _, iterations, rounds in runs:
            lines.append(f"| {labels[name]} | {iterations} | {rounds} | {fmt(s_build[name], 's', 2)} |")
        if "torch" in s_build:
            same = "hip_short" if "hip_short" in s_build else "hip"
            out["register_pairs_speedup"] = s_build["torch"]["median"] / s_build[same]["median"]
            out["register_pairs_max_difference"] = float(np.abs(fields["torch"] - fields[same]).max())
            lines += ["", f"- torch / HIP at {n_torch} iterations per level: {out['register_pairs_speedup']:.2f} x; max |field difference| "
                          f"{out['register_pairs_max_difference']:.3g} voxel (max |field| {float(np.abs(fields[same]).max()):.3g})"]
        del fields
        t0 = time.perf_counter()
        model = Model.build_default(images, signals=signals, reference_phase=reference, **kw)
        out["build_default_s"] = time.perf_counter() - t0
        mean_uz = float(np.abs(np.asarray(model.mean_vector_field).reshape(3, *shape)[2]).max())
        lines += [f"- one whole build_default ({args.iterations} iterations per level, the fit on the host included; a single run): {out['build_default_s']:.1f} s; "
                  f"largest |z component| of the model's mean field {mean_uz:.2f} voxels"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
