"""Time the water pre-correction fit at the reference's size: 894 projections of 1024 x 768 pixels of 0.388 mm, half-fan offset
-159.856 mm, pad 1, hann 1, hannY 1, volume 464 x 250 x 464 at 1 mm, slab of 50 slices, order 5.  The projections are the exact chords
of the water phantom's cylinder (radius 100 mm) under a two-energy beam; weight and template come from
water_precorrection.phantom_weight_and_template(MCWaterPhantomGeometry(shape=(464, 464, 250))).

  fused    : water_precorrection.normal_equations (mcgpu_wpc_fit), once per layout of the back-projector's input (1 = one plane per
             power, 2 = powers interleaved per pixel): wall time and the report's stages
  composed : the route without the fused call: order + 1 reconstruction.fdk(..., water_pre_correction=e_n) calls, the slab mean of
             each volume and the (order + 1)^2 + order + 1 weighted sums in numpy
  --resources : VGPRs, waves per SIMD and scratch of every slab_backproject instantiation, from the compiler's resource-usage remarks
             (needs hipcc, no GPU)

One warm-up round, then --rounds rounds (at least 5) of the fused route and --composed-rounds of the composed one; every call ends
with the device synchronised.  Median [min, max].  Prints the tables, optionally writes them (--out), and ends with one JSON line.
Usage: python tools/wpc_fit_bench.py [--rounds 5] [--composed-rounds 5] [--order 5] [--projections 894] [--out FILE.md] [--resources]"""
from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

NU, NV, PIX, DIM, SPACING, SLICES = 1024, 768, 0.388, (464, 250, 464), (1.0, 1.0, 1.0), 50


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def fmt(s, unit="ms", digits=0):
    return f"{s['median']:.{digits}f} [{s['min']:.{digits}f}, {s['max']:.{digits}f}] {unit}"


def cylinder_projection(radius, off_x, sid, sdd):
    """[NV][NU] line integrals of a long water cylinder about the rotation axis (the same for every gantry angle) under a beam of two
    energies, mu = 0.03 and 0.015 per mm."""
    u = -(NU - 1) / 2 * PIX + PIX * np.arange(NU) + off_x
    v = -(NV - 1) / 2 * PIX + PIX * np.arange(NV)
    dx, dy = np.meshgrid(u, v)
    qa, qb, qc = dx * dx + sdd * sdd, -2.0 * sid * sdd, sid * sid - radius * radius
    disc = qb * qb - 4.0 * qa * qc
    L = np.where(disc > 0, np.sqrt(np.maximum(disc, 0.0)) / qa * np.sqrt(dx * dx + dy * dy + sdd * sdd), 0.0)
    return (-np.log(0.5 * np.exp(-0.03 * L) + 0.5 * np.exp(-0.015 * L))).astype(np.float32)


def resources():
    """{(powers, layout): (vgprs, waves per SIMD, scratch bytes)} of slab_backproject_kernel, from hipcc's remarks."""
    src = ROOT / "4d-cbct-mc_amd" / "csrc" / "wpc_fit.hip"
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          "-c", str(src), "-o", "/dev/null"], capture_output=True, text=True, check=True).stderr
    table = {}
    for block in out.split("Function Name: ")[1:]:
        m = re.match(r"\S*slab_backproject_kernelILi(\d)ELb(\d)E", block)
        if m:
            value = {k: int(re.search(k + r"[^:]*: (\d+)", block).group(1)) for k in ("VGPRs", "Occupancy", "ScratchSize")}
            table[(int(m.group(1)), 2 if m.group(2) == "1" else 1)] = (value["VGPRs"], value["Occupancy"], value["ScratchSize"])
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--composed-rounds", type=int, default=5)
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--projections", type=int, default=894)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    lines, out = [], {}
    if args.resources:
        table = resources()
        out["resources"] = {f"{c}_{layout}": v for (c, layout), v in sorted(table.items())}
        lines += ["| powers (order + 1) | layout | VGPRs | waves per SIMD | scratch bytes per lane |", "|---|---|---|---|---|"]
        lines += [f"| {c} | {'interleaved' if layout == 2 else 'planes'} | {v[0]} | {v[1]} | {v[2]} |" for (c, layout), v in sorted(table.items())]
        lines.append("")
    if args.rounds > 0:
        pkg = load_package()
        wp, recon = pkg.water_precorrection, pkg.reconstruction
        pkg.engine.load_library()
        n, order = args.projections, args.order
        geo = recon.create_geometry(n, start_angle=90.0)
        proj = np.broadcast_to(cylinder_projection(100.0, geo.projection_offsets_x[0], geo.source_to_isocenter, geo.source_to_detector), (n, NV, NU)).copy()
        weight, template, slab = wp.phantom_weight_and_template(pkg.geometry.MCWaterPhantomGeometry(shape=(DIM[0], DIM[2], DIM[1])), SLICES)
        common = (proj, geo, (PIX, PIX), None, DIM, SPACING)
        t = {f"{k}_{layout}": [] for layout in (1, 2) for k in ("wall", "ms_upload", "ms_filter", "ms_backproject", "ms_reduce")}
        t["composed"] = []
        fused, composed = {}, None
        for i in range(args.rounds + 1):  # round 0 warms both layouts up
            for layout in (1, 2):
                t0 = time.perf_counter()
                B, a, basis, rep = wp.normal_equations(*common, weight, template, slab, order, None, 1.0, 1.0, 1.0, channel_layout=layout)
                wall = (time.perf_counter() - t0) * 1e3
                fused[layout] = (B, a, basis, rep)
                if i:
                    t[f"wall_{layout}"].append(wall)
                    for k in ("ms_upload", "ms_filter", "ms_backproject", "ms_reduce"):
                        t[f"{k}_{layout}"].append(rep[k])
        for i in range(args.composed_rounds + 1 if args.composed_rounds > 0 else 0):
            t0 = time.perf_counter()
            e = np.eye(order + 1)
            means = [recon.fdk(*common, None, 1.0, 1.0, e[k], pad=1.0)[0][:, slab[0]: slab[0] + slab[1], :].mean(1) for k in range(order + 1)]
            Bc = np.array([[np.sum(weight * fi * fj, dtype=np.float64) for fj in means] for fi in means])
            ac = np.array([np.sum(weight * fi * template, dtype=np.float64) for fi in means])
            if i:
                t["composed"].append((time.perf_counter() - t0) * 1e3)
            composed = (Bc, ac, np.stack(means))
        s = {k: stats(v) for k, v in t.items() if v}
        out.update(projections=n, order=order, slab=list(slab), rounds=args.rounds, composed_rounds=args.composed_rounds, times_ms=s,
                   peak_device_bytes={layout: int(fused[layout][3]["peak_device_bytes"]) for layout in (1, 2)},
                   layouts_equal=bool(all(x.tobytes() == y.tobytes() for x, y in zip(fused[1][:3], fused[2][:3]))))
        lines += [f"{n} projections of {NU} x {NV} pixels ({proj.nbytes / 1e9:.2f} GB), volume {DIM[0]} x {DIM[1]} x {DIM[2]}, slab {slab}, order {order}; "
                  f"{args.rounds} rounds after one warm-up", "",
                  "| route | wall | upload | filter | back-projection | reduction | peak device bytes |", "|---|---|---|---|---|---|---|"]
        for layout, label in ((1, "fused, one plane per power"), (2, "fused, powers interleaved per pixel")):
            lines.append(f"| {label} | {fmt(s[f'wall_{layout}'])} | {fmt(s[f'ms_upload_{layout}'])} | {fmt(s[f'ms_filter_{layout}'])} | "
                         f"{fmt(s[f'ms_backproject_{layout}'], digits=1)} | {fmt(s[f'ms_reduce_{layout}'], digits=2)} | {out['peak_device_bytes'][layout] / 1e9:.2f} GB |")
        if composed is not None:
            lines.append(f"| composed: {order + 1} fdk() calls + numpy sums | {fmt(s['composed'])} | | | | | |")
            scale = np.abs(composed[2]).max(axis=(1, 2))
            diff = np.abs(fused[2][2].astype(np.float64) - composed[2]).max(axis=(1, 2)) / scale
            out["fused_vs_composed_basis"] = [float(v) for v in diff]
            c_fused, c_composed = wp.solve(fused[2][0], fused[2][1]), wp.solve(*composed[:2])
            out["coefficients_fused"], out["coefficients_composed"] = [float(v) for v in c_fused], [float(v) for v in c_composed]
            out["condition"] = float(np.linalg.cond(fused[2][0]))
            lines += ["", f"- max |fused - composed| / max |composed| of the slab means per power: {', '.join(f'{v:.1e}' for v in diff)}",
                      f"- cond(B) = {out['condition']:.3g}; c (fused) = {out['coefficients_fused']}", f"- c (composed) = {out['coefficients_composed']}"]
        lines.append(f"- both layouts give the same bytes (B, a, basis_mean): {out['layouts_equal']}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
