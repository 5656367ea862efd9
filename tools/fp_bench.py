"""Time the Joseph forward projector (csrc/forward_project.hip) at the reference's size: the Catphan604 geometry in 512^3 voxels of
1 mm, 894 projections of 1024 x 768 pixels (0.388 mm, half-fan offset -159.856 mm, start angle 90 degrees; what
`run-mc --forward-projection` computes for density_fp.mha).

Prints one line per measurement and a final JSON line:
  host     : mcgpu_forward_project on the float volume from the host (kernel ms, upload ms, rays/s)
  context  : mcgpu_forward_project_context on the same geometry resident in an engine context (u8 palette volume)
  axis A/B : 16 projections around 0 degrees (main axis = IEC Z, the slowest-varying axis of the volume: taps along x and y)
             against 16 around 90 degrees (main axis = IEC X, the fastest-varying one: taps strided along y and z)
Usage: python tools/fp_bench.py [--n-proj 894] [--n-vox 512] [--skip-context]"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-proj", type=int, default=894)
    ap.add_argument("--n-vox", type=int, default=512)
    ap.add_argument("--skip-context", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    fp, eng, d = pkg.forward_projection, pkg.engine, pkg.defaults.DEFAULTS
    eng.load_library()
    g = pkg.workloads.workload_geometry("catphan", args.n_vox)
    det, pix = d.n_detector_pixels_half_fan, d.detector_pixel_size
    img = fp.prepare_image_for_rtk(g.densities, image_spacing=g.image_spacing, input_value_range=None, output_value_range=None)
    rays = args.n_proj * det[0] * det[1]
    result = {"n_proj": args.n_proj, "n_vox": args.n_vox, "detector": list(det)}

    warm = fp.create_geometry(16, start_angle=90.0)
    fp.project_forward(img, warm, detector_size=det, detector_pixel_spacing=pix)  # code objects, allocator
    geo = fp.create_geometry(args.n_proj, start_angle=90.0)
    rep = {}
    t0 = time.perf_counter()
    out = fp.project_forward(img, geo, detector_size=det, detector_pixel_spacing=pix, report=rep)
    wall = time.perf_counter() - t0
    result["host"] = dict(ms_kernel=rep["ms_kernel"], ms_upload=rep["ms_upload"], s_wall=wall, rays_per_s=rays / (rep["ms_kernel"] * 1e-3),
                          max=float(out.array.max()), mean=float(out.array.mean()))
    print(f"host    : kernel {rep['ms_kernel']:.1f} ms, upload {rep['ms_upload']:.1f} ms, wall {wall:.2f} s, "
          f"{result['host']['rays_per_s']:.3e} rays/s", flush=True)

    for name, start in (("axis_z", 0.0), ("axis_x", 90.0)):
        gg = fp.create_geometry(16, start_angle=start - 8.0, arc=16.0)  # 16 projections, 1 degree apart
        r = {}
        fp.project_forward(img, gg, detector_size=det, detector_pixel_spacing=pix, report=r)
        result[name] = dict(ms_kernel=r["ms_kernel"], ms_per_projection=r["ms_kernel"] / 16)
        print(f"{name}  : {r['ms_kernel'] / 16:.2f} ms per projection", flush=True)

    if not args.skip_context:
        with tempfile.TemporaryDirectory() as tmp:
            sim = pkg.simulation.MCSimulation(pkg.geometry.MCAirGeometry(), pkg.workloads.material_files(), pkg.workloads.spectrum_file(),
                                              n_histories=100_000, n_projections=1)
            ctx = eng.create(str(sim.prepare_simulation(Path(tmp))), device=0)
            try:
                ctx.set_geometry(g)
                spacing, origin = fp.rtk_frame(g.image_shape, g.image_spacing)
                ctx.project_forward([90.0], spacing_iec=spacing, origin_iec=origin)  # warm-up
                t0 = time.perf_counter()
                got, r = ctx.project_forward(geo.gantry_angles, spacing_iec=spacing, origin_iec=origin)
                wall = time.perf_counter() - t0
                same = bool(np.array_equal(got, out.array))
                result["context"] = dict(volume_kind=ctx.geti("volume_kind"), ms_kernel=r["ms_kernel"], s_wall=wall,
                                         rays_per_s=rays / (r["ms_kernel"] * 1e-3), equals_host=same)
                print(f"context : volume kind {ctx.geti('volume_kind')}, kernel {r['ms_kernel']:.1f} ms, wall {wall:.2f} s, "
                      f"{result['context']['rays_per_s']:.3e} rays/s, equals host path: {same}", flush=True)
            finally:
                ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
