"""Time "CT image and segmentations in host memory" -> "context ready to launch" on the two routes, at the reference's size
(512 x 512 x 256; image and segmentations from workloads.synthetic_ct(MCThoraxLikeGeometry(bone_texture=True))):

  (a) host route  : MaterialMapperPipeline.execute (numpy + scipy erosion) + Context.set_geometry, i.e. mcgpu_set_geometry_arrays:
                    "%.6f" pass, palette, tiling and brick classification on the host, then the upload.  With --parent-lib PATH the
                    engine half runs in that library (the build of the commit before the device route existed); the function is the
                    same code in both.
  (b) device route: Context.set_geometry_image: copies of image + segmentations, one mapping kernel, palette from the class
                    statistics, brick levels and tile records by the device kernels.

The two routes alternate in one process after one warm-up round; both calls end with the device synchronised.  Per route: median and
[min, max] over the rounds.  The mapping kernel alone (HIP events) is reported as bytes moved once (every input byte read, every
volume byte written) over its time, against the streaming-copy rate mcgpu_microbench measures in the same run.  Prints the table,
optionally writes it (--out), and ends with one JSON line.
Usage: python tools/image_map_bench.py [--rounds 3] [--shape 512,512,256] [--dtype int16|float32] [--parent-lib PATH] [--out FILE.md]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402


class ArraysContext:
    """mcgpu_create / mcgpu_set_geometry_arrays / mcgpu_destroy of another build of the engine library (route (a) on the parent commit)."""

    def __init__(self, lib_path, input_path, device=0):
        self.lib = C.CDLL(str(lib_path))
        self.lib.mcgpu_last_error.restype = C.c_char_p
        self.lib.mcgpu_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        self.lib.mcgpu_set_geometry_arrays.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.lib.mcgpu_destroy.argtypes = [C.c_void_p]
        self.lib.mcgpu_destroy.restype = None
        self.h = C.c_void_p()
        self._check(self.lib.mcgpu_create(str(input_path).encode(), int(device), C.byref(self.h)))

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"[{rc}] {self.lib.mcgpu_last_error().decode(errors='replace')}")

    def set_geometry(self, geometry):
        mats, dens, spacing_cm = geometry.mcgpu_arrays()
        nx, ny, nz = mats.shape
        m = np.ascontiguousarray(np.transpose(mats, (2, 1, 0)), dtype=np.uint8)
        d = np.ascontiguousarray(np.transpose(dens, (2, 1, 0)), dtype=np.float32)
        self._check(self.lib.mcgpu_set_geometry_arrays(self.h, (C.c_int * 3)(nx, ny, nz), (C.c_float * 3)(*map(float, spacing_cm)), m.ctypes.data, d.ctypes.data))

    def close(self):
        if self.h:
            self.lib.mcgpu_destroy(self.h)
            self.h = None


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def fmt(s, unit="ms", digits=1):
    return f"{s['median']:.{digits}f} [{s['min']:.{digits}f}, {s['max']:.{digits}f}] {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", default="512,512,256")
    ap.add_argument("--dtype", default="int16", choices=("int16", "float32"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    eng, geo = pkg.engine, pkg.geometry
    eng.load_library()
    shape = tuple(int(v) for v in args.shape.split(","))
    spacing = tuple(512.0 / shape[0] * s for s in (1.0, 1.0, 1.0))
    image, segs = pkg.workloads.synthetic_ct(geo.MCThoraxLikeGeometry(shape=shape, image_spacing=spacing, bone_texture=True), dtype=np.dtype(args.dtype))
    n = image.size
    kw = {f"{k}_segmentation": v for k, v in segs.items()}
    out = {"shape": list(shape), "voxels": n, "image_dtype": args.dtype, "rounds": args.rounds, "parent_lib": bool(args.parent_lib)}
    a = dict(wall=[], map=[], install=[])
    b = dict(wall=[], upload=[], kernel=[], install=[])
    with tempfile.TemporaryDirectory() as tmp:
        sim = pkg.simulation.MCSimulation(geo.MCAirGeometry(), pkg.workloads.material_files(), pkg.workloads.spectrum_file(), n_histories=100_000, n_projections=1)
        inp = str(sim.prepare_simulation(Path(tmp)))
        ctx_b = eng.create(inp, device=0)
        ctx_a = ArraysContext(args.parent_lib, inp) if args.parent_lib else eng.create(inp, device=0)
        try:
            out["copy_rate_tb_per_s"] = ctx_b.microbench("copy_rate") / 1e12
            for i in range(args.rounds + 1):  # round 0 warms both routes up
                t0 = time.perf_counter()
                m, d = geo.MaterialMapperPipeline.create_default_pipeline(**kw).execute(image)
                t1 = time.perf_counter()
                ctx_a.set_geometry(geo.MCGeometry(m, d, spacing))
                t2 = time.perf_counter()
                rep = ctx_b.set_geometry_image(image, segs, frame="geometry", image_spacing=spacing)
                t3 = time.perf_counter()
                if i == 0:
                    continue
                a["wall"].append((t2 - t0) * 1e3); a["map"].append((t1 - t0) * 1e3); a["install"].append((t2 - t1) * 1e3)
                b["wall"].append((t3 - t2) * 1e3); b["upload"].append(rep["ms_upload"]); b["kernel"].append(rep["ms_kernel"]); b["install"].append(rep["ms_install"])
            out["kernel_bytes"] = rep["kernel_bytes"]
            out["class_counts"] = rep["count"]
            if not args.parent_lib:  # after the timed rounds: the voxels of both contexts
                out["routes_equal"] = bool(np.array_equal(ctx_a.host_table("voxel_mat_dens"), ctx_b.host_table("voxel_mat_dens")))
        finally:
            ctx_a.close()
            ctx_b.close()
    out["host_route"] = {k: stats(v) for k, v in a.items()}
    out["device_route"] = {k: stats(v) for k, v in b.items()}
    tbs = out["kernel_bytes"] / (out["device_route"]["kernel"]["median"] * 1e-3) / 1e12
    out["kernel_tb_per_s"] = tbs
    out["kernel_fraction_of_copy_rate"] = tbs / out["copy_rate_tb_per_s"] if out["copy_rate_tb_per_s"] > 0 else None
    out["spread_ms"] = max(s["wall"]["max"] - s["wall"]["min"] for s in (out["host_route"], out["device_route"]))
    out["wall_ratio_a_over_b"] = out["host_route"]["wall"]["median"] / out["device_route"]["wall"]["median"]
    ha, db = out["host_route"], out["device_route"]
    lines = [f"{'x'.join(map(str, shape))} voxels, {args.dtype} image, 8 segmentations, {args.rounds} rounds after one warm-up, routes alternating in one process"
             + (" (route (a)'s engine half in the parent commit's library)" if args.parent_lib else ""), "",
             "| route | wall, arrays in host memory -> context ready | mapping | rest |", "|---|---|---|---|",
             f"| (a) numpy execute + set_geometry | {fmt(ha['wall'])} | numpy {fmt(ha['map'])} | set_geometry {fmt(ha['install'])} |",
             f"| (b) set_geometry_image | {fmt(db['wall'])} | copies to the device {fmt(db['upload'])}, kernel {fmt(db['kernel'], digits=3)} | palette, brick levels, tables, upload {fmt(db['install'])} |",
             "",
             f"- median wall (a) / (b) = {out['wall_ratio_a_over_b']:.1f}; run-to-run spread (larger max - min of the two) {out['spread_ms']:.1f} ms",
             f"- mapping kernel: {out['kernel_bytes'] / 1e6:.0f} MB moved once in {db['kernel']['median']:.3f} ms = {tbs:.2f} TB/s, "
             f"{100 * out['kernel_fraction_of_copy_rate']:.0f} % of the {out['copy_rate_tb_per_s']:.2f} TB/s a streaming copy reaches in the same run (mcgpu_microbench)",
             f"- voxels per class (air .. blood): {out['class_counts']}"]
    if "routes_equal" in out:
        lines.append(f"- both contexts hold the same voxels: {out['routes_equal']}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
