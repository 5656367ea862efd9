"""Time the device resampler on a clinical CT: an int16 image of 512 x 512 x 160 voxels at (0.9765625, 0.9765625, 2.5) mm with eight
segmentations (workloads.synthetic_ct of the bone-textured thorax phantom at that shape), resampled to 1 mm (500 x 500 x 400).

  kernels : Context.resample_volume of the image (linear) and of one segmentation (nearest): kernel time (HIP events), the bytes of the
            input and output arrays, the bandwidth that implies, against the streaming-copy rate mcgpu_microbench measures in the same run
  (a)     : nine Context.resample_volume calls (every result comes back to the host) followed by Context.set_geometry_image
  (b)     : Context.set_geometry_image_resampled: the native arrays go up once, nothing comes back
  (c)     : Context.set_geometry_from_image(image_spacing=(1, 1, 1)) on uncompressed .mha files: (b) plus reading the files

Routes alternate in one process after one warm-up round; every call ends with the device synchronised.  Median and [min, max] over the
rounds.  Prints the table, optionally writes it (--out), and ends with one JSON line.
Usage: python tools/resample_bench.py [--rounds 3] [--shape 512,512,160] [--out FILE.md]"""
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

CT, ONE = (0.9765625, 0.9765625, 2.5), (1.0, 1.0, 1.0)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def fmt(s, unit="ms", digits=1):
    return f"{s['median']:.{digits}f} [{s['min']:.{digits}f}, {s['max']:.{digits}f}] {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", default="512,512,160")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    eng, geo, recon = pkg.engine, pkg.geometry, pkg.reconstruction
    eng.load_library()
    shape = tuple(int(v) for v in args.shape.split(","))
    image, segs = pkg.workloads.synthetic_ct(geo.MCThoraxLikeGeometry(shape=shape, image_spacing=CT, bone_texture=True), dtype=np.dtype(np.int16))
    out = {"shape": list(shape), "spacing": list(CT), "new_spacing": list(ONE), "rounds": args.rounds, "segmentations": len(segs)}
    t = dict(image_kernel=[], seg_kernel=[], a_wall=[], a_resample=[], b_wall=[], b_kernel=[], b_upload=[], b_install=[], c_wall=[])
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        sim = pkg.simulation.MCSimulation(geo.MCAirGeometry(), pkg.workloads.material_files(), pkg.workloads.spectrum_file(), n_histories=100_000, n_projections=1)
        inp = str(sim.prepare_simulation(tmp))
        recon.write_mha(tmp / "ct.mha", image.swapaxes(0, 2), CT, (0.0, 0.0, 0.0), element_type="MET_SHORT")
        paths = {f"{k}_segmentation_filepath": recon.write_mha(tmp / f"{k}.mha", v.swapaxes(0, 2), CT, (0.0, 0.0, 0.0), element_type="MET_UCHAR")
                 for k, v in segs.items()}
        with eng.create(inp, device=0) as ctx:
            out["copy_rate_tb_per_s"] = ctx.microbench("copy_rate") / 1e12
            for i in range(args.rounds + 1):  # round 0 warms every route up
                t0 = time.perf_counter()
                r_image = ctx.resample_volume(image, CT, ONE, "linear", geo.IMAGE_DEFAULT_HU)
                k_image, bytes_image = ctx.last_resample_report["ms_kernel"], ctx.last_resample_report["kernel_bytes"]
                r_segs = {}
                for k, v in segs.items():
                    r_segs[k] = ctx.resample_volume(v, CT, ONE, "nearest", 0.0)
                k_seg, bytes_seg = ctx.last_resample_report["ms_kernel"], ctx.last_resample_report["kernel_bytes"]
                t1 = time.perf_counter()
                ctx.set_geometry_image(r_image, r_segs, frame="geometry", image_spacing=ONE)
                t2 = time.perf_counter()
                voxels_a = ctx.host_table("voxel_mat_dens") if i == args.rounds else None
                t3 = time.perf_counter()
                rep = ctx.set_geometry_image_resampled(image, segs, CT, ONE, frame="geometry", image_default=geo.IMAGE_DEFAULT_HU)
                rrep = ctx.last_resample_report
                t4 = time.perf_counter()
                voxels_b = ctx.host_table("voxel_mat_dens") if i == args.rounds else None
                t5 = time.perf_counter()
                ctx.set_geometry_from_image(tmp / "ct.mha", image_spacing=ONE, **paths)
                t6 = time.perf_counter()
                if i == 0:
                    continue
                t["image_kernel"].append(k_image); t["seg_kernel"].append(k_seg)
                t["a_wall"].append((t2 - t0) * 1e3); t["a_resample"].append((t1 - t0) * 1e3)
                t["b_wall"].append((t4 - t3) * 1e3); t["b_kernel"].append(rrep["ms_kernel"]); t["b_upload"].append(rrep["ms_upload"])
                t["b_install"].append(rep["ms_install"]); t["c_wall"].append((t6 - t5) * 1e3)
            out["resampled_shape"] = list(r_image.shape)
            out["routes_equal"] = bool(np.array_equal(voxels_a, voxels_b))
            out["bytes"] = {"image": bytes_image, "segmentation": bytes_seg, "chain": rrep["kernel_bytes"]}
    s = {k: stats(v) for k, v in t.items()}
    out["times_ms"] = s
    rate = {k: out["bytes"][b] / (s[m]["median"] * 1e-3) / 1e12 for k, b, m in (("image", "image", "image_kernel"), ("segmentation", "segmentation", "seg_kernel"),
                                                                               ("chain", "chain", "b_kernel"))}
    out["tb_per_s"] = rate
    copy = out["copy_rate_tb_per_s"]
    lines = [f"{'x'.join(map(str, shape))} int16 CT at {CT} mm and {len(segs)} uint8 segmentations -> {ONE} mm = {'x'.join(map(str, out['resampled_shape']))}; "
             f"{args.rounds} rounds after one warm-up, routes alternating in one process", "",
             "| kernel | time (HIP events) | bytes of input + output | bandwidth | of the streaming copy |", "|---|---|---|---|---|",
             f"| image, linear, int16 | {fmt(s['image_kernel'], digits=3)} | {out['bytes']['image'] / 1e6:.0f} MB | {rate['image']:.2f} TB/s | {100 * rate['image'] / copy:.0f} % |",
             f"| one segmentation, nearest, uint8 | {fmt(s['seg_kernel'], digits=3)} | {out['bytes']['segmentation'] / 1e6:.0f} MB | {rate['segmentation']:.2f} TB/s | {100 * rate['segmentation'] / copy:.0f} % |",
             f"| all nine in the chain | {fmt(s['b_kernel'], digits=3)} | {out['bytes']['chain'] / 1e6:.0f} MB | {rate['chain']:.2f} TB/s | {100 * rate['chain'] / copy:.0f} % |",
             "", f"streaming copy in the same run (mcgpu_microbench): {copy:.2f} TB/s", "",
             "| route | wall, arrays or files -> context ready | of which |", "|---|---|---|",
             f"| (a) nine resample_volume + set_geometry_image | {fmt(s['a_wall'])} | the nine calls {fmt(s['a_resample'])} |",
             f"| (b) set_geometry_image_resampled | {fmt(s['b_wall'])} | copies to the device {fmt(s['b_upload'])}, resampling kernels {fmt(s['b_kernel'], digits=3)}, install {fmt(s['b_install'])} |",
             f"| (c) set_geometry_from_image(image_spacing=...) on .mha files | {fmt(s['c_wall'])} | (b) plus reading {1 + len(segs)} files |",
             "", f"- routes (a) and (b) leave the same voxels: {out['routes_equal']}"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
