"""Time a respiratory state change of a resident context with and without the correspondence model on the device, on the CIRS
phantom (305 x 300 x 152) and the 512 x 512 x 256 thorax, K = 2, ten states each after one warm-up state, the two routes alternating:

  (a) host field : model.predict(signal) in numpy + ctx.warp_geometry(field)      predict | copy of the field | everything else
  (b) resident   : ctx.warp_geometry_by_signal(signal)                            wall, and the warp kernel alone (HIP events) with
                   its bytes -- 3 N (4 + 8 K) + N read, N written -- over that time against the HBM peak

Wall times end in a device synchronise (both calls read results back).  Per route: median and [min, max] over the ten states; the
run-to-run spread is the larger of the two routes' (max - min).  The fit (T = 10 fields) is timed once per volume, host numpy
against device (wall, upload included), for the volumes named by --fit.  Prints the table, optionally writes it (--out), and ends
with one JSON line.
Usage: python tools/correspondence_bench.py [--volumes cirs,thorax] [--fit cirs] [--states 10] [--out FILE.md]"""
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

HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3  # MI355X: specification / measured float4 copy


def breathing(T):
    t = np.arange(T)
    return 0.5 + 0.5 * np.cos(2 * np.pi * t / T), -np.pi / T * np.sin(2 * np.pi * t / T)


def motion_fields(shape):
    """Two smooth fields [3, x, y, z] in voxels: F moves with the signal (SI motion growing towards the diaphragm), G with its derivative."""
    x, y, z = (np.linspace(-1, 1, n, dtype=np.float32).reshape([-1 if a == k else 1 for a in range(3)]) for k, n in enumerate(shape))
    F = np.empty((3,) + tuple(shape), dtype=np.float32)
    F[0], F[1], F[2] = 1.5 * np.sin(2.0 * y) * (1 - x * x) + 0 * z, 2.0 * x * y + 0 * z, 6.0 * (1 - z) * np.cos(1.2 * x) * np.cos(1.2 * y)
    G = np.empty_like(F)
    G[0], G[1], G[2] = 2.0 * z * x + 0 * y, 1.5 * np.sin(3.0 * x + y) + 0 * z, 1.0 * y * y - 0.5 + 0 * x * z
    return F, G


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def fmt(s, unit="ms"):
    return f"{s['median']:.2f} [{s['min']:.2f}, {s['max']:.2f}] {unit}"


def bench_volume(pkg, name, n_states, do_fit):
    eng = pkg.engine
    CorrespondenceModel = pkg.correspondence.CorrespondenceModel
    g = pkg.workloads.workload_geometry(name)
    shape = g.materials.shape
    n = int(np.prod(shape))
    K = 2
    out = {"volume": name, "shape": list(shape), "voxels": n, "K": K}
    F, G = motion_fields(shape)
    s10, ds10 = breathing(10)
    model = CorrespondenceModel()
    model.coefficients = np.stack([F.reshape(-1), G.reshape(-1)], axis=1).astype(np.float64)
    model.mean_signal = np.array([[s10.mean()], [ds10.mean()]])
    model.mean_vector_field = (F * np.float32(s10.mean())).reshape(-1, 1)
    model.timesteps, model.signal_n_dims, model.spatial_shape, model.reference_phase = 10, K, tuple(shape), 2
    model.signals = np.stack([s10, ds10])
    sn, dsn = breathing(n_states + 1)
    signals = np.stack([sn, dsn], axis=1)
    with tempfile.TemporaryDirectory() as tmp:
        sim = pkg.simulation.MCSimulation(pkg.geometry.MCAirGeometry(), pkg.workloads.material_files(), pkg.workloads.spectrum_file(),
                                          n_histories=100_000, n_projections=1)
        ctx = eng.create(str(sim.prepare_simulation(Path(tmp))), device=0)
        try:
            ctx.set_geometry(g)
            t0 = time.perf_counter()
            ctx.set_correspondence_model(model)
            out["upload_model_s"] = time.perf_counter() - t0
            out["resident_bytes"] = 3 * n * 4 + 3 * n * K * 8
            a = dict(wall=[], predict=[], copy=[], device=[], kernel=[])
            b = dict(wall=[], kernel=[])
            tables = {}
            for i, s in enumerate(signals):  # state 0 warms both routes up
                t0 = time.perf_counter()
                field = np.asarray(model.predict(s), dtype=np.float32)
                t1 = time.perf_counter()
                ctx.warp_geometry(field, frame="geometry")
                t2 = time.perf_counter()
                copy_ms = ctx.getf("warp_field_copy_ms")
                kernel_a = ctx.getf("warp_kernel_ms")
                t3 = time.perf_counter()
                ctx.warp_geometry_by_signal(s)
                t4 = time.perf_counter()
                kernel_b = ctx.getf("warp_kernel_ms")
                if i == 0:
                    continue
                a["wall"].append((t2 - t0) * 1e3); a["predict"].append((t1 - t0) * 1e3); a["copy"].append(copy_ms)
                a["device"].append((t2 - t1) * 1e3 - copy_ms); a["kernel"].append(kernel_a)
                b["wall"].append((t4 - t3) * 1e3); b["kernel"].append(kernel_b)
            # after the timed states (downloading the voxels builds a host table whose release the next state would pay for)
            ctx.warp_geometry(np.asarray(model.predict(signals[3]), dtype=np.float32), frame="geometry")
            tables["a"] = ctx.host_table("voxel_mat_dens")
            ctx.warp_geometry_by_signal(signals[3])
            tables["b"] = ctx.host_table("voxel_mat_dens")
            out["routes_equal"] = bool(np.array_equal(tables["a"], tables["b"]))
            out["host_field"] = {k: stats(v) for k, v in a.items()}
            out["resident"] = {k: stats(v) for k, v in b.items()}
            kernel_bytes = 3 * n * (4 + 8 * K) + n + n
            tbs = kernel_bytes / (out["resident"]["kernel"]["median"] * 1e-3) / 1e12
            out["resident"]["kernel_bytes"] = kernel_bytes
            out["resident"]["kernel_tb_per_s"] = tbs
            out["resident"]["fraction_of_hbm_peak"] = tbs / HBM_PEAK_TBS
            out["spread_ms"] = max(out["host_field"]["wall"]["max"] - out["host_field"]["wall"]["min"],
                                   out["resident"]["wall"]["max"] - out["resident"]["wall"]["min"])
            out["resident_not_slower"] = bool(out["resident"]["wall"]["median"] <= out["host_field"]["wall"]["median"] + out["spread_ms"])
            if do_fit:
                fields = np.stack([F * np.float32(s10[t]) + G * np.float32(ds10[t]) for t in range(10)])
                sig = np.stack([s10, ds10], axis=1)
                t0 = time.perf_counter()
                on_device = CorrespondenceModel().fit(fields, sig, ctx=ctx)
                t1 = time.perf_counter()
                on_host = CorrespondenceModel().fit(fields, sig)
                t2 = time.perf_counter()
                out["fit"] = dict(device_s=t1 - t0, host_s=t2 - t1,
                                  equal=bool(np.array_equal(on_device.coefficients, on_host.coefficients) and
                                             np.array_equal(on_device.mean_vector_field, on_host.mean_vector_field)))
        finally:
            ctx.close()
    return out


def table(results):
    lines = ["| volume | route | wall per state change | predict | field copy | rest (device + tables) | warp kernel | kernel bytes / time |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        a, b = r["host_field"], r["resident"]
        vol = f"{r['volume']} {'x'.join(map(str, r['shape']))}"
        lines.append(f"| {vol} | (a) host predict + field copy | {fmt(a['wall'])} | {fmt(a['predict'])} | {fmt(a['copy'])} | {fmt(a['device'])} | {fmt(a['kernel'])} | |")
        lines.append(f"| {vol} | (b) resident model | {fmt(b['wall'])} | | | | {fmt(b['kernel'])} | {b['kernel_bytes'] / 1e6:.0f} MB: {b['kernel_tb_per_s']:.2f} TB/s = "
                     f"{100 * b['fraction_of_hbm_peak']:.0f} % of {HBM_PEAK_TBS:.1f} TB/s ({100 * b['kernel_tb_per_s'] / HBM_ACHIEVABLE_TBS:.0f} % of the {HBM_ACHIEVABLE_TBS} TB/s a copy reaches) |")
    lines.append("")
    for r in results:
        lines.append(f"- {r['volume']}: median wall (a) / (b) = {r['host_field']['wall']['median'] / r['resident']['wall']['median']:.1f}; run-to-run spread "
                     f"{r['spread_ms']:.2f} ms; (b) not slower than (a) beyond the spread: {r['resident_not_slower']}; both routes give the same voxels: "
                     f"{r['routes_equal']}; model resident: {r['resident_bytes'] / 1e9:.2f} GB, uploaded in {r['upload_model_s']:.2f} s")
        if "fit" in r:
            f = r["fit"]
            lines.append(f"- {r['volume']}: fit of T = 10 fields, wall with upload: device {f['device_s']:.2f} s, host numpy {f['host_s']:.2f} s; bit-equal: {f['equal']}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", default="cirs,thorax")
    ap.add_argument("--fit", default="cirs", help="volumes whose fit is timed too (ten whole fields on the host: 8 GB for the thorax)")
    ap.add_argument("--states", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.engine.load_library()
    fit = set(filter(None, args.fit.split(",")))
    results = []
    for name in filter(None, args.volumes.split(",")):
        results.append(bench_volume(pkg, name, args.states, name in fit))
        print(table(results[-1:]), flush=True)
    text = table(results)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
