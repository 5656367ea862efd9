"""Time the speed-up network (csrc/speedup_net.hip) on one 1024 x 768 projection with seeded weights (tests/speedup_ref.py:
seeded_weights(7); the reference ships no trained ones).

Prints one line per measurement and a final JSON line:
  network  : mcgpu_speedup_run on one projection and on a stack (per-stage ms of the report, ms per projection)
  layers   : every convolution of the two nets alone (mcgpu_speedup_stage CONV on random data of the layer's shape): ms, TFLOP/s
             of the useful arithmetic 2 x 9 C_in C_out H W, and its share of the 155 TFLOP/s float32-MFMA peak measured on the MI355X
  torch    : the float32 restatement (tests/speedup_ref.py) through torch on the same GPU -- what a user of the reference gets from
             PyTorch-ROCm -- and the largest difference between the two results
Usage: python tools/speedup_bench.py [--nu 1024] [--nv 768] [--stack 8] [--skip-layers] [--skip-torch]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

try:  # before the engine library brings up HIP (tests/conftest.py has the reason)
    import torch
except Exception:  # noqa: BLE001
    torch = None

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

PEAK_TFLOPS = 155.0


def network_layers(nu, nv):
    """(name, c1, c2 (read through the upsample), c_out, H, W) of every convolution, in the order of the forward pass."""
    out = []
    for prefix, (c_in, levels, base) in (("mean_net", (2, 4, 64)), ("var_net", (1, 2, 16))):
        out.append((f"{prefix}.init_conv", c_in, 0, base, nv, nu))
        for i in range(levels):
            c_prev, c = (base << (i - 1) if i else base), base << i
            out.append((f"{prefix}.enc_{i}.convs.0", c_prev, 0, c, nv >> (i + 1), nu >> (i + 1)))
            out.append((f"{prefix}.enc_{i}.convs.3", c, 0, c, nv >> (i + 1), nu >> (i + 1)))
        for i in reversed(range(levels)):
            skip, below, c = (base << (i - 1) if i else base), base << (levels - 1 if i == levels - 1 else i + 1), base << i
            out.append((f"{prefix}.dec_{i}.convs.0", skip, below, c, nv >> i, nu >> i))
            out.append((f"{prefix}.dec_{i}.convs.3", c, 0, c, nv >> i, nu >> i))
        out.append((f"{prefix}.final_conv", base, 0, 1, nv, nu))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=768)
    ap.add_argument("--stack", type=int, default=8)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    speedup = pkg.speedup
    pkg.engine.load_library()
    import speedup_ref
    weights = speedup_ref.seeded_weights(7)
    model = speedup.MCSpeedup(weights)
    lp, fp = speedup_ref.seeded_inputs(4, args.stack, args.nv, args.nu)
    result = {"nu": args.nu, "nv": args.nv}

    model.execute(lp[:1], fp[:1], seed=1)  # code objects, allocator
    runs = []
    for _ in range(3):
        mean, variance, _ = model.execute(lp[:1], fp[:1], seed=1)
        runs.append(dict(model.last_report))
    one = min(runs, key=lambda r: r["ms_total"])
    result["one_projection"] = one
    print("network : one projection  " + ", ".join(f"{k} {v:.2f}" for k, v in one.items() if k.startswith("ms_")) +
          f", peak {one['peak_device_bytes'] / 2 ** 20:.0f} MiB", flush=True)
    t0 = time.perf_counter()
    model.execute(lp, fp, seed=1)
    wall = time.perf_counter() - t0
    rep = dict(model.last_report)
    kernels = rep["ms_preprocess"] + rep["ms_conv"] + rep["ms_norm"] + rep["ms_other"]
    result["stack"] = dict(n=args.stack, s_wall=wall, ms_kernels_per_projection=kernels / args.stack, ms_total_per_projection=rep["ms_total"] / args.stack,
                           report=rep)
    print(f"network : stack of {args.stack}: kernels {kernels / args.stack:.2f} ms per projection, call {rep['ms_total'] / args.stack:.2f} ms per projection "
          f"(conv {rep['ms_conv'] / args.stack:.2f}, norm {rep['ms_norm'] / args.stack:.2f}, upload {rep['ms_upload'] / args.stack:.2f})", flush=True)

    if not args.skip_layers:
        rng = np.random.default_rng(0)
        rows, total_ms, total_flop = [], 0.0, 0.0
        for name, c1, c2, c_out, H, W in network_layers(args.nu, args.nv):
            x1 = rng.normal(size=(c1, H, W)).astype(np.float32)
            x2 = rng.normal(size=(c2, H // 2, W // 2)).astype(np.float32) if c2 else None
            w = rng.normal(size=(c_out, c1 + c2, 3, 3)).astype(np.float32)
            b = rng.normal(size=(c_out,)).astype(np.float32)
            ms = min(speedup.speedup_stage("conv", x1, in2=x2, weight=w, bias=b, upsample=bool(c2))[1]["ms_conv"] for _ in range(3))
            flop = 2.0 * 9 * (c1 + c2) * c_out * H * W
            rows.append(dict(layer=name, c_in=c1 + c2, c_out=c_out, H=H, W=W, ms=ms, gflop=flop / 1e9, tflops=flop / ms / 1e9,
                             share_of_peak=flop / ms / 1e9 / PEAK_TFLOPS))
            total_ms += ms
            total_flop += flop
            print(f"layer   : {name:26s} {c1 + c2:4d} -> {c_out:3d} at {W:4d} x {H:3d}: {ms:7.3f} ms, {flop / 1e9:7.1f} GFLOP, {flop / ms / 1e9:6.1f} TFLOP/s "
                  f"({100 * flop / ms / 1e9 / PEAK_TFLOPS:4.1f} % of peak)", flush=True)
        result["layers"] = rows
        result["layers_total"] = dict(ms=total_ms, gflop=total_flop / 1e9, tflops=total_flop / total_ms / 1e9)
        print(f"layers  : {total_ms:.2f} ms, {total_flop / 1e9:.0f} GFLOP, {total_flop / total_ms / 1e9:.1f} TFLOP/s", flush=True)

    if not args.skip_torch:
        if torch is None or not torch.cuda.is_available():
            raise SystemExit("torch sees no GPU: run with --skip-torch")
        times = []
        for k in range(4):  # the first run chooses the convolution algorithms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m32, v32 = speedup_ref.predict(weights, lp[:1], fp[:1], dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            print(f"torch   : run {k} with the weights sent per call: {times[-1]:.2f} ms", flush=True)
        w_dev = {k: torch.as_tensor(v, device="cuda") for k, v in weights.items() if k != "var_scale"}
        lp_t, fp_t = torch.as_tensor(lp[:1, None], device="cuda"), torch.as_tensor(fp[:1, None], device="cuda")
        resident = []
        with torch.no_grad():
            for k in range(5):  # weights and inputs resident on the device: the forward pass alone
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = torch.cat([lp_t, speedup_ref.preprocess(lp_t, fp_t)], dim=1)
                m = torch.relu(lp_t + 10.0 * torch.tanh(speedup_ref.unet(x, w_dev, "mean_net")))
                v = m * (0.10 * torch.sigmoid(speedup_ref.unet(m, w_dev, "var_net"))) + 1e-6
                torch.cuda.synchronize()
                resident.append((time.perf_counter() - t0) * 1e3)
        ms_torch = statistics.median(resident[1:])
        ours = one["ms_preprocess"] + one["ms_conv"] + one["ms_norm"] + one["ms_other"]
        result["torch"] = dict(ms_forward_resident=ms_torch, ms_runs=resident, ms_with_weight_upload=times,
                               max_abs_difference_mean=float(np.abs(m[0, 0].cpu().numpy() - mean[0]).max()),
                               max_abs_difference_variance=float(np.abs(v[0, 0].cpu().numpy() - variance[0]).max()),
                               ratio_torch_over_hip_kernels=ms_torch / ours)
        print(f"torch   : forward pass with resident weights {ms_torch:.2f} ms (runs {', '.join(f'{t:.2f}' for t in resident)}); this engine's kernels "
              f"{ours:.2f} ms: torch / engine = {ms_torch / ours:.2f}; largest difference mean {result['torch']['max_abs_difference_mean']:.3g}, "
              f"variance {result['torch']['max_abs_difference_variance']:.3g}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
