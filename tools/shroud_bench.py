"""Time stage A of the projection-derived breathing signal (csrc/shroud.hip: row_sums + combine) at the reference's size, 894
projections of 1024 x 768 pixels (2.8 GB of float32), with the stack resident on the device, against the same rule composed from
torch operations on the same tensor: the central difference of the rows (one float32 subtraction per pixel), then sum(-1) in float64,
which reads the stack at least twice and writes and reads the difference as well.

Prints for both the median ms over --repeats runs after --warmup runs, the fused kernel's GB/s over the bytes of the stack, and the
largest difference of the two results; writes profiles/shroud.md unless --no-write.  Final line: JSON.
Usage: python tools/shroud_bench.py [--n-proj 894] [--repeats 10] [--warmup 2]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402  -- before the engine brings up HIP

from __graft_entry__ import load_package  # noqa: E402


def composed(stack):
    """D [n, nv] float64 by torch: t = P[v + 1] - P[v - 1] with clamped rows in float32, 0.5 * sum over u in float64."""
    nv = stack.shape[1]
    v = torch.arange(nv, device=stack.device)
    t = stack[:, torch.clamp(v + 1, max=nv - 1)] - stack[:, torch.clamp(v - 1, min=0)]
    return 0.5 * t.sum(-1, dtype=torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-proj", type=int, default=894)
    ap.add_argument("--nv", type=int, default=768)
    ap.add_argument("--nu", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    shroud = pkg.shroud
    engine, lib = shroud._library()
    n, nv, nu = args.n_proj, args.nv, args.nu
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    stack = torch.rand((n, nv, nu), device=dev, dtype=torch.float32, generator=gen) * 4.0
    rows = torch.empty((n, nv), device=dev, dtype=torch.float64)
    o = shroud._ShroudOptions(C.sizeof(shroud._ShroudOptions), n_proj=n, nu=nu, nv=nv, device=0)
    rep = shroud._ShroudReport(C.sizeof(shroud._ShroudReport))
    torch.cuda.synchronize()
    fused_ms = []
    for i in range(args.warmup + args.repeats):
        engine._check(lib.mcgpu_shroud_rows_device(C.byref(o), stack.data_ptr(), rows.data_ptr(), C.byref(rep)))
        if i >= args.warmup:
            fused_ms.append(rep.ms_shroud)
    torch_ms, want = [], None
    for i in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        want = composed(stack)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            torch_ms.append(e0.elapsed_time(e1))
    difference = float((rows - want).abs().max())
    scale = float(want.abs().max())
    nbytes = stack.numel() * 4
    fused, torch_med = statistics.median(fused_ms), statistics.median(torch_ms)
    res = dict(n_proj=n, nv=nv, nu=nu, stack_gb=nbytes / 1e9, repeats=args.repeats, fused_ms_median=fused, fused_ms_min=min(fused_ms), fused_ms_max=max(fused_ms),
               fused_gb_per_s=nbytes / (fused * 1e-3) / 1e9, torch_ms_median=torch_med, torch_ms_min=min(torch_ms), torch_ms_max=max(torch_ms),
               torch_over_fused=torch_med / fused, max_abs_difference=difference, max_abs_value=scale, device=torch.cuda.get_device_name(0))
    print(f"fused   : {fused:.3f} ms (min {min(fused_ms):.3f}, max {max(fused_ms):.3f}), {res['fused_gb_per_s']:.0f} GB/s over {nbytes / 1e9:.2f} GB", flush=True)
    print(f"torch   : {torch_med:.3f} ms (min {min(torch_ms):.3f}, max {max(torch_ms):.3f}), {torch_med / fused:.1f} x the fused kernel", flush=True)
    print(f"results : differ by at most {difference:.3g} at values up to {scale:.3g}", flush=True)
    if not args.no_write:
        out = ROOT / "profiles" / "shroud.md"
        out.write_text(
            "# Stage A of the Amsterdam shroud: the fused kernel against the rule composed from torch operations\n\n"
            f"`python tools/shroud_bench.py --n-proj {n} --nv {nv} --nu {nu} --repeats {args.repeats} --warmup {args.warmup}` on {res['device']}, the stack "
            f"({nbytes / 1e9:.2f} GB of float32) resident on the device; medians over {args.repeats} runs (min .. max).\n\n"
            "| what | ms | GB/s over the stack's bytes |\n|---|---|---|\n"
            f"| `row_sums` + `combine` (csrc/shroud.hip, device events around the launches) | {fused:.3f} ({min(fused_ms):.3f} .. {max(fused_ms):.3f}) | {res['fused_gb_per_s']:.0f} |\n"
            f"| torch: clamped central difference in float32, `sum(-1, dtype=float64)` | {torch_med:.3f} ({min(torch_ms):.3f} .. {max(torch_ms):.3f}) | "
            f"{nbytes / (torch_med * 1e-3) / 1e9:.0f} |\n\n"
            f"The composition takes {torch_med / fused:.1f} x the fused kernel's time.  The two results differ by at most {difference:.3g} at values up to {scale:.3g}.\n"
            "The GB/s figure divides the bytes of the stack, each counted once, by the time: the 2 rows around every band of 32 that a neighbouring "
            "workgroup reads again are not counted.\n")
        print(f"wrote {out}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
