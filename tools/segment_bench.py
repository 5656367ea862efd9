"""Time the segmentation network (csrc/segment_net.hip) with seeded weights (tests/segment_ref.py: seeded_weights(7), L = 4, 32
filters; the reference ships no trained ones) and write the tables of profiles/segment_ab.md.

  layers : every convolution of the network at one patch (default 128^3) alone, mcgpu_segment_stage CONV on random data of the
           layer's shape: ms, TFLOP/s of the useful arithmetic 2 x 27 C_in C_out voxels and its share of the 155 TFLOP/s
           float32-MFMA peak; interleaved with torch's float32 Conv3d and the same Conv3d under autocast (what the reference runs)
           on the same GPU and weights, best of three after a warm-up each
  patch  : the whole network on one patch: this engine's report against the float32 restatement (tests/segment_ref.py) through
           torch, in float32 and under autocast
  volume : MCSegmenter.segment on a whole volume (default 512 x 512 x 96)
Usage: python tools/segment_bench.py [--patch 128 128 128] [--volume 512 512 96] [--out profiles/segment_ab.md] [--skip-torch]"""
from __future__ import annotations

import argparse
import json
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
FILTERS, LEVELS = (32,) * 10, 4


def network_layers(patch, filters=FILTERS, levels=LEVELS):
    """(name, c1, c2 (read through the upsample), c_out, shape) of every convolution, in the order of the forward pass."""
    f = list(filters)
    skip = f[:levels + 1]
    at = lambda i: tuple(p >> i for p in patch)  # noqa: E731
    out = [("init_conv", 1, 0, f[0], at(0))]
    for i in range(levels):
        out += [(f"enc_{i}.convs.0", skip[i], 0, skip[i + 1], at(i + 1)), (f"enc_{i}.convs.3", skip[i + 1], 0, skip[i + 1], at(i + 1))]
    below = skip[levels]
    for j, i in enumerate(reversed(range(levels))):
        c = f[levels + 1 + j]
        out += [(f"dec_{i}.convs.0", skip[i], below, c, at(i)), (f"dec_{i}.convs.3", c, 0, c, at(i))]
        below = c
    return out + [("final_conv", f[-1], 0, 9, at(0))]


def torch_ms(fn, repeats=3):
    """Best of `repeats` after one warm-up, by device events."""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--volume", type=int, nargs=3, default=[512, 512, 96])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_ab.md"))
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not args.skip_torch and (torch is None or not torch.cuda.is_available()):
        raise SystemExit("torch sees no GPU: run with --skip-torch")
    pkg = load_package()
    seg = pkg.segmentation
    pkg.engine.load_library()
    import segment_ref
    import torch.nn.functional as F
    patch = tuple(args.patch)
    weights = segment_ref.seeded_weights(7, FILTERS, LEVELS)
    rng = np.random.default_rng(0)
    result = {"patch": patch, "volume": tuple(args.volume)}
    md = [f"# The segmentation network at one {' x '.join(map(str, patch))} patch: HIP kernels, per layer, against torch on the same GPU", "",
          "Written by `python tools/segment_bench.py` on one MI355X; the remarks at the end are by hand.  Weights: `tests/segment_ref.py:",
          "seeded_weights(7)`, L = 4, 32 filters (the reference ships no trained ones; the time does not depend on the values).  Per-layer",
          "times of the HIP path are `mcgpu_segment_stage` CONV on random data of the layer's shape (HIP events around the kernel); torch is",
          "`F.conv3d` on the materialised (concatenated, upsampled) input with resident tensors, in float32 and under `torch.autocast` (float16:",
          "what the reference runs), by device events.  All three interleaved per layer, best of three after one warm-up each.  FLOP are the",
          "useful ones, 2 x 27 C_in C_out voxels; the peak is the 155 TFLOP/s measured for `v_mfma_f32_32x32x2_f32` on this part.", "",
          "## Per convolution layer", "",
          "| layer | C_in -> C_out | shape | ms | GFLOP | TFLOP/s | of peak | torch float32 ms | torch autocast ms |", "|---|---|---|---|---|---|---|---|---|"]
    rows, total = [], dict(ms=0.0, flop=0.0, t32=0.0, t16=0.0)
    for name, c1, c2, c_out, shape in network_layers(patch):
        x1 = rng.normal(size=(c1,) + shape).astype(np.float32)
        x2 = rng.normal(size=(c2,) + tuple(d // 2 for d in shape)).astype(np.float32) if c2 else None
        w = rng.normal(size=(c_out, c1 + c2, 3, 3, 3)).astype(np.float32)
        b = rng.normal(size=(c_out,)).astype(np.float32)
        ours = lambda: seg.segment_stage("conv", x1, in2=x2, weight=w, bias=b, upsample=bool(c2))[1]["ms_conv"]  # noqa: E731
        ours()
        t32 = t16 = float("nan") if args.skip_torch else float("inf")
        if not args.skip_torch:
            x = torch.as_tensor(x1, device="cuda")[None]
            if c2:
                x = torch.cat([x, F.interpolate(torch.as_tensor(x2, device="cuda")[None], scale_factor=2, mode="nearest")], dim=1)
            wt, bt = torch.as_tensor(w, device="cuda"), torch.as_tensor(b, device="cuda")

            def conv16():
                with torch.autocast("cuda"):
                    return F.conv3d(x, wt, bt, padding=1)
        ms = float("inf")
        for _ in range(3):
            ms = min(ms, ours())
            if not args.skip_torch:
                t32 = min(t32, torch_ms(lambda: F.conv3d(x, wt, bt, padding=1), 1))
                t16 = min(t16, torch_ms(conv16, 1))
        flop = 2.0 * 27 * (c1 + c2) * c_out * float(np.prod(shape))
        rows.append(dict(layer=name, c_in=c1 + c2, c_out=c_out, shape=shape, ms=ms, gflop=flop / 1e9, tflops=flop / ms / 1e9, torch_f32_ms=t32,
                         torch_autocast_ms=t16))
        for key, v in (("ms", ms), ("flop", flop), ("t32", t32), ("t16", t16)):
            total[key] += v
        line = (f"| `{name}` | {c1 + c2} -> {c_out} | {' x '.join(map(str, shape))} | {ms:.3f} | {flop / 1e9:.1f} | {flop / ms / 1e9:.1f} | "
                f"{100 * flop / ms / 1e9 / PEAK_TFLOPS:.1f} % | {t32:.3f} | {t16:.3f} |")
        md.append(line)
        print(line, flush=True)
        del x1, x2
    md.append(f"| all | | | {total['ms']:.2f} | {total['flop'] / 1e9:.0f} | {total['flop'] / total['ms'] / 1e9:.1f} | "
              f"{100 * total['flop'] / total['ms'] / 1e9 / PEAK_TFLOPS:.1f} % | {total['t32']:.2f} | {total['t16']:.2f} |")
    print(md[-1], flush=True)
    result["layers"], result["layers_total"] = rows, total

    # the whole network on one patch
    image = segment_ref.seeded_image(7, patch)
    model = seg.MCSegmenter(weights, patch_shape=patch)
    model.segment(image)
    runs = []
    for _ in range(3):
        labels, raw = model.segment(image)
        runs.append(dict(model.last_report))
    one = min(runs, key=lambda r: r["ms_total"])
    result["one_patch"] = one
    md += ["", "## One patch through the whole call", "",
           "| | ms_upload | ms_conv | ms_norm | ms_other | kernels | ms_total | patches run / skipped | peak device memory |", "|---|---|---|---|---|---|---|---|---|",
           f"| `segment` on one patch | {one['ms_upload']:.2f} | {one['ms_conv']:.2f} | {one['ms_norm']:.2f} | {one['ms_other']:.2f} | "
           f"{one['ms_conv'] + one['ms_norm'] + one['ms_other']:.2f} | {one['ms_total']:.2f} | {one['patches_run']} / {one['patches_skipped']} | "
           f"{one['peak_device_bytes']} B = {one['peak_device_bytes'] / 2 ** 20:.0f} MiB |"]
    print(md[-1], flush=True)
    if not args.skip_torch:
        w_dev = {k: torch.as_tensor(v, device="cuda") for k, v in weights.items()}
        x = torch.as_tensor(segment_ref.rescale(image)[None, None], device="cuda")
        with torch.no_grad():
            f32 = torch_ms(lambda: segment_ref.head(segment_ref.unet(x, w_dev)))
            p32 = segment_ref.head(segment_ref.unet(x, w_dev))[0].cpu().numpy()

            def net16():
                with torch.autocast("cuda"):
                    return segment_ref.head(segment_ref.unet(x, w_dev).float())
            f16 = torch_ms(net16)
            p16 = net16()[0].float().cpu().numpy()
        ours = one["ms_conv"] + one["ms_norm"] + one["ms_other"]
        result["torch_patch"] = dict(ms_float32=f32, ms_autocast=f16, max_abs_difference_float32=float(np.abs(p32 - raw).max()),
                                     max_abs_difference_autocast=float(np.abs(p16 - raw).max()))
        md += ["", f"The float32 restatement through torch on the same GPU (resident weights and input, device events, best of three): "
               f"**{f32:.2f} ms**; under autocast **{f16:.2f} ms**; this engine's kernels **{ours:.2f} ms** (torch float32 / engine = {f32 / ours:.2f}, "
               f"torch autocast / engine = {f16 / ours:.2f}).  Largest difference of the probabilities: {np.abs(p32 - raw).max():.3g} against torch "
               f"float32, {np.abs(p16 - raw).max():.3g} against torch autocast."]
        print(md[-1], flush=True)
        del w_dev, x
        torch.cuda.empty_cache()

    # a whole volume
    volume = segment_ref.seeded_image(5, tuple(args.volume))
    t0 = time.perf_counter()
    model.segment(volume)
    wall = time.perf_counter() - t0
    rep = dict(model.last_report)
    result["volume_report"] = dict(rep, s_wall=wall)
    md += ["", f"## `segment` on a {' x '.join(map(str, args.volume))} volume", "",
           "| ms_upload | ms_conv | ms_norm | ms_other | ms_total | wall s | patches run / skipped | peak device memory |", "|---|---|---|---|---|---|---|---|",
           f"| {rep['ms_upload']:.1f} | {rep['ms_conv']:.1f} | {rep['ms_norm']:.1f} | {rep['ms_other']:.1f} | {rep['ms_total']:.1f} | {wall:.2f} | "
           f"{rep['patches_run']} / {rep['patches_skipped']} | {rep['peak_device_bytes']} B = {rep['peak_device_bytes'] / 2 ** 20:.0f} MiB |"]
    print(md[-1], flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(md) + "\n")
    print(json.dumps(result, default=list))


if __name__ == "__main__":
    main()
