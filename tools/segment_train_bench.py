"""Time one training step of the segmentation network (csrc/segment_train.hip) at the reference driver's patch, 384 x 384 x 64 with
a batch of 1, the reference's filters, seeded initialisation.

Prints one line per measurement and a final JSON line:
  engine : per-stage ms of mcgpu_segment_train_step's report (medians of `--repeat` steps after a warm-up step, all in one process),
           the peak of the device memory and the dry plan
  torch  : the float32 restatement (tests/segment_train_ref.py: autograd of tests/segment_ref.py: unet, torch.optim.Adam) through
           torch on the same GPU, weights and patch resident on the device
Usage: python tools/segment_train_bench.py [--patch 384 384 64] [--repeat 3] [--skip-torch]"""
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

STAGES = ("ms_forward", "ms_wgrad", "ms_dgrad", "ms_norm", "ms_optimizer", "ms_total")


def fixed_patch(shape):
    """A rescaled patch of eight tissue blocks with noise and its target; label 6 carries the vessel overlay."""
    rng = np.random.default_rng(0)
    z, y, x = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    field = ((z // max(shape[0] // 8, 1)) + 2 * (y // max(shape[1] // 6, 1)) + (x // max(shape[2] // 4, 1))) % 8
    image = (0.1 * field + 0.05 * rng.random(shape, dtype=np.float32)).astype(np.float32)
    target = np.zeros((9,) + tuple(shape), np.uint8)
    for c in range(8):
        target[c] = field == c
    target[8] = (field == 6) & ((z + y + x) % 3 == 0)
    return image, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, nargs=3, default=(384, 384, 64))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    shape = tuple(args.patch)
    pkg = load_package()
    training = pkg.segmentation_training
    pkg.engine.load_library()
    image, target = fixed_patch(shape)
    data = {"image": image[None, None], "segmentation": target[None]}
    result = {"patch": list(shape), "batch": 1}

    trainer = training.CTSegmentationTrainer(seed=0)
    planned = trainer.planned_device_bytes(1, shape)
    trainer.train_on_batch(data)  # code objects, allocator
    reports, losses = [], []
    for _ in range(args.repeat):
        losses.append(trainer.train_on_batch(data)["loss"])
        reports.append(dict(trainer.last_report))
    trainer.close()
    row = {k: statistics.median(r[k] for r in reports) for k in STAGES}
    row.update(peak_device_bytes=reports[-1]["peak_device_bytes"], planned_device_bytes=planned, losses=losses)
    result["engine"] = row
    print("engine : " + ", ".join(f"{k[3:]} {row[k]:.1f}" for k in STAGES) + f" ms; peak {row['peak_device_bytes'] / 2 ** 20:.0f} MiB "
          f"(planned {planned / 2 ** 20:.0f} MiB); wgrad is {100.0 * row['ms_wgrad'] / row['ms_total']:.0f} % of the step", flush=True)

    if not args.skip_torch:
        if torch is None or not torch.cuda.is_available():
            raise SystemExit("torch sees no GPU: run with --skip-torch")
        import segment_ref
        import segment_train_ref as ref
        w = {k: torch.as_tensor(v, device="cuda").clone().requires_grad_(True) for k, v in training.initial_weights(0).items()}
        x = torch.as_tensor(image[None, None], device="cuda")
        t = torch.as_tensor(target[None], device="cuda").float()
        opt = torch.optim.Adam(list(w.values()), lr=1e-4)
        times = []
        try:
            for _ in range(args.repeat + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                opt.zero_grad(set_to_none=True)
                ref.loss_of(segment_ref.unet(x, w), t).backward()
                opt.step()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
                print(f"torch  : run {len(times)} took {times[-1]:.1f} ms", flush=True)  # the first one holds the library's search for kernels
            result["torch"] = {"ms_step": statistics.median(times[1:]), "ms_runs": times, "peak_device_bytes": int(torch.cuda.max_memory_allocated())}
            print(f"torch  : step {statistics.median(times[1:]):.1f} ms (runs {', '.join(f'{v:.1f}' for v in times)}); "
                  f"peak {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB", flush=True)
        except RuntimeError as e:  # out of memory, an operator without a device kernel: said, not hidden
            result["torch"] = {"error": str(e).splitlines()[0]}
            print(f"torch  : could not run: {result['torch']['error']}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
