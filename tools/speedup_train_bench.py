"""Time one training step of the speed-up network (csrc/speedup_train.hip) at 1024 x 768 with the reference's batch of 10, golden
architecture, seeded initialisation.

Prints one line per measurement and a final JSON line:
  engine : per-stage ms of mcgpu_speedup_train_step's report for both phases (medians of `--repeat` steps after a warm-up step, all
           in one process) and the peak of the device memory
  torch  : the float32 restatement (tests/speedup_train_ref.py: autograd of tests/speedup_ref.py, torch.optim.Adam) through torch on
           the same GPU, weights and batch resident on the device, samples one at a time as the engine runs them
Usage: python tools/speedup_train_bench.py [--nu 1024] [--nv 768] [--batch 10] [--repeat 3] [--skip-torch]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=768)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    pkg = load_package()
    training = pkg.speedup_training
    pkg.engine.load_library()
    import speedup_ref
    lp, fp = speedup_ref.seeded_inputs(4, args.batch, args.nv, args.nu)
    t = (lp + np.random.default_rng(5).normal(0.0, 0.3, size=lp.shape)).astype(np.float32)
    data = {"low_photon": lp, "forward_projection": fp, "high_photon": t}
    result = {"nu": args.nu, "nv": args.nv, "batch": args.batch}

    for phase, pretrain in (("mean", 10 ** 9), ("variance", 0)):
        trainer = training.MCSpeedupTrainer(seed=0, n_pretrain_steps=pretrain)
        trainer.train_on_batch(data)  # code objects, allocator
        reports = []
        for _ in range(args.repeat):
            trainer.train_on_batch(data)
            reports.append(dict(trainer.last_report))
        trainer.close()
        row = {k: statistics.median(r[k] for r in reports) for k in STAGES}
        row["peak_device_bytes"] = reports[-1]["peak_device_bytes"]
        result[phase] = row
        print(f"engine : phase {phase:8s} " + ", ".join(f"{k[3:]} {row[k]:.1f}" for k in STAGES) + f" ms; peak {row['peak_device_bytes'] / 2 ** 20:.0f} MiB",
              flush=True)

    if not args.skip_torch:
        if torch is None or not torch.cuda.is_available():
            raise SystemExit("torch sees no GPU: run with --skip-torch")
        import speedup_train_ref as ref
        w0 = training.initial_weights(0)
        w = {k: torch.as_tensor(v, device="cuda").clone().requires_grad_(True) for k, v in w0.items()}
        dev = {k: torch.as_tensor(v[:, None], device="cuda") for k, v in data.items()}
        N = float(lp.size)
        result["torch"] = {}
        for phase, prefix in (("mean", "mean_net"), ("variance", "var_net")):
            for k, v in w.items():  # the other net is frozen, as the reference freezes it: no graph is kept for it
                v.requires_grad_(k.startswith(prefix))
            opt = torch.optim.Adam([v for k, v in w.items() if k.startswith(prefix)], lr=1e-3)
            times = []
            try:
                for _ in range(args.repeat + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    opt.zero_grad(set_to_none=True)
                    for p in range(args.batch):
                        _, m, _, v = ref.forward(w, dev["low_photon"][p:p + 1], dev["forward_projection"][p:p + 1])
                        tt = dev["high_photon"][p:p + 1]
                        if phase == "mean":
                            loss = torch.nn.functional.l1_loss(m, tt, reduction="sum") / N
                        else:
                            loss = torch.nn.functional.gaussian_nll_loss(m.detach(), tt, v, reduction="sum") / N
                        loss.backward()
                    opt.step()
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
            except RuntimeError as e:  # out of memory, an operator without a device kernel: said, not hidden
                result["torch"][phase] = {"error": str(e).splitlines()[0]}
                print(f"torch  : phase {phase:8s} could not run: {result['torch'][phase]['error']}", flush=True)
                continue
            result["torch"][phase] = {"ms_step": statistics.median(times[1:]), "ms_runs": times,
                                      "peak_device_bytes": int(torch.cuda.max_memory_allocated())}
            print(f"torch  : phase {phase:8s} step {statistics.median(times[1:]):.1f} ms (runs {', '.join(f'{x:.1f}' for x in times)}); "
                  f"peak {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
