"""SHA-256 of what the two trainers return on the tests' small cases, as one JSON object: run it once per library (MCGPU_AMD_LIB)
in one session on one box and compare the two objects key for key.  The cases are the tests' own builders (tests/ goes on the path):
  speedup gradient <case>  the flat gradient of every entry of test_speedup_train_gpu.GRADIENT_CASES
  speedup state / predict  weights, both moments, step counts and lr after 3 mean and 2 variance updates of (2,2,8)/(1,2,8) at
                           32 x 48 with batch 2 (the tests' fixed batch), and predict on the same
  segment gradient <case>  the flat gradient and the ten metrics of L2_8x8x8 and L4_16x16x32 of test_segment_train_gpu
  segment state / predict  weights, both moments and the step count after 3 updates of L2_8x8x8, and predict on the same
  <net> stage <operator>   conv_wgrad, conv_dgrad and maxpool_backward of both stage entry points on float data: (5, 3) -> 7 at
                           33 x 70 and (4, 6) -> 4 at 4 x 10 x 66, the second source upsampled; the 3-D max-pool with and without
                           an initial dx
  <net> run / norm         the inference entry points, whose objects hold their own copy of the instance norm: MCSpeedup.predict
                           on test_speedup_gpu's 1 x 32 x 32 case, MCSegmenter.segment on test_segmentation_gpu's "unequal" net, and
                           the norm_lrelu stage of both on their tests' "segments" input
Usage: [MCGPU_AMD_LIB=other.so] python tools/train_digest.py [--out FILE.json]"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401 -- the tests' builders need it, and before the engine library brings up HIP (tests/conftest.py has the reason)

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from __graft_entry__ import load_package  # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def flat(named):
    return np.concatenate([v.ravel() for v in named.values()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.engine.load_library()
    import test_segment_train_gpu as G
    import test_speedup_train_gpu as S
    out = {}

    for name in S.GRADIENT_CASES:
        c = S._gradient_case(name)
        trainer = S.training.MCSpeedupTrainer(weights=c["weights"], mean_net=c["nets"][0], var_net=c["nets"][1])
        out[f"speedup gradient {name}"] = sha(flat(trainer.gradients(c["data"], phase=c["phase"])))
        trainer.close()
    data = S._fixed_batch()
    trainer = S.training.MCSpeedupTrainer(seed=3, n_pretrain_steps=3, mean_net=(2, 2, 8), var_net=(1, 2, 8))
    for _ in range(5):
        trainer.train_on_batch(data)
    out["speedup predict"] = sha(*trainer.predict(data["low_photon"], data["forward_projection"]))
    trainer.close()
    out["speedup state"] = sha(trainer._flat, trainer._moment1, trainer._moment2, np.asarray(trainer._steps, np.int64), np.float64(trainer._lr))

    for name in ("L2_8x8x8", "L4_16x16x32"):
        c = G._gradient_case(name)
        trainer = G.training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"], lr=1e-3)
        out[f"segment gradient {name}"] = sha(flat(trainer.gradients(c["data"])))
        metrics = trainer.validate_on_batch(c["data"])
        out[f"segment metrics {name}"] = sha(np.asarray([metrics[k] for k in G.training.METRICS], np.float64))
        if name == "L2_8x8x8":
            for _ in range(3):
                trainer.train_on_batch(c["data"])
            out["segment predict"] = sha(trainer.predict(c["data"]))
            trainer.close()
            out["segment state"] = sha(trainer._flat, trainer._moment1, trainer._moment2, np.int64(trainer.i_step))
        trainer.close()

    x1, x2, w, dy, _ = S._conv_case(np.random.default_rng(1), 5, 3, 7, 33, 70, integers=False)
    out["speedup stage conv_wgrad"] = sha(*S.stage("conv_wgrad", x1, in2=x2, in3=dy, upsample=True)[0][:2])
    out["speedup stage conv_dgrad"] = sha(*S.stage("conv_dgrad", dy, in2=w, c_out=5, upsample=True)[0])
    out["speedup stage maxpool_backward"] = sha(S.stage("maxpool_backward", x1, in2=dy[:5, :16, :35])[0])
    x1, x2, w, dy = G._conv_case(np.random.default_rng(2), 4, 6, 4, (4, 10, 66), integers=False)
    out["segment stage conv_wgrad"] = sha(*G.stage("conv_wgrad", x1, in2=x2, in3=dy, upsample=True)[0][:2])
    out["segment stage conv_dgrad"] = sha(*G.stage("conv_dgrad", dy, in2=w, c1=4, upsample=True)[0])
    out["segment stage maxpool_backward"] = sha(G.stage("maxpool_backward", x1, in2=dy[:, :2, :5, :33])[0])
    out["segment stage maxpool_backward onto dx"] = sha(G.stage("maxpool_backward", x1, in2=dy[:, :2, :5, :33], in3=dy)[0])

    import test_segmentation_gpu as N3
    import test_speedup_gpu as N2
    lp, fp = N2.speedup_ref.seeded_inputs(7, *N2.NETWORK_SHAPES[0])
    out["speedup run"] = sha(*N2.speedup.MCSpeedup(N2.speedup_ref.seeded_weights(7)).predict(lp, fp))
    out["speedup norm"] = sha(N2.speedup.speedup_stage("norm_lrelu", N2._norm_inputs()["segments"])[0])
    filters, levels = N3.NETWORKS["unequal"]
    model = N3.seg.MCSegmenter(N3.segment_ref.seeded_weights(7, filters, levels), patch_shape=N3.PATCH)
    out["segment run"] = sha(*model.segment(N3.segment_ref.seeded_image(7, N3.PATCH)))
    out["segment norm"] = sha(N3.seg.segment_stage("norm_lrelu", N3._norm_inputs()["segments"])[0])

    print(json.dumps(out, sort_keys=True))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
