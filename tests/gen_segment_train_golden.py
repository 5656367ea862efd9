"""Regenerate the fixture that chains tests/segment_train_ref.py to the reference's own Dice loss:

  tests/golden/segment_train_pin.npz   one 8 x 8 x 8 case: float64 logits [1, 9, 8, 8, 8], the uint8 target, the reference class's
                                       f [1, 9] and its autograd gradient of mean(f) with respect to the logits

Usage: python tests/gen_segment_train_golden.py <reference tree>.  cbctmc/segmentation/losses.py is loaded from its file at run time
(it needs only torch); nothing of it is kept.  The three lines of the driver's SegmentationLoss (softmax over channels 0 .. 7,
sigmoid on channel 8, then DiceLoss(include_background=True, reduction="none")) live in a script that cannot be imported; they are
restated here and in the test.  Label 5 is absent from the target, and channel 8 overlaps label 6."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

PIN_SEED, PIN_SHAPE = 11, (8, 8, 8)


def reference_dice(reference_tree):
    spec = importlib.util.spec_from_file_location("reference_losses", Path(reference_tree) / "cbctmc" / "segmentation" / "losses.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.DiceLoss(include_background=True, reduction="none")


def pin_inputs():
    import segment_train_ref
    rng = np.random.default_rng(PIN_SEED)
    logits = rng.normal(0.0, 2.0, size=(1, 9) + PIN_SHAPE)
    target = segment_train_ref.seeded_target(PIN_SEED, PIN_SHAPE)[None]
    return logits, target


def main(reference_tree):
    logits, target = pin_inputs()
    z = torch.as_tensor(logits, dtype=torch.float64).requires_grad_(True)
    p = torch.cat([torch.softmax(z[:, 0:-1], dim=1), torch.sigmoid(z[:, -1:])], dim=1)  # the driver's two activations
    f = reference_dice(reference_tree)(input=p, target=torch.as_tensor(target, dtype=torch.float64))
    f.mean().backward()
    f = f.detach().numpy().reshape(1, 9)
    np.savez_compressed(HERE / "golden" / "segment_train_pin.npz", logits=logits, target=target, f=f, gradient=z.grad.numpy())
    print("f", f.round(6), "absent labels", [c for c in range(9) if not target[0, c].any()], "overlap of 8 and 6", int((target[0, 8] & target[0, 6]).sum()))


if __name__ == "__main__":
    main(Path(sys.argv[1]))
