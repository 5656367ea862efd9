"""Regenerate the fixtures that chain tests/speedup_ref.py to the reference's own network class:

  tests/golden/speedup_state_dict.json   names and shapes of MCSpeedUpUNet(2, 2).state_dict(), in its order
  tests/golden/speedup_pin.npz           the reference class's float64 mean and variance for seeded_weights(7), 32 x 48 x 2

Usage: python tests/gen_speedup_golden.py <reference tree>.  The reference class is imported at run time; nothing of it is kept."""
from __future__ import annotations

import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

PIN_SEED, PIN_SHAPE = 7, (2, 32, 48)


def reference_predict(reference_tree, weights: dict, low_photon: np.ndarray, forward_projection, in_channels: int = 2):
    """(mean, variance) [n, nv, nu] float64 of the reference's MCSpeedUpUNet after MCSpeedup.preprocess_inputs' matching, one
    sample per call."""
    sys.path.insert(0, str(reference_tree))
    from cbctmc.speedup.models import MCSpeedUpUNet
    model = MCSpeedUpUNet(in_channels=in_channels, out_channels=2).double().eval()
    state = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in weights.items()}
    state.setdefault("var_scale", model.state_dict()["var_scale"])
    model.load_state_dict(state)
    means, variances = [], []
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):  # the class prints a diagnostic per call
        for p in range(low_photon.shape[0]):
            lp = torch.as_tensor(low_photon[p:p + 1, None], dtype=torch.float64)
            x = lp
            if forward_projection is not None:
                fp = torch.as_tensor(forward_projection[p:p + 1, None], dtype=torch.float64)
                d = dict(dim=(2, 3), keepdim=True)  # inference.py: preprocess_inputs, restated (that module imports itk)
                fp = (fp - torch.mean(fp, **d)) / torch.std(fp, **d) * torch.std(lp, **d) + torch.mean(lp, **d)
                x = torch.cat((lp, fp), dim=1)
            out = model(x)
            means.append(out[0, 0].numpy())
            variances.append(out[0, 1].numpy())
    return np.stack(means), np.stack(variances)


def main(reference_tree):
    sys.path.insert(0, str(reference_tree))
    from cbctmc.speedup.models import MCSpeedUpUNet
    state = MCSpeedUpUNet(in_channels=2, out_channels=2).state_dict()
    golden = HERE / "golden"
    (golden / "speedup_state_dict.json").write_text(json.dumps([[k, list(v.shape)] for k, v in state.items()], indent=0) + "\n")
    import speedup_ref
    weights = speedup_ref.seeded_weights(PIN_SEED)
    low_photon, forward_projection = speedup_ref.seeded_inputs(PIN_SEED, *PIN_SHAPE)
    mean, variance = reference_predict(reference_tree, weights, low_photon, forward_projection)
    np.savez_compressed(golden / "speedup_pin.npz", mean=mean, variance=variance)
    print(f"{len(state)} tensors, {sum(v.numel() for v in state.values())} values; mean {mean.min():.3g} .. {mean.max():.3g}, "
          f"variance {variance.min():.3g} .. {variance.max():.3g}, zero mean pixels {np.mean(mean == 0):.2%}")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
