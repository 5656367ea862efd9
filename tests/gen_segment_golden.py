"""Regenerate the fixtures that chain tests/segment_ref.py to the reference's own network class:

  tests/golden/segment_state_dict.json   names and shapes of FlexUNet(1, 9, 4, n_filters=[32] * 10).state_dict(), in its order
  tests/golden/segment_pin.npz           the reference class's float64 logits for seeded_weights(7) on one 16 x 16 x 32 patch

Usage: python tests/gen_segment_golden.py <reference tree>.  The reference class is imported at run time; nothing of it is kept.
Its patching module is not imported (it needs SimpleITK); the patch rule is tested in plain integers."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))


def reference_model(reference_tree, n_filters, levels):
    """The network as cbctmc/segmentation/segmenter.py builds it, in float64."""
    sys.path.insert(0, str(reference_tree))
    import torch.nn as nn
    from cbctmc.speedup.models import FlexUNet
    return FlexUNet(n_channels=1, n_classes=9, n_levels=levels, n_filters=list(n_filters), convolution_layer=nn.Conv3d, downsampling_layer=nn.MaxPool3d,
                    upsampling_layer=nn.Upsample, norm_layer=nn.InstanceNorm3d, skip_connections=True, return_bottleneck=False).double().eval()


def reference_logits(reference_tree, weights: dict, patch: np.ndarray, n_filters, levels) -> np.ndarray:
    """[9, d0, d1, d2] float64 of the reference class on one rescaled patch."""
    model = reference_model(reference_tree, n_filters, levels)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in weights.items()})
    with torch.no_grad():
        return model(torch.as_tensor(patch[None, None], dtype=torch.float64))[0].numpy()


def main(reference_tree):
    import segment_ref
    state = reference_model(reference_tree, segment_ref.REFERENCE_FILTERS, 4).state_dict()
    golden = HERE / "golden"
    (golden / "segment_state_dict.json").write_text(json.dumps([[k, list(v.shape)] for k, v in state.items()], indent=0) + "\n")
    weights = segment_ref.seeded_weights(segment_ref.PIN_SEED)
    patch = segment_ref.rescale(segment_ref.seeded_image(segment_ref.PIN_SEED, segment_ref.PIN_PATCH))
    logits = reference_logits(reference_tree, weights, patch, segment_ref.REFERENCE_FILTERS, 4)
    np.savez(golden / "segment_pin.npz", logits=logits)
    print(f"{len(state)} tensors, {sum(v.numel() for v in state.values())} values; logits {logits.shape} {logits.min():.3g} .. {logits.max():.3g}")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
