"""Float64 restatement of the training of the CT segmentation network, written from its description (csrc/segment_train.hip's
header), not from the reference's source: the oracle of tests/test_segment_train.py and tests/test_segment_train_gpu.py.  It builds
on tests/segment_ref.py (`unet`, `head`).  tests/golden/segment_train_pin.npz chains the loss to the reference's own `DiceLoss`.

Loss (the reference driver's SegmentationLoss(use_dice=True) on DiceLoss(include_background=True, reduction="none")): p = softmax
over channels 0 .. 7, sigmoid on channel 8; per sample and channel I = sum t p, G = sum t, P = sum p; f = 1 - (2 I + 1e-5) /
(G + P + 1e-5); loss = mean of f."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import segment_ref

GOLDEN = Path(__file__).resolve().parent / "golden"
SMALL_FILTERS = (4, 4, 6, 6, 4, 4)  # L = 2


# ----------------------------------------------------------------------------------------------------------------- the loss
def dice_f(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """f [B, 9] of logits and target [B, 9, ...]."""
    p = segment_ref.head(logits)
    axes = tuple(range(2, p.ndim))
    inter, ground, pred = (target * p).sum(axes), target.sum(axes), p.sum(axes)
    return 1.0 - (2.0 * inter + 1e-5) / (ground + pred + 1e-5)


def loss_of(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return dice_f(logits, target).mean()


def head_gradient(logits: np.ndarray, target: np.ndarray) -> np.ndarray:
    """d loss / d logits [B, 9, ...] in closed form, float64: with D = G + P + 1e-5, g = (-2 t / D + (2 I + 1e-5) / D^2) / (9 B);
    dz_c = p_c (g_c - sum_{j<8} g_j p_j) for c < 8; dz_8 = g_8 p_8 (1 - p_8)."""
    z, t = np.asarray(logits, dtype=np.float64), np.asarray(target, dtype=np.float64)
    p = segment_ref.head(torch.as_tensor(z)).numpy()
    axes = tuple(range(2, z.ndim))
    inter, denom = (t * p).sum(axes, keepdims=True), t.sum(axes, keepdims=True) + p.sum(axes, keepdims=True) + 1e-5
    g = (-2.0 * t / denom + (2.0 * inter + 1e-5) / denom ** 2) / (9.0 * z.shape[0])
    out = np.empty_like(z)
    dot = (g[:, :8] * p[:, :8]).sum(1, keepdims=True)
    out[:, :8] = p[:, :8] * (g[:, :8] - dot)
    out[:, 8] = g[:, 8] * p[:, 8] * (1.0 - p[:, 8])
    return out


def seeded_target(seed: int, shape, absent: int = 5) -> np.ndarray:
    """uint8 [9, ...]: a one-hot of labels 0 .. 7 in blobs with label `absent` missing, and channel 8 an overlay inside label 6."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij")
    field = np.floor(4.0 * (np.sin(5.0 * z + 1.0) + np.cos(4.0 * y) + np.sin(3.0 * x + 2.0 * z)) + 12.0).astype(np.int64) % 8
    field[field == absent] = (absent + 1) % 8
    field.flat[0], field.flat[-1] = 6, 6
    out = np.zeros((9,) + tuple(shape), np.uint8)
    for c in range(8):
        out[c] = field == c
    out[8] = (field == 6) & (rng.random(shape) < 0.7)
    out[8].flat[0] = 1
    return out


# ----------------------------------------------------------------------------------------------------------- the operators
def staged_input(x, x2, upsample):
    """What a convolution sees: cat([x, x2 (through the x 2 nearest upsample, cropped to x's extent)]); tensors [1, c, ...]."""
    if x2 is None:
        return x
    if upsample:
        x2 = F.interpolate(x2, scale_factor=2, mode="nearest")[..., :x.shape[2], :x.shape[3], :x.shape[4]]
    return torch.cat([x, x2], dim=1)


def conv_gradients(x, x2, upsample, weight, dy):
    """(dW, db, dx, dx2) in float64 by autograd of the zero-padded 3 x 3 x 3 convolution of the staged input; arrays without batch."""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float64)[None].requires_grad_(True)  # noqa: E731
    tx, tx2 = t(x), t(x2)
    tw = torch.as_tensor(np.asarray(weight), dtype=torch.float64).requires_grad_(True)
    tb = torch.zeros(tw.shape[0], dtype=torch.float64, requires_grad=True)
    y = F.conv3d(staged_input(tx, tx2, upsample), tw, tb, padding=1)
    y.backward(torch.as_tensor(np.asarray(dy), dtype=torch.float64)[None])
    return tw.grad.numpy(), tb.grad.numpy(), tx.grad[0].numpy(), None if tx2 is None else tx2.grad[0].numpy()


def maxpool_backward(x, dy):
    """dx [c, ...] in float64 by torch's CPU autograd of max_pool3d(2): the first maximum of a window in scan order gets it."""
    tx = torch.as_tensor(np.asarray(x), dtype=torch.float64)[None].requires_grad_(True)
    F.max_pool3d(tx, 2).backward(torch.as_tensor(np.asarray(dy), dtype=torch.float64)[None])
    return tx.grad[0].numpy()


def gradients(weights: dict, patches: np.ndarray, targets: np.ndarray, dtype=torch.float64):
    """(loss, f [B, 9], {name: gradient}) of a batch [B, P0, P1, P2] with targets [B, 9, ...] by autograd of segment_ref.unet."""
    w = {k: v.requires_grad_(True) for k, v in segment_ref.as_tensors(weights, dtype).items()}
    logits = torch.cat([segment_ref.unet(torch.as_tensor(p[None, None], dtype=dtype), w) for p in patches])
    f = dice_f(logits, torch.as_tensor(np.asarray(targets), dtype=dtype))
    loss = f.mean()
    loss.backward()
    return float(loss.detach()), f.detach().numpy(), {k: v.grad.numpy() for k, v in w.items()}


def adam_step(w, g, m, v, t: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """One Adam update in float64 -> (w, m, v)."""
    w, g, m, v = (np.asarray(a, dtype=np.float64) for a in (w, g, m, v))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return w - lr / (1.0 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps), m, v


def train(weights: dict, patch: np.ndarray, target: np.ndarray, steps: int, lr: float):
    """The losses before each of `steps` updates of torch.optim.Adam on one fixed patch, in float64."""
    w = {k: v.requires_grad_(True) for k, v in segment_ref.as_tensors(weights, torch.float64).items()}
    opt = torch.optim.Adam(list(w.values()), lr=lr)
    x, t = torch.as_tensor(patch[None, None], dtype=torch.float64), torch.as_tensor(target[None], dtype=torch.float64)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_of(segment_ref.unet(x, w), t)
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out


# ------------------------------------------------------------------------------------------------------------ the host rules
def plateau(losses, lr, factor=0.9, patience=1000, threshold=1e-2, cooldown=1000, min_lr=1e-6, eps=1e-8):
    """The learning rate after each loss: an improvement is loss < best (1 - threshold); more than `patience` steps without one
    lower the rate to max(lr factor, min_lr) and start `cooldown` steps during which bad steps do not count."""
    best, bad, cool, out = float("inf"), 0, 0, []
    for loss in losses:
        if loss < best * (1.0 - threshold):
            best, bad = loss, 0
        else:
            bad += 1
        if cool > 0:
            cool, bad = cool - 1, 0
        if bad > patience:
            new = max(lr * factor, min_lr)
            lr = new if lr - new > eps else lr
            cool, bad = cooldown, 0
        out.append(lr)
    return out


def merge(seg: dict) -> np.ndarray:
    """uint8 [9, ...]: background = body == 0; other = none of the six tissues nor background; lung_vessels as it is."""
    background = seg["body"] == 0
    six = ("upper_body_bones", "upper_body_muscles", "upper_body_fat", "liver", "stomach", "lung")
    other = ~(np.any([seg[k] != 0 for k in six], axis=0) | background)
    order = [background] + [seg[k] for k in six[:3]] + [seg["liver"], seg["stomach"], seg["lung"], other, seg["lung_vessels"]]
    return np.stack(order).astype(np.uint8)


def pad_widths(shape, patch_shape):
    """(left, right) per axis: left = pad // 2."""
    return [((p - n) // 2, (p - n) - (p - n) // 2) if n < p else (0, 0) for n, p in zip(shape, patch_shape)]


def decision_margins(weights: dict, patch: np.ndarray):
    """How far the discrete decisions of a forward pass lie from being taken the other way by float32 arithmetic, from the restatement
    alone (float64 for the values, torch's float32 CPU run for the error): per normed layer, in the order of the pass, the smallest
    |normalised value| (its sign is the LeakyReLU's slope) over the largest float32 error of that layer; per max-pool, the smallest
    non-zero gap between the two largest values of a window over the float32 error of the pooled tensor (a gap of exactly 0 is a true
    tie, which the scan order decides in any precision).  -> (ratios of the normed layers, ratios of the pools)."""
    def run(dtype):
        w = segment_ref.as_tensors(weights, dtype)
        levels = 1 + max(int(k.split(".")[0][4:]) for k in w if k.startswith("enc_"))
        normed = []

        def block(y, name):
            for j in (0, 3):
                xh = F.instance_norm(segment_ref.conv3(y, w[f"{name}.convs.{j}.weight"], w[f"{name}.convs.{j}.bias"]), eps=1e-5)
                normed.append(xh.double())
                y = F.leaky_relu(xh, 0.01)
            return y

        with torch.no_grad():
            skips = [segment_ref.conv3(torch.as_tensor(patch[None, None], dtype=dtype), w["init_conv.weight"], w["init_conv.bias"])]
            for i in range(levels):
                skips.append(block(F.max_pool3d(skips[-1], 2), f"enc_{i}"))
            y = skips[-1]
            for i in reversed(range(levels)):
                y = block(torch.cat([skips[i], F.interpolate(y, scale_factor=2, mode="nearest")], dim=1), f"dec_{i}")
        return normed, [s.double() for s in skips[:-1]]

    n64, s64 = run(torch.float64)
    n32, s32 = run(torch.float32)
    layers = [float(a.abs().min() / (a - b).abs().max()) for a, b in zip(n64, n32)]
    pools = []
    for a, b in zip(s64, s32):
        top = a.unfold(2, 2, 2).unfold(3, 2, 2).unfold(4, 2, 2).reshape(*a.shape[:2], -1, 8).topk(2, dim=-1).values
        gap = top[..., 0] - top[..., 1]
        pools.append(float(gap[gap > 0].min() / (a - b).abs().max()) if (gap > 0).any() else float("inf"))
    return layers, pools
