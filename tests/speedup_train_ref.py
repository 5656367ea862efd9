"""Restatement in float64 of the training rule of the speed-up network (csrc/speedup_train.hip's header), written from that
description: the oracle of tests/test_speedup_train.py and tests/test_speedup_train_gpu.py.  The network is speedup_ref's
functional one, differentiated by autograd; the operators of the backward pass are stated once more in numpy, the way the kernels
compute them, and test_speedup_train.py holds the two statements against each other.

Per batch of B samples (low_photon lp, forward_projection or None, high_photon t), N = B nv nu, every sample run alone:
  phase "mean":      loss = mean |m - t|, gradients of the mean net only;
  phase "variance":  loss = mean 0.5 (log v' + (m - t)^2 / v'), v' = max(v, 1e-6), m detached, gradients of the variance net only."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import speedup_ref

PSNR_MAX = 8.711442


# ------------------------------------------------------------------------------------------------------ losses and heads, numpy
def l1_loss(m, t, n_total=None):
    """(loss, dL/dm): mean |m - t| over n_total elements (default: m.size); the sign of 0 is 0."""
    m, t = np.asarray(m, np.float64), np.asarray(t, np.float64)
    n = m.size if n_total is None else n_total
    return np.abs(m - t).sum() / n, np.sign(m - t) / n


def head_mean_grad(lp, net, dl_dm):
    """dL/dnet through m = relu(lp + 10 tanh(net))."""
    lp, net = np.asarray(lp, np.float64), np.asarray(net, np.float64)
    th = np.tanh(net)
    return dl_dm * (lp + 10.0 * th > 0) * 10.0 * (1.0 - th * th)


def nll_loss(m, v, t, n_total=None):
    """(loss, dL/dv): mean 0.5 (log v' + (m - t)^2 / v'), v' = max(v, 1e-6); no gradient where the clamp holds."""
    m, v, t = (np.asarray(a, np.float64) for a in (m, v, t))
    n = m.size if n_total is None else n_total
    vc = np.maximum(v, 1e-6)
    loss = (0.5 * (np.log(vc) + (m - t) ** 2 / vc)).sum() / n
    return loss, np.where(v > 1e-6, 0.5 * (1.0 / vc - (m - t) ** 2 / vc ** 2) / n, 0.0)


def head_variance_grad(m, s, dl_dv):
    """dL/ds through v = m 0.1 sigmoid(s) + 1e-6, m held fixed."""
    m, s = np.asarray(m, np.float64), np.asarray(s, np.float64)
    sg = 1.0 / (1.0 + np.exp(-s))
    return dl_dv * m * 0.1 * sg * (1.0 - sg)


def adam(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One update -> (w, m, v), float64."""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return w - lr / (1.0 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps), m, v


def psnr(image, reference_image):
    return 20.0 * np.log10(PSNR_MAX / np.sqrt(np.mean((np.asarray(image, np.float64) - np.asarray(reference_image, np.float64)) ** 2)))


# ------------------------------------------------------------------------------------------------------------ operators, numpy
def upsampled(a, H, W):
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)[:, :H, :W]


def conv_dgrad(dy, w, c1, upsample):
    """The input gradient of conv3x3(cat([a, upsample(b)])) as the kernels compute it: the zero-padded correlation of dY with the
    weights transposed in (co, ci) and flipped in the taps on rows -1 .. H and columns -1 .. W, the border folded inwards, the
    channels split into the two sources, the second summed over 2 x 2 blocks -> (d a [c1, H, W], d b or None)."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    c_out, H, W = dy.shape
    c_in = w.shape[1]
    pad = np.zeros((c_out, H + 4, W + 4))
    pad[:, 2:H + 2, 2:W + 2] = dy
    ext = np.zeros((c_in, H + 2, W + 2))
    for ty in range(3):
        for tx in range(3):
            # ext[ci, q] += sum_co w[co, ci, 2 - ty, 2 - tx] dY[co, q + (ty - 1, tx - 1)], q on the extended grid
            ext += np.einsum("oi,ohw->ihw", w[:, :, 2 - ty, 2 - tx], pad[:, ty:ty + H + 2, tx:tx + W + 2])
    g = ext[:, 1:H + 1, 1:W + 1].copy()
    g[:, 0, :] += ext[:, 0, 1:W + 1]
    g[:, H - 1, :] += ext[:, H + 1, 1:W + 1]
    g[:, :, 0] += ext[:, 1:H + 1, 0]
    g[:, :, W - 1] += ext[:, 1:H + 1, W + 1]
    g[:, 0, 0] += ext[:, 0, 0]
    g[:, 0, W - 1] += ext[:, 0, W + 1]
    g[:, H - 1, 0] += ext[:, H + 1, 0]
    g[:, H - 1, W - 1] += ext[:, H + 1, W + 1]
    if c_in == c1:
        return g, None
    second = g[c1:]
    if upsample:
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        full = np.zeros((c_in - c1, 2 * H2, 2 * W2))
        full[:, :H, :W] = second
        second = full.reshape(c_in - c1, H2, 2, W2, 2).sum(axis=(2, 4))
    return g[:c1], second


def conv_wgrad(x, dy):
    """dW [c_out, c_in, 3, 3] and db [c_out] of conv3x3 (replicate padding) for its input x [c_in, H, W] and dY [c_out, H, W]."""
    x, dy = torch.as_tensor(np.asarray(x, np.float64)), torch.as_tensor(np.asarray(dy, np.float64))
    xp = F.pad(x[None], (1, 1, 1, 1), mode="replicate")[0]
    dw = F.conv2d(xp[:, None], dy[:, None])  # [c_in, c_out, 3, 3]: a correlation of every input channel with every dY channel
    return dw.permute(1, 0, 2, 3).contiguous().numpy(), dy.sum(dim=(1, 2)).numpy()


def maxpool_backward(x, dy):
    """The gradient goes to the first maximal element of each 2 x 2 window in the order (0,0), (0,1), (1,0), (1,1)."""
    x = np.asarray(x)
    C, H, W = x.shape
    dx = np.zeros((C, H, W), np.float64)
    for c in range(C):
        for yo in range(H // 2):
            for xo in range(W // 2):
                win = x[c, 2 * yo:2 * yo + 2, 2 * xo:2 * xo + 2].ravel()
                k = int(np.argmax(win))  # the first maximum
                dx[c, 2 * yo + k // 2, 2 * xo + k % 2] += dy[c, yo, xo]
    return dx


def norm_lrelu_backward(x, dy, dtype=torch.float64):
    """dx of leaky_relu(instance_norm(x)) by autograd."""
    t = torch.as_tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True)
    y = speedup_ref.norm_lrelu(t[None])[0]
    y.backward(torch.as_tensor(np.asarray(dy), dtype=dtype))
    return t.grad.numpy()


def norm_lrelu_backward_statement(x, dy):
    """The same by the rule of the kernels, float64: d xh = dy (xh > 0 ? 1 : 0.01), dx = rstd (d xh - mean d xh - xh mean(d xh xh))."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    mean = x.mean(axis=(1, 2), keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(axis=(1, 2), keepdims=True) + 1e-5)
    xh = (x - mean) * rstd
    dxh = dy * np.where(xh > 0, 1.0, 0.01)
    return rstd * (dxh - dxh.mean(axis=(1, 2), keepdims=True) - xh * (dxh * xh).mean(axis=(1, 2), keepdims=True))


# ------------------------------------------------------------------------------------------------------- the whole rule, autograd
def normed_biases(names):
    """The biases of convolutions that feed an instance norm: every bias but init_conv's and final_conv's."""
    return [n for n in names if n.endswith(".bias") and ".init_conv." not in n and ".final_conv." not in n]


def forward(w, lp, fp):
    """(net_m, m, s, v) of one sample, tensors [1, 1, H, W]; w: tensors by name."""
    x = lp if fp is None else torch.cat([lp, speedup_ref.preprocess(lp, fp)], dim=1)
    net_m = speedup_ref.unet(x, w, "mean_net")
    m = torch.relu(lp + 10.0 * torch.tanh(net_m))
    s = speedup_ref.unet(m.detach(), w, "var_net")
    v = m.detach() * (0.10 * torch.sigmoid(s)) + 1e-6
    return net_m, m, s, v


def loss_and_gradients(weights: dict, low_photon, forward_projection, high_photon, phase: str, dtype=torch.float64):
    """-> (metrics dict, gradients by name as float64 numpy arrays; zero outside the phase's net).  Samples run alone; the losses
    are sums over samples divided by N = B nv nu (what reduction="mean" over the batch gives)."""
    w = {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(True) for k, v in weights.items() if k != "var_scale"}
    B = low_photon.shape[0]
    N = float(np.prod(low_photon.shape))
    l1 = nll = 0.0
    se_before = se_after = 0.0
    for p in range(B):
        lp = torch.as_tensor(low_photon[p:p + 1, None], dtype=dtype)
        fp = None if forward_projection is None else torch.as_tensor(forward_projection[p:p + 1, None], dtype=dtype)
        t = torch.as_tensor(high_photon[p:p + 1, None], dtype=dtype)
        _, m, _, v = forward(w, lp, fp)
        l1 = l1 + F.l1_loss(m, t, reduction="sum") / N
        nll = nll + F.gaussian_nll_loss(m.detach(), t, v, reduction="sum") / N
        se_before += float(((lp - t) ** 2).sum())
        se_after += float(((m.detach() - t) ** 2).sum())
    loss = l1 if phase == "mean" else nll
    loss.backward()
    grads = {k: (t.grad.numpy().astype(np.float64) if t.grad is not None else np.zeros(t.shape)) for k, t in w.items()}
    metrics = {"loss": float(loss), "l1_loss": float(l1), "gaussian_nll_loss": float(nll),
               "psnr_before": 20.0 * np.log10(PSNR_MAX / np.sqrt(se_before / N)), "psnr_after": 20.0 * np.log10(PSNR_MAX / np.sqrt(se_after / N))}
    return metrics, grads


def mean_and_variance(weights: dict, low_photon, forward_projection, dtype=torch.float64):
    return speedup_ref.predict(weights, low_photon, forward_projection, dtype=dtype)
