"""Training of the speed-up network on the MI355X (csrc/speedup_train.hip through mcgpu_speedup_train_*): every backward operator
against float64, the whole gradient against float64 autograd of the restatement (speedup_train_ref.py) with torch's float32 CPU run of
the same restatement as the yardstick, and short training runs."""
import numpy as np
import pytest

import cases
import speedup_ref
import speedup_train_ref as ref

torch = pytest.importorskip("torch")

speedup = cases.pkg.speedup
training = cases.pkg.speedup_training
stage = training.speedup_train_stage
pytestmark = pytest.mark.gpu

CONV_PAIRS = [((2, 0), 64), ((64, 0), 64), ((64, 0), 1), ((1, 0), 16), ((48, 0), 32), ((64, 128), 64), ((5, 3), 7)]  # ((c1, c2 upsampled), c_out)
CONV_SHAPES = [(1, 1), (5, 7), (33, 70), (32, 48)]  # rows x columns: one pixel, below a tile, several tiles with ragged edges, whole tiles


def _spacing(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _conv_case(rng, c1, c2, c_out, H, W, integers):
    draw = (lambda lo, hi, size: rng.integers(lo, hi + 1, size=size).astype(np.float32)) if integers else \
        (lambda lo, hi, size: rng.uniform(lo, hi, size=size).astype(np.float32))
    x1 = draw(-3, 3, (c1, H, W))
    x2 = draw(-3, 3, (c2, (H + 1) // 2, (W + 1) // 2)) if c2 else None
    w = draw(-8, 8, (c_out, c1 + c2, 3, 3)) if integers else draw(-1, 1, (c_out, c1 + c2, 3, 3))
    dy = draw(-3, 3, (c_out, H, W))
    x = x1 if x2 is None else np.concatenate([x1, ref.upsampled(x2, H, W)])
    return x1, x2, w, dy, x


# --------------------------------------------------------------------------------------------------------------- convolution
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", CONV_PAIRS, ids=lambda p: f"{p[0][0]}+{p[0][1]}to{p[1]}")
def test_conv_gradients_of_small_integers_are_bit_equal_to_float64(engine, pair, shape):
    """|x|, |dy| <= 3 and |w| <= 8, unrelated across channels, taps and pixels: every sum is an integer below 2^24 (asserted), exact in
    float32 in any order, so both gradients equal float64 bit for bit; a slip in a lane map, the tap flip, the fold, the split of the
    sources or the order of the partials gives a wrong integer."""
    (c1, c2), c_out = pair
    H, W = shape
    x1, x2, w, dy, x = _conv_case(np.random.default_rng(c1 * 1000 + c_out + H), c1, c2, c_out, H, W, integers=True)
    (dw, db, partials), _ = stage("conv_wgrad", x1, in2=x2, in3=dy, upsample=bool(c2))
    want_w, want_b = ref.conv_wgrad(x, dy)
    assert ref.conv_wgrad(np.abs(x), np.abs(dy))[0].max() < 2 ** 24 and partials >= 4
    assert np.array_equal(dw.astype(np.float64), want_w) and np.array_equal(db.astype(np.float64), want_b)
    (d1, d2), _ = stage("conv_dgrad", dy, in2=w, c_out=c1, upsample=bool(c2))
    want1, want2 = ref.conv_dgrad(dy, w, c1, upsample=bool(c2))
    bound1, bound2 = ref.conv_dgrad(np.abs(dy), np.abs(w), c1, upsample=bool(c2))
    assert bound1.max() < 2 ** 24 and (bound2 is None or bound2.max() < 2 ** 24)
    assert np.array_equal(d1.astype(np.float64), want1)
    assert (d2 is None and want2 is None) or np.array_equal(d2.astype(np.float64), want2)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", CONV_PAIRS, ids=lambda p: f"{p[0][0]}+{p[0][1]}to{p[1]}")
def test_conv_gradients_of_float_data_are_within_the_bound_of_a_float32_fma_chain(engine, pair, shape):
    """Weight gradient: |got - float64| <= (pixels + partials) 2^-24 sum |x dy|; input gradient: <= (9 C_out + 1) 2^-24 sum |dy w|
    (the forward's bound with the roles of the channels exchanged).

    Measured on the MI355X, largest error / bound over all cases: weight gradient 0.199 (one pixel, 4 partials; 1e-4 at 32 x 48), input
    gradient 0.343 (64 -> 1 at 33 x 70: one output channel, so a chain of 9 products)."""
    (c1, c2), c_out = pair
    H, W = shape
    x1, x2, w, dy, x = _conv_case(np.random.default_rng(c1 * 1000 + c_out + W), c1, c2, c_out, H, W, integers=False)
    (dw, _, partials), _ = stage("conv_wgrad", x1, in2=x2, in3=dy, upsample=bool(c2))
    want_w, _ = ref.conv_wgrad(x, dy)
    bound = (H * W + partials) * 2.0 ** -24 * ref.conv_wgrad(np.abs(x), np.abs(dy))[0]
    excess_w = (np.abs(dw - want_w) / bound).max()
    (d1, d2), _ = stage("conv_dgrad", dy, in2=w, c_out=c1, upsample=bool(c2))
    want1, want2 = ref.conv_dgrad(dy, w, c1, upsample=bool(c2))
    bound1, bound2 = ref.conv_dgrad(np.abs(dy), np.abs(w), c1, upsample=bool(c2))
    excess_d = (np.abs(d1 - want1) / ((9 * c_out + 1) * 2.0 ** -24 * bound1)).max()
    if c2:
        excess_d = max(excess_d, (np.abs(d2 - want2) / ((9 * c_out + 1) * 2.0 ** -24 * bound2)).max())
    print(f"conv gradients {pair} {shape}: max error / bound = {excess_w:.3g} (weights, {partials} partials), {excess_d:.3g} (input)")
    assert excess_w <= 1.0 and excess_d <= 1.0


def test_weight_gradient_at_full_size_indexes_every_tile(engine):
    """768 x 1024, 2 -> 8 channels, values in {-1, 0, 1}: exact, every tile indexed, 1892 partials of which the last group is ragged
    (6144 tiles in 473 splits of 13)."""
    rng = np.random.default_rng(6)
    H, W = 768, 1024
    x = rng.integers(-1, 2, size=(2, H, W)).astype(np.float32)
    dy = rng.integers(-1, 2, size=(8, H, W)).astype(np.float32)
    (dw, db, partials), rep = stage("conv_wgrad", x, in3=dy)
    want_w, want_b = ref.conv_wgrad(x, dy)
    assert partials == 4 * 473 and (H // 4) * (W // 32) % 473 != 0
    assert np.array_equal(dw.astype(np.float64), want_w) and np.array_equal(db.astype(np.float64), want_b)
    assert rep["ms_wgrad"] > 0


# ------------------------------------------------------------------------------------------------------ norm, pool, losses, Adam
def _norm_inputs():
    rng = np.random.default_rng(13)
    smallest = rng.normal(size=(3, 2, 2)).astype(np.float32)           # H W = 4: the bottleneck of the smallest legal image
    offset = rng.normal(size=(4, 33, 70)).astype(np.float32)
    offset[0] += 1e3                                                   # mean 1e3, spread 1
    offset[1] *= 1e-3
    segments = rng.normal(2.0, 3.0, size=(2, 256, 160)).astype(np.float32)  # 40960 pixels: three segments of sums
    return {"2x2": smallest, "offset": offset, "segments": segments}


@pytest.mark.parametrize("name", ["2x2", "offset", "segments"])
def test_norm_lrelu_backward_is_as_close_to_float64_as_the_float32_operator_of_torch(engine, name):
    """Error against float64 autograd at most 2 x the largest error of torch's float32 CPU autograd in the same channel, with a floor
    of 4 spacings of the value; the gradient of a channel sums to zero to rounding.

    Measured on the MI355X, max error / bound: 2x2 0.343, offset 0.125, segments 0.125 (errors 1.37e-7, 3.03e-5, 5.85e-8)."""
    x = _norm_inputs()[name]
    dy = np.random.default_rng(14).normal(size=x.shape).astype(np.float32)
    want = ref.norm_lrelu_backward(x, dy)
    yard = np.abs(ref.norm_lrelu_backward(x, dy, dtype=torch.float32) - want).max(axis=(1, 2), keepdims=True)
    got, _ = stage("norm_lrelu_backward", x, in2=dy)
    err = np.abs(got - want)
    bound = np.maximum(2 * yard, 4 * _spacing(want))
    print(f"norm backward {name}: max error {err.max():.3g}, yardstick {yard.max():.3g}, max error / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    n = x.shape[1] * x.shape[2]
    assert np.all(np.abs(got.astype(np.float64).sum(axis=(1, 2))) <= n * 2.0 ** -24 * np.abs(got).max(axis=(1, 2)))
    again, _ = stage("norm_lrelu_backward", x, in2=dy)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 6, 10), (2, 7, 9), (5, 64, 96)])
def test_maxpool_backward_is_bit_equal_ties_included(engine, shape):
    rng = np.random.default_rng(1)
    x = rng.integers(0, 3, size=shape).astype(np.float32)  # three values: most windows hold a tie
    dy = rng.normal(size=(shape[0], shape[1] // 2, shape[2] // 2)).astype(np.float32)
    t = torch.as_tensor(x).clone().requires_grad_(True)
    torch.nn.functional.max_pool2d(t[None], 2).backward(torch.as_tensor(dy)[None])
    got, _ = stage("maxpool_backward", x, in2=dy)
    assert np.array_equal(got, t.grad.numpy())
    y = rng.normal(size=shape).astype(np.float32)
    t = torch.as_tensor(y).clone().requires_grad_(True)
    torch.nn.functional.max_pool2d(t[None], 2).backward(torch.as_tensor(dy)[None])
    assert np.array_equal(stage("maxpool_backward", y, in2=dy)[0], t.grad.numpy())


def test_losses_and_head_gradients_equal_their_statements(engine):
    """Within 4 float32 spacings, from the device's own head outputs (m and v are the forward's float32 values)."""
    rng = np.random.default_rng(2)
    lp = rng.uniform(1.0, 4.0, size=(2, 33, 70)).astype(np.float32)
    net = rng.normal(0.0, 0.02, size=lp.shape).astype(np.float32)  # 10 tanh: a spread of 0.2 under lp >= 1
    lp[0, 0, 0], net[0, 0, 0] = 0.2, -0.5  # clipped by the relu: m = 0, v = 1e-6
    t = (lp + rng.choice([-1.0, 1.0], size=lp.shape) * rng.uniform(0.2, 0.5, size=lp.shape)).astype(np.float32)
    (loss, g, m), _ = stage("loss_l1", lp, in2=net, in3=t)
    t[1, 2, 3] = m[1, 2, 3]  # m == t: sign 0
    (loss, g, m), _ = stage("loss_l1", lp, in2=net, in3=t)
    assert m[0, 0, 0] == 0 and np.count_nonzero(m == 0) == 1
    want_loss, dl_dm = ref.l1_loss(m, t)
    want = ref.head_mean_grad(lp, net, dl_dm) * (m > 0)
    assert abs(loss - want_loss) <= 4 * np.spacing(np.float32(want_loss))
    assert g[0, 0, 0] == 0 and g[1, 2, 3] == 0 and np.all(np.abs(g - want) <= 4 * _spacing(want))
    s = rng.normal(0.0, 1.0, size=lp.shape).astype(np.float32)
    (loss, g, v), _ = stage("loss_nll", m, in2=s, in3=t)
    assert v[0, 0, 0] == np.float32(1e-6) and v.min() == np.float32(1e-6)
    want_loss, dl_dv = ref.nll_loss(m, v, t)
    want = ref.head_variance_grad(m, s, dl_dv)
    assert abs(loss - want_loss) <= 4 * np.spacing(np.float32(abs(want_loss)))
    assert g[0, 0, 0] == 0 and np.all(np.abs(g - want) <= 4 * _spacing(want))


def test_one_adam_step_equals_the_float64_statement(engine):
    rng = np.random.default_rng(3)
    n = 1000
    w = rng.normal(size=n).astype(np.float32)
    g = (rng.normal(size=n) * 10.0 ** rng.integers(-6, 2, size=n)).astype(np.float32)
    m = (rng.normal(size=n) * 1e-2).astype(np.float32)
    v = (rng.uniform(size=n) * 1e-3).astype(np.float32)
    g[:10], m[:10], v[:10] = 0, 0, 0  # no gradient and no history: nothing may move
    for t in (1, 7, 5000):
        (w2, m2, v2), _ = stage("adam", g, state=(w, m, v), step=t, lr=1e-3)
        want = ref.adam(w, g, m, v, t, 1e-3)
        for got, wnt in zip((w2, m2, v2), want):
            assert np.all(np.abs(got - wnt) <= 2 * _spacing(wnt))
        assert w2[:10].tobytes() == w[:10].tobytes() and not m2[:10].any() and not v2[:10].any()


# ------------------------------------------------------------------------------------------------------------- whole gradient
GOLDEN = ((2, 4, 64), (1, 2, 16))
GRADIENT_CASES = {  # (mean net, variance net), (nv, nu), batch, phase
    "2-1-8_32x48_b1_mean": (((2, 1, 8), (1, 1, 8)), (32, 48), 1, "mean"),
    "2-1-8_64x80_b3_variance": (((2, 1, 8), (1, 1, 8)), (64, 80), 3, "variance"),
    "2-2-8_64x80_b3_mean": (((2, 2, 8), (1, 2, 8)), (64, 80), 3, "mean"),
    "2-2-8_32x48_b1_variance": (((2, 2, 8), (1, 2, 8)), (32, 48), 1, "variance"),
    "golden_32x48_b1_mean": (GOLDEN, (32, 48), 1, "mean"),
    "golden_64x80_b1_mean": (GOLDEN, (64, 80), 1, "mean"),
    "golden_64x80_b3_variance": (GOLDEN, (64, 80), 3, "variance"),
    "no-fp_1-2-8_32x48_b3_mean": (((1, 2, 8), (1, 2, 8)), (32, 48), 3, "mean"),
}
_cases = {}


def _gradient_case(name):
    """Weights, a batch in which no decision is fragile, the float64 gradient and the float32 CPU yardstick; computed once."""
    if name in _cases:
        return _cases[name]
    nets, (nv, nu), batch, phase = GRADIENT_CASES[name]
    weights = speedup_ref.seeded_weights(7, speedup.state_dict_tensors(*nets))
    for part in ("weight", "bias"):  # damped further than seeded_weights does: the mean must stay clear of the relu's kink
        weights[f"mean_net.final_conv.{part}"] = weights[f"mean_net.final_conv.{part}"] * np.float32(0.2)
    lp, fp = speedup_ref.seeded_inputs(7, batch, nv, nu)
    fp = fp if nets[0][0] == 2 else None
    m64, v64 = ref.mean_and_variance(weights, lp, fp)
    rng = np.random.default_rng(8)
    t = (m64 + rng.choice([-1.0, 1.0], size=m64.shape) * rng.uniform(0.2, 0.5, size=m64.shape)).astype(np.float32)
    assert m64.min() >= 0.1 and v64.min() >= 1e-3
    assert 0.2 - 1e-6 <= np.abs(m64 - t).min() and np.abs(m64 - t).max() <= 0.5 + 1e-6
    metrics, g64 = ref.loss_and_gradients(weights, lp, fp, t, phase)
    _, g32 = ref.loss_and_gradients(weights, lp, fp, t, phase, dtype=torch.float32)
    _cases[name] = dict(nets=nets, weights=weights, data={"low_photon": lp, "forward_projection": fp, "high_photon": t}, phase=phase, metrics=metrics,
                        g64=g64, g32=g32)
    return _cases[name]


def _rel_l2(a, b):
    return np.linalg.norm(np.asarray(a, np.float64).ravel() - b.ravel()) / np.linalg.norm(b.ravel())


@pytest.mark.parametrize("name", list(GRADIENT_CASES))
def test_gradients_are_as_close_to_float64_autograd_as_the_float32_run_of_torch(engine, name):
    """Per tensor, the relative L2 error against float64 autograd of the restatement is at most 4 x that of torch's float32 CPU
    autograd of the same restatement; the biases of normed convolutions are exactly 0; the losses equal the restatement's.

    Measured on the MI355X, largest ratio per case in the order of GRADIENT_CASES: 1.10, 1.15, 1.00, 1.20, 1.88, 1.99, 2.33, 1.07
    (profiles/speedup_train.md names the tensors)."""
    c = _gradient_case(name)
    mean_net, var_net = c["nets"]
    trainer = training.MCSpeedupTrainer(weights=c["weights"], mean_net=mean_net, var_net=var_net)
    got = trainer.gradients(c["data"], phase=c["phase"])
    trainer.close()
    rep = trainer.last_report
    for key in ("loss", "l1_loss", "gaussian_nll_loss", "psnr_before", "psnr_after"):
        assert abs(rep[key] - c["metrics"][key]) <= 1e-3 * max(1.0, abs(c["metrics"][key])), key
    net = "mean_net" if c["phase"] == "mean" else "var_net"
    normed = set(ref.normed_biases(got))
    worst = (0.0, None)
    for tensor, g in got.items():
        if not tensor.startswith(net) or tensor in normed:
            assert not g.any(), tensor
            continue
        yard, err = _rel_l2(c["g32"][tensor], c["g64"][tensor]), _rel_l2(g, c["g64"][tensor])
        print(f"gradient {name} {tensor}: error {err:.3g}, yardstick {yard:.3g}, ratio {err / yard:.3g}")
        worst = max(worst, (err / yard, tensor))
    print(f"gradient {name}: largest ratio {worst[0]:.3g} at {worst[1]}")
    assert worst[0] <= 4.0


def test_batch_gradient_is_the_sum_of_its_samples_and_repeats_bit_for_bit(engine):
    """A sample's backward pass does not depend on the batch it is in; its share 1 / B is applied where its gradient is rounded to
    float32 and added to the batch's.  So (a) two calls give the same bytes; (b) the gradient of the batch of 3 of the gradient
    cases equals the sum of its single-sample gradients, each a third, within 4 float32 spacings of the largest term; (c) with a batch
    of 4 the share is a power of two, a term is the single-sample gradient's bytes with the exponent lowered, and the batch equals
    ((g0 + g1) + g2) + g3 added in float32 in that order bit for bit, which another order of the samples does not give.

    Measured on the MI355X: (b) largest deviation 3.33 spacings of the largest term; (c) equal; 5441 of 25914 elements differ when
    the float32 sum is taken in the reverse order."""
    c = _gradient_case("2-2-8_64x80_b3_mean")
    mean_net, var_net = c["nets"]
    trainer = training.MCSpeedupTrainer(weights=c["weights"], mean_net=mean_net, var_net=var_net)
    three = trainer.gradients(c["data"], phase="mean")
    again = trainer.gradients(c["data"], phase="mean")
    singles = [trainer.gradients({k: v[p:p + 1] for k, v in c["data"].items()}, phase="mean") for p in range(3)]
    lp, fp = speedup_ref.seeded_inputs(17, 4, 32, 48)
    four_data = {"low_photon": lp, "forward_projection": fp, "high_photon": lp + np.float32(0.3) * np.sign(fp - np.float32(2.5))}
    four = trainer.gradients(four_data, phase="mean")
    four_singles = [trainer.gradients({k: v[p:p + 1] for k, v in four_data.items()}, phase="mean") for p in range(4)]
    trainer.close()
    worst, reordered, total = 0.0, 0, 0
    for tensor, g in three.items():
        assert g.tobytes() == again[tensor].tobytes()
        terms = np.stack([s[tensor].astype(np.float64) / 3.0 for s in singles])
        if terms.any():
            worst = max(worst, (np.abs(g - terms.sum(axis=0)) / _spacing(np.abs(terms).max(axis=0))).max())
        quarter = [s[tensor] * np.float32(0.25) for s in four_singles]
        assert all(np.array_equal(q.astype(np.float64), s[tensor].astype(np.float64) / 4.0) for q, s in zip(quarter, four_singles))  # exact
        in_order = ((quarter[0] + quarter[1]) + quarter[2]) + quarter[3]
        assert in_order.dtype == np.float32 and four[tensor].tobytes() == in_order.tobytes(), tensor
        reverse = ((quarter[3] + quarter[2]) + quarter[1]) + quarter[0]
        reordered += int(np.count_nonzero(reverse != in_order))
        total += in_order.size
    print(f"batch of 3: largest deviation from the sum of the single-sample gradients {worst:.3g} spacings of the largest term; "
          f"batch of 4: {reordered} of {total} elements differ in the reverse order")
    assert worst <= 4.0
    assert reordered > 0  # the order of the samples is visible in the bytes


# ------------------------------------------------------------------------------------------------------------------- training
def _fixed_batch():
    y, x = np.mgrid[0:32, 0:48].astype(np.float64)
    t = np.stack([2.5 + np.sin(x / 7.0 + p) * np.cos(y / 5.0) for p in (0.0, 1.0)])
    lp = t + np.random.default_rng(11).normal(0.0, 0.3, size=t.shape)
    return {"low_photon": lp.astype(np.float32), "forward_projection": (3.0 * t + 1.0).astype(np.float32), "high_photon": t.astype(np.float32)}


@pytest.fixture(scope="module")
def trained(engine):
    """41 updates of the mean net, then 20 of the variance net, on one fixed batch; golden architecture, initialisation of seed 0."""
    data = _fixed_batch()
    trainer = training.MCSpeedupTrainer(seed=0, n_pretrain_steps=41)
    start = trainer.state_dict()
    first = trainer.validate_on_batch(data)
    grads = trainer.gradients(data)
    mean_losses = [trainer.train_on_batch(data) for _ in range(1)]
    after_one = trainer.state_dict()
    mean_losses += [trainer.train_on_batch(data) for _ in range(40)]
    after_mean = trainer.state_dict()
    predicted = [trainer.predict(data["low_photon"], data["forward_projection"])]
    var_losses = [trainer.train_on_batch(data) for _ in range(20)]
    predicted.append(trainer.predict(data["low_photon"], data["forward_projection"]))
    return dict(predicted=predicted, trainer=trainer, data=data, start=start, first=first, grads=grads, after_one=after_one, mean=mean_losses, after_mean=after_mean,
                var=var_losses, end=trainer.state_dict())


def test_mean_stage_learns_the_fixed_batch(engine, trained):
    """loss[0] equals the float64 restatement's within the forward's tolerance (4 x the float32 CPU error of the restatement's
    mean, which bounds the error of a mean of |m - t|); after 41 updates at 1e-3 the L1 loss is below a quarter of where it began and,
    over the last 11, below the L1 distance of the input itself.

    Measured on the MI355X: loss[0] 2.02919 (restatement 2.02918), loss[40] 0.1557, min(loss[30:41]) 0.1557, the input's own L1 0.2393
    (torch on the CPU from the same initialisation: float64 0.1910 / 0.1771, float32 0.2088 / 0.2064)."""
    data, losses = trained["data"], [m["loss"] for m in trained["mean"]]
    assert all(m["loss"] == m["l1_loss"] for m in trained["mean"])
    weights = {k: v for k, v in trained["start"].items()}
    m64, _ = ref.mean_and_variance(weights, data["low_photon"], data["forward_projection"])
    m32, _ = ref.mean_and_variance(weights, data["low_photon"], data["forward_projection"], dtype=torch.float32)
    want = np.abs(m64 - data["high_photon"]).mean()
    own = np.abs(data["low_photon"].astype(np.float64) - data["high_photon"]).mean()
    print(f"training: loss[0] {losses[0]:.6g} (restatement {want:.6g}), loss[40] {losses[40]:.4g}, min(loss[30:41]) {min(losses[30:41]):.4g}, "
          f"the input's own L1 {own:.4g}")
    assert trained["first"]["loss"] == losses[0]  # validation changes nothing and sees what the first update sees
    assert abs(losses[0] - want) <= 4 * np.abs(m32 - m64).max()
    assert losses[40] < 0.25 * losses[0]
    assert min(losses[30:41]) < own
    assert abs(trained["first"]["psnr_before"] - ref.psnr(data["low_photon"], data["high_photon"])) < 1e-6
    assert abs(trained["first"]["psnr_after"] - ref.psnr(m64, data["high_photon"])) < 1e-3


def test_variance_stage_lowers_the_nll_and_leaves_the_mean_net_alone(engine, trained):
    """The reported NLL falls, and so does the part of it that the variance net can move: after the 41 updates the mean is clipped to
    0 at a few pixels, where v is the floor 1e-6, (m - t)^2 / v is some 1e6 and no gradient reaches the variance net.  Those pixels
    dominate the reported sum, so the NLL over the pixels with v above the floor is computed from the trainer's own forward before and
    after the 20 updates and must fall too.

    Measured on the MI355X: reported NLL 78189.7139 -> 78189.2731; over the 96.3 % of pixels above the floor -0.9233 -> -1.4044."""
    nll = [m["gaussian_nll_loss"] for m in trained["var"]]
    t = trained["data"]["high_photon"]
    free = []
    for mean, variance in trained["predicted"]:
        above = variance > np.float32(1e-6)
        assert above.mean() > 0.5
        free.append(ref.nll_loss(mean[above], variance[above], t[above])[0])
    assert abs(ref.nll_loss(*trained["predicted"][0], t)[0] / nll[0] - 1.0) < 1e-6  # the report's NLL is that of this forward
    assert np.array_equal(trained["predicted"][0][0], trained["predicted"][1][0])  # the mean did not move
    print(f"training: NLL {nll[0]:.12g} -> {nll[-1]:.12g}; over the {100 * above.mean():.1f} % of pixels above the floor {free[0]:.6g} -> {free[1]:.6g}")
    assert all(m["loss"] == m["gaussian_nll_loss"] for m in trained["var"])
    assert nll[-1] < nll[0]
    assert free[1] < free[0]
    normed = set(ref.normed_biases(trained["end"]))
    for name, w in trained["end"].items():
        same = w.tobytes() == trained["after_mean"][name].tobytes()
        assert same == (not name.startswith("var_net") or name in normed), name
    assert trained["trainer"].last_report["step"] == 61


def test_first_update_is_adam_applied_to_the_device_gradient(engine, trained):
    """Within 2 spacings of numpy Adam on gradients(); the variance net and the biases of normed convolutions do not move."""
    normed = set(ref.normed_biases(trained["start"]))
    for name, w0 in trained["start"].items():
        w1 = trained["after_one"][name]
        if name == "var_scale" or name.startswith("var_net") or name in normed:
            assert w1.tobytes() == w0.tobytes(), name
            continue
        want, _, _ = ref.adam(w0, trained["grads"][name], 0.0 * w0, 0.0 * w0, 1, 1e-3)
        assert np.all(np.abs(w1 - want) <= 2 * _spacing(want)), name
        assert not np.array_equal(w1, w0), name


def test_validation_changes_nothing_and_a_split_run_equals_a_whole_one(engine, tmp_path):
    nets = dict(mean_net=(2, 2, 8), var_net=(1, 2, 8))
    data = _fixed_batch()
    whole = training.MCSpeedupTrainer(seed=3, n_pretrain_steps=3, **nets)
    before = whole.state_dict()
    a = whole.validate_on_batch(data)
    assert all(v.tobytes() == before[k].tobytes() for k, v in whole.state_dict().items()) and whole.i_step == 0
    assert a == whole.validate_on_batch(data)
    run = [whole.train_on_batch(data) for _ in range(5)]  # three updates of the mean net, two of the variance net
    split = training.MCSpeedupTrainer(seed=3, n_pretrain_steps=3, **nets)
    first = [split.train_on_batch(data) for _ in range(3)]
    split.save_checkpoint(tmp_path / "check.npz")
    split.close()
    resumed = training.MCSpeedupTrainer(seed=99, n_pretrain_steps=3, **nets)
    resumed.load_checkpoint(tmp_path / "check.npz")
    second = [resumed.train_on_batch(data) for _ in range(2)]
    assert first + second == run
    end, end2 = whole.state_dict(), resumed.state_dict()
    assert all(end[k].tobytes() == end2[k].tobytes() for k in end)
    assert whole._moment1.tobytes() == resumed._moment1.tobytes() and whole._moment2.tobytes() == resumed._moment2.tobytes()
    assert whole._lr == resumed._lr and whole._steps == resumed._steps == [3, 2]
    assert abs(whole._lr - 1e-3 * 0.99999 ** 2) < 1e-18  # set back to 1e-3 at the switch to the variance stage


def test_a_handle_made_anew_for_a_larger_batch_carries_the_whole_state(engine):
    """Trainer A takes two updates at batch 1, then one at batch 2: the larger batch closes the handle (state to the host), makes one
    for batches of 2 and pushes the state into it.  Trainer B validates a batch of 2 first, so its one handle serves all three updates.
    A sample's backward pass does not depend on the batch it is in and validation changes nothing (both asserted above), so A and B
    end with the same bytes: weights, both moments, step counts, learning rate.  n_pretrain_steps = 2: the third update is also the
    first of the variance net."""
    nets = dict(mean_net=(2, 1, 4), var_net=(1, 1, 4))
    lp, fp = speedup_ref.seeded_inputs(5, 2, 8, 12)
    data = {"low_photon": lp, "forward_projection": fp, "high_photon": lp + np.float32(0.3) * np.sign(fp - np.float32(2.5))}
    one = {k: v[:1] for k, v in data.items()}
    a, b = (training.MCSpeedupTrainer(seed=4, n_pretrain_steps=2, **nets) for _ in range(2))
    b.validate_on_batch(data)
    runs, sizes = [], []
    for t in (a, b):
        metrics = []
        for batch in (one, one, data):
            metrics.append(t.train_on_batch(batch))
            sizes.append(t._shape[0])
        runs.append(metrics)
    assert sizes == [1, 1, 2, 2, 2, 2]  # A's handle was made anew, B's was not
    assert runs[0] == runs[1]
    end_a, end_b = a.state_dict(), b.state_dict()
    assert all(end_a[k].tobytes() == end_b[k].tobytes() for k in end_a)
    assert a._moment1.tobytes() == b._moment1.tobytes() and a._moment2.tobytes() == b._moment2.tobytes()
    assert a._moment1.any() and a._moment2.any()
    assert a._steps == b._steps == [2, 1] and a._lr == b._lr and a.i_step == b.i_step == 3
    a.close()
    b.close()


def test_saved_weights_predict_what_the_trainer_validated(engine, trained, tmp_path):
    trainer, data = trained["trainer"], trained["data"]
    mean, variance = trainer.predict(data["low_photon"], data["forward_projection"])
    metrics = trainer.validate_on_batch(data)
    assert abs(metrics["l1_loss"] - np.abs(mean.astype(np.float64) - data["high_photon"]).mean()) < 1e-9
    for suffix in (".npz", ".pth"):
        model = speedup.MCSpeedup.from_filepath(trainer.save(tmp_path / ("trained" + suffix)))
        m2, v2 = model.predict(data["low_photon"], data["forward_projection"])
        assert m2.tobytes() == mean.tobytes() and v2.tobytes() == variance.tobytes()


def test_one_update_at_full_size(engine):
    """1024 x 768, batch 1, golden architecture: a finite loss and the peak of the device memory.
    Measured on the MI355X: peak_device_bytes 4,022,890,280 (3837 MiB); ms_forward 11.9, ms_wgrad 22.3, ms_dgrad 11.8, ms_norm 2.6,
    ms_optimizer 0.25, ms_total 49.6 (warm medians at the batch of 10: profiles/speedup_train.md)."""
    lp, fp = speedup_ref.seeded_inputs(4, 1, 768, 1024)
    trainer = training.MCSpeedupTrainer(seed=0)
    metrics = trainer.train_on_batch({"low_photon": lp, "forward_projection": fp, "high_photon": lp + np.float32(0.25)})
    rep = dict(trainer.last_report)
    trainer.close()
    print("full size update:", metrics, rep)
    assert all(np.isfinite(v) for v in metrics.values())
    assert rep["peak_device_bytes"] > 4 * 4 * 13_401_586 and rep["step"] == 1
    for key in ("ms_forward", "ms_wgrad", "ms_dgrad", "ms_norm", "ms_optimizer", "ms_total"):
        assert rep[key] > 0, key
