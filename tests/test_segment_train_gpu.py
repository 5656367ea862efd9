"""Training of the segmentation network on the MI355X (csrc/segment_train.hip through mcgpu_segment_train_*): every new backward
operator against float64, the whole gradient against float64 autograd of the restatement (segment_train_ref.py) with torch's float32
CPU run of the same restatement as the yardstick, short training runs, checkpoints, saved weights and one update at the driver's
patch."""
import numpy as np
import pytest

import cases
import segment_ref
import segment_train_ref as ref

torch = pytest.importorskip("torch")

seg = cases.pkg.segmentation
training = cases.pkg.segmentation_training
stage = training.segment_train_stage
pytestmark = pytest.mark.gpu

CONV_PAIRS = [((1, 0), 5), ((3, 0), 9), ((33, 0), 34), ((4, 6), 4), ((32, 32), 32)]  # ((c1, c2 upsampled), c_out)
EVEN_SHAPES = [(2, 2, 2), (2, 6, 34), (4, 10, 66)]  # one window; one past the 4 x 32 tile on d1 and d2; several tiles, ragged
ODD_SHAPE = (3, 5, 7)                               # only for the pairs without upsample
CONV_CASES = [(p, s) for p in CONV_PAIRS for s in EVEN_SHAPES + ([ODD_SHAPE] if not p[0][1] else [])]
_conv_id = lambda v: "x".join(map(str, v)) if len(v) == 3 else f"{v[0][0]}+{v[0][1]}to{v[1]}"  # noqa: E731


def _spacing(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _conv_case(rng, c1, c2, c_out, shape, integers):
    draw = (lambda lo, hi, size: rng.integers(lo, hi + 1, size=size).astype(np.float32)) if integers else \
        (lambda lo, hi, size: rng.uniform(lo, hi, size=size).astype(np.float32))
    x1 = draw(-3, 3, (c1,) + shape)
    x2 = draw(-3, 3, (c2,) + tuple((v + 1) // 2 for v in shape)) if c2 else None
    w = draw(-8, 8, (c_out, c1 + c2, 3, 3, 3)) if integers else draw(-1, 1, (c_out, c1 + c2, 3, 3, 3))
    dy = draw(-3, 3, (c_out,) + shape)
    return x1, x2, w, dy


def _conv_run(x1, x2, w, dy, c1):
    (dw, db, partials), _ = stage("conv_wgrad", x1, in2=x2, in3=dy, upsample=x2 is not None)
    (d1, d2), _ = stage("conv_dgrad", dy, in2=w, c1=c1, upsample=x2 is not None)
    return dw, db, partials, d1, d2


# --------------------------------------------------------------------------------------------------------------- convolution
@pytest.mark.parametrize("pair,shape", CONV_CASES, ids=_conv_id)
def test_conv_gradients_of_small_integers_are_bit_equal_to_float64(engine, pair, shape):
    """|x|, |dy| <= 3 and |w| <= 8, unrelated across channels, taps and voxels: every sum is an integer below 2^24 (asserted), exact
    in float32 in any order, so both gradients equal float64 bit for bit; a slip in a lane map, the tap flip, the dz of the grid, the
    zero mask, the split of the sources, the 2 x 2 x 2 sum or the order of the partials gives a wrong integer."""
    (c1, c2), c_out = pair
    x1, x2, w, dy = _conv_case(np.random.default_rng(c1 * 1000 + c_out + shape[2]), c1, c2, c_out, shape, integers=True)
    dw, db, partials, d1, d2 = _conv_run(x1, x2, w, dy, c1)
    want_w, want_b, want1, want2 = ref.conv_gradients(x1, x2, bool(c2), w, dy)
    bound_w, _, bound1, bound2 = ref.conv_gradients(np.abs(x1), None if x2 is None else np.abs(x2), bool(c2), np.abs(w), np.abs(dy))
    assert bound_w.max() < 2 ** 24 and bound1.max() < 2 ** 24 and (bound2 is None or bound2.max() < 2 ** 24) and partials >= 4
    assert np.array_equal(dw.astype(np.float64), want_w) and np.array_equal(db.astype(np.float64), want_b)
    assert np.array_equal(d1.astype(np.float64), want1)
    assert (d2 is None and want2 is None) or np.array_equal(d2.astype(np.float64), want2)


@pytest.mark.parametrize("pair,shape", CONV_CASES, ids=_conv_id)
def test_conv_gradients_of_float_data_are_within_the_bound_of_a_float32_fma_chain(engine, pair, shape):
    """Weight gradient: |got - float64| <= (voxels + partials) 2^-24 x (the same gradient of |x|, |dy|); input gradient: <= (27 C_out
    + 1) 2^-24 x (the same gradient of |dy|, |w|), and 8 more terms for the second source, whose 2 x 2 x 2 block is summed.

    Measured on the MI355X, largest error / bound over all cases: weight gradient 0.121 (32 + 32 -> 32 at 2 x 2 x 2, 8 partials; 9e-5 at
    4 x 10 x 66), input gradient 0.0147 (4 + 6 -> 4 at 4 x 10 x 66: the shortest chains)."""
    (c1, c2), c_out = pair
    x1, x2, w, dy = _conv_case(np.random.default_rng(c1 * 1000 + c_out + shape[1]), c1, c2, c_out, shape, integers=False)
    dw, _, partials, d1, d2 = _conv_run(x1, x2, w, dy, c1)
    want_w, _, want1, want2 = ref.conv_gradients(x1, x2, bool(c2), w, dy)
    bound_w, _, bound1, bound2 = ref.conv_gradients(np.abs(x1), None if x2 is None else np.abs(x2), bool(c2), np.abs(w), np.abs(dy))
    voxels = shape[0] * shape[1] * shape[2]
    excess_w = (np.abs(dw - want_w) / ((voxels + partials) * 2.0 ** -24 * bound_w)).max()
    excess_d = (np.abs(d1 - want1) / ((27 * c_out + 1) * 2.0 ** -24 * bound1)).max()
    if c2:
        excess_d = max(excess_d, (np.abs(d2 - want2) / ((27 * c_out + 1 + 8) * 2.0 ** -24 * bound2)).max())
    print(f"conv gradients {pair} {shape}: max error / bound = {excess_w:.3g} (weights, {partials} partials), {excess_d:.3g} (input)")
    assert excess_w <= 1.0 and excess_d <= 1.0


def test_weight_gradient_at_the_drivers_extent_indexes_every_tile(engine):
    """dec_0's first convolution at the driver's patch: 32 skip channels and 32 upsampled ones in, 32 out, 384 x 384 x 64.  X = 1
    everywhere and dY = small integers that depend on position and channel, so dW[co][ci][tap] = the sum of dY[co] over the voxels
    whose tap neighbour lies inside: three ranges per axis, the same for every ci.  The partials are float32 sums of fewer than 2^24
    ones in magnitude (exact), folded in float64 and rounded once: bit-equal to the float32 of the float64 slice sums."""
    D = (384, 384, 64)
    x1 = np.ones((32,) + D, np.float32)
    x2 = np.ones((32,) + tuple(v // 2 for v in D), np.float32)
    z, y, x = np.ogrid[0:D[0], 0:D[1], 0:D[2]]
    base = 3 * z * z + 5 * y + x * x + (z * y) // 7  # not periodic along any axis: the three ranges of an axis give three sums
    dy = np.empty((32,) + D, np.float32)
    for co in range(32):
        dy[co] = (base + co * (x + 1)) % 7 - 3 + ((z * (co + 1) + y + x) % (5 + co) == 0)
    (dw, db, partials), rep = stage("conv_wgrad", x1, in2=x2, in3=dy, upsample=True)
    assert dw.shape == (32, 64, 3, 3, 3) and partials >= 4 * 64
    s = dy.astype(np.float64)
    along2 = np.stack([s.sum(3) - s[..., 0], s.sum(3), s.sum(3) - s[..., -1]], axis=-1)                            # [co][z][y][dx]
    along1 = np.stack([along2.sum(2) - along2[:, :, 0], along2.sum(2), along2.sum(2) - along2[:, :, -1]], axis=-2)  # [co][z][dy][dx]
    want = np.stack([along1.sum(1) - along1[:, 0], along1.sum(1), along1.sum(1) - along1[:, -1]], axis=1)           # [co][dz][dy][dx]
    assert len(np.unique(want[:, 1, 1, 1])) == 32 and min(len(np.unique(w)) for w in want) >= 18  # channels and taps are told apart
    assert np.array_equal(dw, np.broadcast_to(want[:, None], dw.shape).astype(np.float32))
    assert np.array_equal(db, want[:, 1, 1, 1].astype(np.float32))
    assert rep["ms_wgrad"] > 0
    print(f"weight gradient 32+32 -> 32 at {D}: {partials} partials, {rep['ms_wgrad']:.1f} ms with its fold and bias sums")


# ------------------------------------------------------------------------------------------------------------ pool and loss
@pytest.mark.parametrize("shape", [(1, 2, 2, 2), (3, 6, 10, 4), (5, 16, 32, 64)], ids=lambda s: "x".join(map(str, s)))
def test_maxpool_backward_is_bit_equal_ties_included(engine, shape):
    rng = np.random.default_rng(1)
    x = rng.integers(0, 3, size=shape).astype(np.float32)  # three values: most windows hold a tie
    dy = rng.normal(size=(shape[0],) + tuple(v // 2 for v in shape[1:])).astype(np.float32)
    want = ref.maxpool_backward(x, dy)
    got, _ = stage("maxpool_backward", x, in2=dy)
    assert np.array_equal(got.astype(np.float64), want)
    before = rng.normal(size=shape).astype(np.float32)  # what the decoder left in the skip's gradient
    added, _ = stage("maxpool_backward", x, in2=dy, in3=before)
    assert np.array_equal(added, before + want.astype(np.float32))
    y = rng.normal(size=shape).astype(np.float32)
    assert np.array_equal(stage("maxpool_backward", y, in2=dy)[0].astype(np.float64), ref.maxpool_backward(y, dy))


def _loss_cases():
    with np.load(ref.GOLDEN / "segment_train_pin.npz") as g:
        golden = (g["logits"].astype(np.float32), g["target"])
    rng = np.random.default_rng(4)
    shape = (16, 16, 32)
    logits = rng.normal(0.0, 2.0, size=(2, 9) + shape).astype(np.float32)
    target = np.stack([ref.seeded_target(5, shape), ref.seeded_target(6, shape, absent=0)])
    return {"golden": golden, "16x16x32_b2": (logits, target)}


@pytest.mark.parametrize("name", ["golden", "16x16x32_b2"])
def test_loss_and_head_gradient_equal_the_restatement(engine, name):
    """Every f within 4 x 2^-24 absolute (p is rounded once to float32 and the sums are float64, so I and P are each relatively
    within 2^-24, the ratio within twice that, plus the final rounding; f <= 1); the gradient within 2 spacings of the float32 value.

    Measured on the MI355X: largest |f - float64| 1.17e-9 (golden) and 4.4e-10 (16 x 16 x 32), 0.02 x 2^-24; gradient within 0.5
    spacings in both."""
    logits, target = _loss_cases()[name]
    (loss, f, g), _ = stage("loss", logits, in2=target)
    want_f = ref.dice_f(torch.as_tensor(logits, dtype=torch.float64), torch.as_tensor(target, dtype=torch.float64)).numpy()
    want_g = ref.head_gradient(logits, target)
    err_f = np.abs(f - want_f).max()
    err_g = (np.abs(g - want_g) / _spacing(want_g)).max()
    print(f"loss {name}: max |f - f64| = {err_f:.3g} ({err_f * 2.0 ** 24:.3g} x 2^-24), gradient within {err_g:.3g} spacings")
    assert err_f <= 4 * 2.0 ** -24 and abs(loss - want_f.mean()) <= 4 * 2.0 ** -24
    assert err_g <= 2.0
    if name == "golden":
        with np.load(ref.GOLDEN / "segment_train_pin.npz") as gold:
            assert np.abs(f - gold["f"]).max() <= 1e-6  # float32 logits here, float64 there


# ------------------------------------------------------------------------------------------------------------- whole gradient
# filters, levels, patch, seed of the image.  A LeakyReLU slope or a max-pool winner that float32 rounding decides otherwise than float64
# moves the gradient of a whole tensor by per cent, in any float32 implementation (one-ulp changes of the input do it to torch's CPU
# float32 run of the 16 x 16 x 32 case with seed 7: 2e-6 <-> 1.4e-2 on dec_1.convs.3.weight).  With the reference's filters no image
# keeps every such decision clear of float32's own error (segment_train_ref.decision_margins: smallest |value| or gap over the largest
# float32 CPU error of its layer); the seeds of the two L = 4 cases are those with the widest such margin among 7 .. 457 (0.62 and
# 0.089; seed 7 has 0.088 and 0.0038), chosen from the restatement alone.
GRADIENT_CASES = {
    "L2_8x8x8": (ref.SMALL_FILTERS, 2, (8, 8, 8), 7),
    "L4_16x16x32": (segment_ref.REFERENCE_FILTERS, 4, (16, 16, 32), 408),
    "L4_32x32x32": (segment_ref.REFERENCE_FILTERS, 4, (32, 32, 32), 293),
}
_cases = {}


def _gradient_case(name):
    """Weights, one patch with its target, the float64 gradient and the float32 CPU yardstick; computed once."""
    if name not in _cases:
        filters, levels, shape, seed = GRADIENT_CASES[name]
        weights = segment_ref.seeded_weights(7, filters, levels)
        patch = segment_ref.rescale(segment_ref.seeded_image(seed, shape))
        target = ref.seeded_target(7, shape)
        loss, f, g64 = ref.gradients(weights, patch[None], target[None])
        _, _, g32 = ref.gradients(weights, patch[None], target[None], dtype=torch.float32)
        _cases[name] = dict(filters=filters, levels=levels, weights=weights, data={"image": patch[None, None], "segmentation": target[None]}, loss=loss, f=f,
                            g64=g64, g32=g32)
    return _cases[name]


def _rel_l2(a, b):
    return np.linalg.norm(np.asarray(a, np.float64).ravel() - b.ravel()) / np.linalg.norm(b.ravel())


def _normed_biases(names):
    return {n for n in names if n.endswith(".bias") and not n.startswith(("init_conv", "final_conv"))}


@pytest.mark.parametrize("name", list(GRADIENT_CASES))
def test_gradients_are_as_close_to_float64_autograd_as_the_float32_run_of_torch(engine, name):
    """Per tensor, the relative L2 error against float64 autograd of the restatement is at most 4 x that of torch's float32 CPU
    autograd of the same restatement; the biases of normed convolutions are exactly 0; the ten metrics equal the restatement's.

    Measured on the MI355X, largest ratio per case: 1.33 (init_conv.bias), 0.64 (enc_3.convs.3.weight), 0.51 (final_conv.weight; every
    other tensor of the 32 x 32 x 32 case is below 0.005, because torch's float32 run takes one decision differently than float64
    there and is 1e-3 away on them, the device 2e-6).  profiles/segment_train.md has the case with seed 7, which is not kept."""
    c = _gradient_case(name)
    trainer = training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"])
    got = trainer.gradients(c["data"])
    metrics = trainer.validate_on_batch(c["data"])
    trainer.close()
    assert abs(metrics["loss"] - c["loss"]) <= 1e-4
    for index, label in seg.LABELS.items():
        assert abs(metrics[f"loss_label_{label}"] - c["f"][0, index]) <= 1e-4, label
    normed, worst = _normed_biases(got), (0.0, None)
    assert len(normed) == 4 * c["levels"]
    for tensor, g in got.items():
        if tensor in normed:
            assert not g.any(), tensor
            continue
        yard, err = _rel_l2(c["g32"][tensor], c["g64"][tensor]), _rel_l2(g, c["g64"][tensor])
        print(f"gradient {name} {tensor}: error {err:.3g}, yardstick {yard:.3g}, ratio {err / yard:.3g}")
        worst = max(worst, (err / yard, tensor))
    print(f"gradient {name}: largest ratio {worst[0]:.3g} at {worst[1]}")
    assert worst[0] <= 4.0


def test_batch_of_three_is_the_sum_of_its_samples_and_repeats_bit_for_bit(engine):
    """A sample's backward pass does not depend on the batch it is in; its share 1 / 3 is applied where its gradient is rounded to
    float32 and added to the batch's: the batch gradient is within 4 float32 spacings (of the largest term) of the sum of its
    single-sample gradients, each a third, and two calls give the same bytes; the metrics are the means over the samples.

    Measured on the MI355X: largest deviation 4.0000 spacings of the largest term, the issue's bound itself; the bytes repeat, so it
    does not move.  The sum can have 4 times the spacing of its largest term, so one unit in its last place reads as 4.0000; the
    worst case of three rounded terms and two additions is 5 (profiles/segment_train.md has the arithmetic)."""
    shape = (8, 8, 16)
    weights = segment_ref.seeded_weights(3, ref.SMALL_FILTERS, 2)
    images = np.stack([segment_ref.rescale(segment_ref.seeded_image(s, shape)) for s in (1, 2, 3)])
    targets = np.stack([ref.seeded_target(s, shape, absent=s) for s in (1, 2, 3)])
    trainer = training.CTSegmentationTrainer(weights=weights, **dict(n_filters=ref.SMALL_FILTERS, levels=2))
    data = {"image": images, "segmentation": targets}
    three = trainer.gradients(data)
    again = trainer.gradients(data)
    batch_metrics = trainer.validate_on_batch(data)
    singles, single_metrics = [], []
    for p in range(3):
        one = {"image": images[p:p + 1], "segmentation": targets[p:p + 1].astype(np.float32)}  # float32 targets give what uint8 ones give
        singles.append(trainer.gradients(one))
        single_metrics.append(trainer.validate_on_batch(one))
    trainer.close()
    worst = 0.0
    for tensor, g in three.items():
        assert g.tobytes() == again[tensor].tobytes()
        terms = np.stack([s[tensor].astype(np.float64) / 3.0 for s in singles])
        if terms.any():
            worst = max(worst, (np.abs(g - terms.sum(axis=0)) / _spacing(np.abs(terms).max(axis=0))).max())
    print(f"batch of 3: largest deviation from the sum of the single-sample gradients {worst:.4f} spacings of the largest term")
    assert worst <= 4.0
    for key in training.METRICS:
        assert abs(batch_metrics[key] - np.mean([m[key] for m in single_metrics])) <= 1e-15, key


# ------------------------------------------------------------------------------------------------------------------- training
def _flat(state):
    return np.concatenate([v.ravel() for v in state.values()])


def test_first_update_is_adams_float64_statement_on_the_devices_own_gradient(engine):
    c = _gradient_case("L2_8x8x8")
    trainer = training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"], lr=1e-3)
    grads = trainer.gradients(c["data"])
    before = trainer.state_dict()
    metrics = trainer.train_on_batch(c["data"])
    after = trainer.state_dict()
    trainer.close()
    assert metrics["learning_rate"] == 1e-3 and trainer.i_step == 1 and set(metrics) == set(training.METRICS) | {"learning_rate"}
    m1, m2 = {}, {}
    for name, g in grads.items():
        w, m1[name], m2[name] = ref.adam_step(before[name], g, np.zeros_like(g), np.zeros_like(g), 1, 1e-3)
        assert np.array_equal(after[name], w.astype(np.float32)), name
        if name in _normed_biases(grads):
            assert np.array_equal(after[name], before[name])
    assert np.array_equal(trainer._moment1, _flat(m1).astype(np.float32)) and np.array_equal(trainer._moment2, _flat(m2).astype(np.float32))
    assert np.count_nonzero(_flat(after) != _flat(before)) > 0.9 * (_flat(after).size - 4 * c["levels"] * 6)


@pytest.mark.parametrize("name", ["L2_8x8x8", "L4_16x16x32"])
def test_training_on_one_fixed_patch_lowers_the_loss(engine, name):
    """30 updates at lr 1e-3 from seeded_weights(7): the loss after the last update is below the first.  No closeness of
    trajectories is asserted; both are printed (profiles/segment_train.md records them beside the float64 restatement's).

    Measured on the MI355X: 0.8686 -> 0.7780 (restatement on the CPU: 0.8686 -> 0.7780) and 0.8699 -> 0.3419 (0.8699 -> 0.3398)."""
    c = _gradient_case(name)
    trainer = training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"], lr=1e-3)
    losses = [trainer.train_on_batch(c["data"])["loss"] for _ in range(30)]
    losses.append(trainer.validate_on_batch(c["data"])["loss"])
    trainer.close()
    print(f"training {name}: " + " ".join(f"{v:.4f}" for v in losses))
    restated = ref.train(c["weights"], c["data"]["image"][0, 0], c["data"]["segmentation"][0], 31, 1e-3)
    print(f"float64 restatement {name}: " + " ".join(f"{v:.4f}" for v in restated))
    assert abs(restated[0] - c["loss"]) <= 1e-12 and restated[-1] < restated[0]
    assert abs(losses[0] - c["loss"]) <= 1e-4 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]


def test_validation_changes_nothing_and_a_checkpoint_splits_a_run_bit_for_bit(engine, tmp_path):
    c = _gradient_case("L2_8x8x8")
    other = {"image": c["data"]["image"][:, :, ::-1].copy(), "segmentation": c["data"]["segmentation"][:, :, ::-1].copy()}
    batches = [c["data"], other] * 4
    make = lambda: training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"], lr=1e-3,  # noqa: E731
                                                  lr_scheduler=training.ReduceLROnPlateau(factor=0.5, patience=2, threshold=0.5, cooldown=1, min_lr=1e-6))
    whole = make()
    start = whole.state_dict()
    first = whole.validate_on_batch(c["data"])
    assert whole.validate_on_batch(c["data"]) == first and whole.i_step == 0
    assert all(np.array_equal(v, start[k]) for k, v in whole.state_dict().items())
    whole_metrics = [whole.train_on_batch(b) for b in batches]
    rates = [m["learning_rate"] for m in whole_metrics]
    assert rates[0] == 1e-3 and rates[-1] < 1e-3 and whole_metrics[0]["loss"] == first["loss"]  # the rate drops inside the run
    split = make()
    split_metrics = [split.train_on_batch(b) for b in batches[:5]]
    path = split.save_checkpoint(tmp_path / "run" / "checkpoint.npz")
    split.close()
    resumed = training.CTSegmentationTrainer(seed=99, n_filters=c["filters"], levels=c["levels"], lr=0.5)
    resumed.load_checkpoint(path)
    assert resumed.i_step == 5 and resumed.lr == split.lr and resumed.lr_scheduler.state_dict() == split.lr_scheduler.state_dict()
    split_metrics += [resumed.train_on_batch(b) for b in batches[5:]]
    assert split_metrics == whole_metrics
    a, b = whole.state_dict(), resumed.state_dict()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert whole._moment1.tobytes() == resumed._moment1.tobytes() and whole._moment2.tobytes() == resumed._moment2.tobytes()
    assert any(not np.array_equal(a[k], start[k]) for k in a)
    whole.close()
    resumed.close()


def test_a_handle_made_anew_for_a_larger_batch_carries_the_whole_state(engine):
    """Trainer A takes two updates at batch 1, then one at batch 2: the larger batch closes the handle (state to the host), makes one
    for batches of 2 and pushes the state into it.  Trainer B validates a batch of 2 first, so its one handle serves all three updates.
    A sample's backward pass does not depend on the batch it is in and validation changes nothing (both asserted above), so A and B
    end with the same bytes: weights, both moments, the step count and the learning rate."""
    c = _gradient_case("L2_8x8x8")
    one = c["data"]
    two = {"image": np.concatenate([one["image"], one["image"][:, :, ::-1]]), "segmentation": np.concatenate([one["segmentation"], one["segmentation"][:, :, ::-1]])}
    a, b = (training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"], lr=1e-3) for _ in range(2))
    b.validate_on_batch(two)
    runs, sizes = [], []
    for t in (a, b):
        metrics = []
        for batch in (one, one, two):
            metrics.append(t.train_on_batch(batch))
            sizes.append(t._shape[0])
        runs.append(metrics)
    assert sizes == [1, 1, 2, 2, 2, 2]  # A's handle was made anew, B's was not
    assert runs[0] == runs[1]
    end_a, end_b = a.state_dict(), b.state_dict()
    assert all(end_a[k].tobytes() == end_b[k].tobytes() for k in end_a)
    assert a._moment1.tobytes() == b._moment1.tobytes() and a._moment2.tobytes() == b._moment2.tobytes()
    assert a._moment1.any() and a._moment2.any()
    assert a.i_step == b.i_step == 3 and a.lr == b.lr == 1e-3
    assert a.last_report["step"] == b.last_report["step"] == 3  # the device's own count came through the hand-over
    a.close()
    b.close()


def test_saved_weights_load_with_the_segmenter_and_segment_gives_predict_plus_head(engine, tmp_path):
    c = _gradient_case("L2_8x8x8")
    trainer = training.CTSegmentationTrainer(weights=c["weights"], n_filters=c["filters"], levels=c["levels"], lr=1e-3)
    trainer.train_on_batch(c["data"])
    logits = trainer.predict(c["data"])
    assert logits.shape == (1, 9, 8, 8, 8) and np.array_equal(trainer.predict(c["data"]["image"]), logits)
    prob, _ = seg.segment_stage("head", logits[0])
    patch = c["data"]["image"][0, 0]
    for suffix in (".npz", ".pth"):
        path = trainer.save(tmp_path / f"step_1{suffix}")
        segmenter = seg.MCSegmenter.from_filepath(path, patch_shape=(8, 8, 8), input_value_range=(0, 1), output_value_range=(0, 1))
        assert segmenter.levels == 2 and tuple(segmenter.n_filters) == tuple(c["filters"])
        labels, raw = segmenter.segment(patch)
        assert np.array_equal(raw, prob)
        assert np.array_equal(labels, segment_ref.finalize(prob))
    trainer.close()


def test_driver_loop_writes_its_files(engine, tmp_path):
    c = _gradient_case("L2_8x8x8")
    volume = segment_ref.seeded_image(2, (12, 10, 9))
    merged = ref.seeded_target(2, (12, 10, 9))
    train = training.SegmentationDataset([volume], [merged], patch_shape=(8, 8, 8), patches_per_image=2, seed=1)
    test = training.SegmentationDataset([volume], [merged], patch_shape=(8, 8, 8), patches_per_image=1, random_rotation=False, add_noise=0.0,
                                        shift_image_values=None, seed=2)
    trainer, history = training.train_segmentation(train, test, steps=3, validation_interval=2, save_interval=2, run_folder=tmp_path / "run",
                                                   weights=c["weights"], n_filters=c["filters"], levels=c["levels"])
    assert [h["step"] for h in history] == [1, 2, 3] and history[0]["validation"] is None
    assert set(history[1]["validation"]) == set(training.METRICS) and history[2]["validation"] is not None
    assert isinstance(trainer.lr_scheduler, training.ReduceLROnPlateau) and trainer.lr == 1e-4
    models = tmp_path / "run" / "models" / "training"
    assert sorted(p.name for p in models.iterdir()) == ["checkpoint_2.npz", "checkpoint_3.npz", "step_2.npz", "step_2.pth", "step_3.npz", "step_3.pth"]
    assert seg.MCSegmenter.from_filepath(models / "step_3.pth").levels == 2
    trainer.close()


def test_one_update_at_the_drivers_patch(engine):
    """384 x 384 x 64 with the reference's filters: finite metrics, the peak of the device memory is the dry plan, and a following
    validation on the same patch gives another loss: the update moved the weights.

    Measured on the MI355X: loss 0.881573 -> 0.853288; the step takes 133 ms (forward 33, weight gradients 65, input gradients 23, norm
    12) and holds 10.63 GiB."""
    shape = (384, 384, 64)
    rng = np.random.default_rng(0)
    z, y, x = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    field = ((z // 48) + 2 * (y // 64) + (x // 16)) % 8
    image = (0.1 * field + 0.05 * rng.random(shape, dtype=np.float32)).astype(np.float32)
    target = np.zeros((9,) + shape, np.uint8)
    for c in range(8):
        target[c] = field == c
    target[8] = (field == 6) & ((z + y + x) % 3 == 0)
    data = {"image": image[None, None], "segmentation": target[None]}
    trainer = training.CTSegmentationTrainer(seed=0)
    planned = trainer.planned_device_bytes(1, shape)
    step = trainer.train_on_batch(data)
    rep = dict(trainer.last_report)
    after = trainer.validate_on_batch(data)
    trainer.close()
    print(f"update at {shape}: loss {step['loss']:.6f} -> {after['loss']:.6f}; forward {rep['ms_forward']:.0f} ms, wgrad {rep['ms_wgrad']:.0f}, dgrad "
          f"{rep['ms_dgrad']:.0f}, norm {rep['ms_norm']:.0f}, optimizer {rep['ms_optimizer']:.1f}, total {rep['ms_total']:.0f}; {planned / 2 ** 30:.2f} GiB")
    assert all(np.isfinite(v) for v in step.values()) and all(0.0 < step[k] <= 1.0 for k in training.METRICS)
    assert rep["peak_device_bytes"] == planned and rep["step"] == 1
    assert after["loss"] != step["loss"]
