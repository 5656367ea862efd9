"""Training of the segmentation network, the parts that need no GPU: the restated Dice loss and its closed-form gradient against
the reference's own DiceLoss (tests/golden/segment_train_pin.npz), the plateau scheduler against torch's, the dataset rule, the
dry planning mode, every refusal, and the ctypes mirrors against the header.

The three lines of the reference driver's SegmentationLoss (softmax over channels 0 .. 7, sigmoid on channel 8, then the Dice loss
per sample and channel) live in scripts/train_segmentation.py, which cannot be imported; they are restated in
tests/segment_train_ref.py: dice_f, and the golden was made with the reference's DiceLoss class on those two activations
(tests/gen_segment_train_golden.py)."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
import segment_ref
import segment_train_ref as ref

torch = pytest.importorskip("torch")

seg = cases.pkg.segmentation
training = cases.pkg.segmentation_training
recon = cases.pkg.reconstruction
ROOT = cases.ROOT

SMALL = dict(n_filters=ref.SMALL_FILTERS, levels=2)


# ------------------------------------------------------------------------------------------------------------------- the loss
def test_restated_loss_and_closed_form_gradient_equal_the_reference_class():
    with np.load(ref.GOLDEN / "segment_train_pin.npz") as g:
        logits, target, f, gradient = g["logits"], g["target"], g["f"], g["gradient"]
    assert logits.shape == (1, 9, 8, 8, 8) and target.dtype == np.uint8 and f.shape == (1, 9)
    assert not target[0, 5].any() and (target[0, 8] & target[0, 6]).any()  # one label absent, the vessels overlap the lung
    assert (target[0, :8].sum(0) == 1).all()
    mine = ref.dice_f(torch.as_tensor(logits), torch.as_tensor(target, dtype=torch.float64)).numpy()
    assert np.abs(mine - f).max() <= 1e-12
    assert 1.0 - 1e-6 < f[0, 5] <= 1.0  # nothing to intersect: only the smoothing keeps it from 1
    closed = ref.head_gradient(logits, target)
    assert np.abs(closed - gradient).max() <= 1e-12 and np.abs(gradient).max() > 1e-5
    # and the closed form is the autograd of the restatement, for a batch of 2 as well
    rng = np.random.default_rng(3)
    z = rng.normal(0.0, 1.5, size=(2, 9, 4, 6, 8))
    t = np.stack([ref.seeded_target(1, (4, 6, 8)), ref.seeded_target(2, (4, 6, 8), absent=2)])
    zt = torch.as_tensor(z).requires_grad_(True)
    ref.loss_of(zt, torch.as_tensor(t, dtype=torch.float64)).backward()
    assert np.abs(ref.head_gradient(z, t) - zt.grad.numpy()).max() <= 1e-15


def test_adam_statement_equals_the_2d_trainers():
    rng = np.random.default_rng(0)
    w, g, m, v = rng.normal(size=(4, 50))
    v = np.abs(v)
    for a, b in zip(ref.adam_step(w, g, m, v, 3, 1e-3), cases.pkg.speedup_training.adam_step(w, g, m, v, 3, 1e-3)):
        assert np.array_equal(a, b)


def test_decision_margins_of_the_small_case_are_wide():
    """The L = 2 case of the GPU tests takes no LeakyReLU slope and no max-pool winner within 4 x torch's float32 CPU error of being
    taken the other way (with the reference's filters no image does: the GPU tests' comment has the figures)."""
    layers, pools = ref.decision_margins(segment_ref.seeded_weights(7, ref.SMALL_FILTERS, 2), segment_ref.rescale(segment_ref.seeded_image(7, (8, 8, 8))))
    assert len(layers) == 8 and len(pools) == 2 and min(layers + pools) >= 4.0


# -------------------------------------------------------------------------------------------------------------- the scheduler
def _plateau_losses():
    """60 steps: a fall by more than the threshold, a plateau, gains below the threshold, a new fall, a long plateau to the floor."""
    out = [1.0, 0.9, 0.8, 0.7]                      # improvements > 1 %
    out += [0.7] * 6                                # plateau: patience 3 is exceeded on its 4th step, then cooldown 2
    out += [0.699, 0.698, 0.697, 0.696, 0.695]      # improvements < 1 % of the best: still bad steps
    out += [0.5, 0.4]                               # improvements > 1 %
    out += [0.4] * (60 - len(out))                  # plateau until min_lr holds
    return out


def test_plateau_scheduler_equals_torch_step_for_step():
    kw = dict(factor=0.5, patience=3, threshold=1e-2, cooldown=2, min_lr=2e-5)
    losses = _plateau_losses()
    assert len(losses) == 60
    param = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([param], lr=1e-4)
    theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", threshold_mode="rel", **kw)
    mine, lr, seen = training.ReduceLROnPlateau(**kw), 1e-4, []
    for loss in losses:
        theirs.step(loss)
        lr = mine.step(loss, lr)
        seen.append(lr)
        assert lr == opt.param_groups[0]["lr"], (len(seen), lr, opt.param_groups[0]["lr"])
        assert (mine.best, mine.num_bad_epochs, mine.cooldown_counter) == (theirs.best, theirs.num_bad_epochs, theirs.cooldown_counter)
    assert seen == ref.plateau(losses, 1e-4, **kw)
    assert seen[3] == 1e-4 and seen[-1] == 2e-5 and len(set(seen)) == 4  # 1e-4 -> 5e-5 -> 2.5e-5 -> the floor 2e-5
    # the driver's defaults, and a state that survives a round trip
    d = training.ReduceLROnPlateau()
    assert (d.factor, d.patience, d.threshold, d.cooldown, d.min_lr) == (0.9, 1000, 1e-2, 1000, 1e-6)
    again = training.ReduceLROnPlateau()
    again.load_state_dict(mine.state_dict())
    assert again.state_dict() == mine.state_dict() and isinstance(again.patience, int)
    with pytest.raises(ValueError, match="1.5"):
        training.ReduceLROnPlateau(factor=1.5)


# ---------------------------------------------------------------------------------------------------------------- the dataset
def _toy_segmentations(shape=(6, 5, 4)):
    rng = np.random.default_rng(5)
    label = rng.integers(0, 9, size=shape)  # 0: outside the body, 1 .. 6 the tissues, 7, 8: body without a tissue
    s = {"body": (label > 0).astype(np.uint8)}
    for i, name in enumerate(["upper_body_bones", "upper_body_muscles", "upper_body_fat", "liver", "stomach", "lung"], start=1):
        s[name] = (label == i).astype(np.uint8)
    s["lung_vessels"] = ((label == 6) & (rng.random(shape) < 0.5)).astype(np.uint8)
    return s, label


def test_merge_rule_on_a_toy_volume():
    s, label = _toy_segmentations()
    merged = training.merge_mc_segmentations(s)
    assert merged.dtype == np.uint8 and merged.shape == (9, 6, 5, 4)
    assert np.array_equal(merged, ref.merge(s))
    assert np.array_equal(merged[0], label == 0) and np.array_equal(merged[7], label >= 7)
    assert (merged[:8].sum(0) == 1).all()                       # background, six tissues and other partition the volume
    assert merged[8].any() and (merged[8] <= merged[6]).all()   # the vessels are an overlay on the lung, outside that union
    assert list(seg.LABELS.values())[7:] == ["other", "lung_vessels"]
    with pytest.raises(ValueError, match="'liver'"):
        training.merge_mc_segmentations({k: v for k, v in s.items() if k != "liver"})


def test_padding_values_and_patch_starts():
    s, _ = _toy_segmentations()
    merged = training.merge_mc_segmentations(s)
    image = np.full((6, 5, 4), 40, np.int16)
    data = training.SegmentationDataset([image], [merged], patch_shape=(8, 5, 8), random_rotation=False, add_noise=0.0, shift_image_values=None,
                                        patches_per_image=3, seed=1)
    items = list(data)
    assert len(items) == 3 and [it["i_patch"] for it in items] == [0, 1, 2]
    pads = ref.pad_widths((6, 5, 4), (8, 5, 8))
    assert pads == [(1, 1), (0, 0), (2, 2)]
    inside = (slice(1, 7), slice(0, 5), slice(2, 6))
    for it in items:
        assert it["patch_slicing"] == (slice(0, 8), slice(0, 5), slice(0, 8))  # the padded image is the patch: one start
        x, t = it["image"], it["segmentation"]
        assert x.shape == (1, 8, 5, 8) and x.dtype == np.float32 and t.shape == (9, 8, 5, 8) and t.dtype == np.float32
        outside = np.ones((8, 5, 8), bool)
        outside[inside] = False
        assert np.array_equal(x[0][outside], segment_ref.rescale(np.full(outside.sum(), -1000.0)))  # the image pads with -1000 HU
        assert np.array_equal(x[0][inside], segment_ref.rescale(image))
        assert (t[0][outside] == 1).all() and (t[1:, outside] == 0).all()  # background pads with 1, the others with 0
        assert np.array_equal(t[(slice(None),) + inside], merged.astype(np.float32))
    big = np.zeros((20, 9, 11), np.int16)
    onehot = np.zeros((9, 20, 9, 11), np.uint8)
    onehot[0] = 1
    data = training.SegmentationDataset([big], [onehot], patch_shape=(8, 8, 8), random_rotation=False, patches_per_image=40, seed=2)
    starts = np.array([[s.start for s in it["patch_slicing"]] for it in data])
    assert len(starts) == 40 and starts.min() == 0
    assert (starts.max(0) == (12, 1, 3)).all()  # every start of 0 .. N - P is reached, none beyond


def test_the_same_seed_gives_the_same_patches_and_rescale_is_the_segmenters():
    rng = np.random.default_rng(9)
    image = rng.integers(-1200, 3300, size=(12, 10, 9)).astype(np.int16)
    onehot = np.zeros((9, 12, 10, 9), np.uint8)
    onehot[1] = 1
    make = lambda seed: list(training.SegmentationDataset([image], [onehot], patch_shape=(8, 8, 8), patches_per_image=4, seed=seed))  # noqa: E731
    a, b, c = make(7), make(7), make(8)
    assert len(a) == 4
    for x, y in zip(a, b):
        assert x["patch_slicing"] == y["patch_slicing"] and np.array_equal(x["image"], y["image"]) and np.array_equal(x["segmentation"], y["segmentation"])
    assert any(not np.array_equal(x["image"], y["image"]) for x, y in zip(a, c))
    assert all(0.0 <= it["image"].min() and it["image"].max() <= 1.0 for it in a)
    values = rng.uniform(-1500.0, 3500.0, size=200)
    assert np.array_equal(training.rescale_range(values), segment_ref.rescale(values))
    plain = next(iter(training.SegmentationDataset([image], [onehot], patch_shape=(12, 10, 9), random_rotation=False, add_noise=0.0,
                                                   shift_image_values=None)))
    assert np.array_equal(plain["image"][0], segment_ref.rescale(image))


def test_balanced_sampling_stops_at_the_cap_when_a_label_is_absent():
    image = np.zeros((8, 8, 8), np.int16)
    onehot = np.zeros((9, 8, 8, 8), np.uint8)
    onehot[0] = 1  # background alone: the label drawn is absent whenever it is not 0
    data = training.SegmentationDataset([image], [onehot], patch_shape=(8, 8, 8), random_rotation=False, patches_per_image=3,
                                        force_balanced_sampling=True, seed=4)
    calls = []
    start = data.patch_start
    data.patch_start = lambda shape: calls.append(1) or start(shape)
    items = list(data)
    assert len(calls) == 30 and len(items) < 3  # 10 x patches_per_image attempts, then the image is given up
    full = np.ones((9, 8, 8, 8), np.uint8)
    data = training.SegmentationDataset([image], [full], patch_shape=(8, 8, 8), random_rotation=False, patches_per_image=3, force_balanced_sampling=True)
    assert len(list(data)) == 3


def test_dataset_reads_mha_files_and_refuses_foreign_spacings(tmp_path):
    s, _ = _toy_segmentations((6, 5, 4))
    image = np.arange(120, dtype=np.int16).reshape(6, 5, 4)
    recon.write_mha(tmp_path / "ct.mha", image.transpose(2, 1, 0), (1.0, 1.5, 2.0), (0, 0, 0), "MET_SHORT")
    paths = {}
    for name, a in s.items():
        paths[name] = recon.write_mha(tmp_path / f"{name}.mha", a.transpose(2, 1, 0), (1.0, 1.5, 2.0), (0, 0, 0), "MET_UCHAR")
    kw = dict(patch_shape=(6, 5, 4), random_rotation=False, add_noise=0.0, shift_image_values=None)
    item = next(iter(training.SegmentationDataset([tmp_path / "ct.mha"], [paths], image_spacing_range=((1.0, 1.0), (1.5, 1.5), (2.0, 2.0)), **kw)))
    assert np.array_equal(item["image"][0], segment_ref.rescale(image)) and item["image_spacing"] == (1.0, 1.5, 2.0)
    assert np.array_equal(item["segmentation"], training.merge_mc_segmentations(s).astype(np.float32))
    with pytest.raises(ValueError, match=r"\(1.0, 1.0\) on axis 1"):
        next(iter(training.SegmentationDataset([tmp_path / "ct.mha"], [paths], image_spacing_range=((1.0, 1.0),) * 3, **kw)))


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_initialisation_and_python_refusals():
    w = training.initial_weights(3)
    assert [(k, v.shape) for k, v in w.items()] == segment_ref.golden_tensors()
    for name, a in w.items():
        c_in = w[name.replace(".bias", ".weight")].shape[1]
        assert a.dtype == np.float32 and np.abs(a).max() <= 1.0 / np.sqrt(27.0 * c_in)
    assert np.array_equal(training.initial_weights(3)["final_conv.weight"], w["final_conv.weight"])
    assert training.METRICS[0] == "loss" and training.METRICS[9] == "loss_label_lung_vessels" and len(training.METRICS) == 10
    with pytest.raises(ValueError, match="single_segmentation='lung'"):
        training.CTSegmentationTrainer(single_segmentation="lung")
    with pytest.raises(ValueError, match="use_dice=False"):
        training.CTSegmentationTrainer(use_dice=False)
    with pytest.raises(ValueError, match="lr is -1.0"):
        training.CTSegmentationTrainer(lr=-1.0, **SMALL)
    with pytest.raises(ValueError, match="missing key"):
        training.CTSegmentationTrainer(weights={"init_conv.weight": np.zeros((4, 1, 3, 3, 3))}, **SMALL)
    t = training.CTSegmentationTrainer(seed=1, **SMALL)
    with pytest.raises(ValueError, match=r"\(1, 9, 8, 8, 8\)"):
        t._inputs({"image": np.zeros((1, 1, 8, 8, 8)), "segmentation": np.zeros((1, 8, 8, 8, 8))})
    with pytest.raises(ValueError, match=r"\(8, 8\)"):
        t._inputs({"image": np.zeros((8, 8)), "segmentation": None})


def test_dry_planning_returns_bytes_without_a_device(engine):
    small = training.CTSegmentationTrainer(seed=1, **SMALL)
    a, b = small.planned_device_bytes(1, (8, 8, 8)), small.planned_device_bytes(1, (16, 16, 16))
    assert 0 < a < b and small.planned_device_bytes(1, (8, 8, 8)) == a
    assert small.planned_device_bytes(3, (8, 8, 8)) - a == 2 * 9 * 8  # a larger batch holds only two more rows of f
    full = training.CTSegmentationTrainer(seed=1)
    n = 384 * 384 * 64
    # two sets of activations (3 full-size tensors of 32 channels and the 9 logits each), the target twice, the upsampled gradient
    assert 2 * (3 * 32 + 9) * 4 * n < full.planned_device_bytes(1, (384, 384, 64)) < 16 * 2 ** 30
    with pytest.raises(engine.EngineError, match=r"patch axis 2 is 12, not divisible by 16 \(2\^levels\)"):
        full.planned_device_bytes(1, (16, 16, 12))


def _options(flat, patch=(8, 8, 8), max_batch=2, levels=2, filters=ref.SMALL_FILTERS, n_classes=9, dry=1, n_weights=None, beta1=0.9):
    o = training._TrainOptions(struct_size=C.sizeof(training._TrainOptions), device=0, max_batch=max_batch, levels=levels, n_classes=n_classes, dry=dry,
                               weights=flat.ctypes.data if flat is not None else None, n_weights=flat.size if n_weights is None else n_weights,
                               beta1=beta1, beta2=0.999)
    o.patch_shape[:] = patch
    o.n_filters[:len(filters)] = filters
    return o


def test_abi_refusals_come_before_any_device_call(engine):
    """A planned (dry) handle touches no device: every refusal of a batch is reached on it, and only then the refusal to run."""
    lib = training._library()
    n = sum(int(np.prod(s)) for _, s in seg.unet_tensors(ref.SMALL_FILTERS, 2))
    flat = np.zeros(n, np.float32)

    def create_refused(o, text):
        h = C.c_void_p()
        assert lib.mcgpu_segment_train_create(C.byref(o) if o is not None else None, C.byref(h)) == -1 and not h.value
        assert text in lib.mcgpu_last_error().decode(), lib.mcgpu_last_error().decode()

    create_refused(None, "struct_size")
    create_refused(_options(None, n_weights=n), "weights is NULL")
    create_refused(_options(flat, n_weights=n - 1), f"n_weights is {n - 1} but the architecture has {n} values")
    create_refused(_options(flat, patch=(8, 10, 8)), "patch axis 1 is 10, not divisible by 4 (2^levels)")
    create_refused(_options(flat, patch=(4, 4, 4)), "the bottleneck of a 4 x 4 x 4 patch has fewer than 2 voxels")
    create_refused(_options(flat, patch=(8, 0, 8)), "patch_shape must be >= 1: 8 x 0 x 8")
    create_refused(_options(flat, patch=(2048, 2048, 1024)), "a patch of 2048 x 2048 x 1024 is too large")
    create_refused(_options(flat, max_batch=0), "max_batch is 0")
    create_refused(_options(flat, levels=9), "levels is 9, expected 1..8")
    create_refused(_options(flat, filters=(4, 4, 6, 6, 4, 0)), "n_filters[5] is 0")
    create_refused(_options(flat, filters=(4, 4, 6, 6, 4, 5)), "final_conv takes 5 channels but dec_0 gives 4")
    create_refused(_options(flat, n_classes=8), "the final convolution has 8 outputs, expected 9")
    create_refused(_options(flat, beta1=1.0), "beta1 and beta2 must be in [0, 1): 1.0")
    assert lib.mcgpu_segment_train_create(C.byref(_options(flat)), None) == -1

    handle = C.c_void_p()
    assert lib.mcgpu_segment_train_create(C.byref(_options(flat)), C.byref(handle)) == 0 and handle.value
    x = np.zeros((2, 8, 8, 8), np.float32)
    t = np.zeros((2, 9, 8, 8, 8), np.uint8)
    rep = training._TrainReport(struct_size=C.sizeof(training._TrainReport))
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def refused(text, h=handle, n=2, a=x, b=t, kind=0, lr=1e-4, update=1, report=rep, gradients=False):
        if gradients:
            rc = lib.mcgpu_segment_train_gradients(h, n, ptr(a), ptr(b), kind, None, C.byref(report))
        else:
            rc = lib.mcgpu_segment_train_step(h, n, ptr(a), ptr(b), kind, lr, update, C.byref(report) if report is not None else None)
        assert rc == -1
        assert text in lib.mcgpu_last_error().decode(), lib.mcgpu_last_error().decode()

    refused("handle is NULL", h=None)
    refused("n is 3 but the trainer was created for 1..2", n=3)
    refused("n is 0 but", n=0)
    refused("image is NULL", a=None)
    refused("target is NULL", b=None)
    refused("target_type 2", kind=2)
    refused("lr is 0.0", lr=0.0)
    refused("lr is nan", lr=float("nan"))
    refused("report->struct_size", report=training._TrainReport(struct_size=4))
    refused("flat_gradient is NULL", gradients=True)
    refused("dry plan")                   # everything in order: only now the handle says that it cannot run
    refused("dry plan", lr=0.0, update=0)  # a validation reads no learning rate
    assert lib.mcgpu_segment_train_predict(handle, 2, ptr(x), None) == -1 and "logits is NULL" in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_segment_train_predict(handle, 5, ptr(x), ptr(x)) == -1 and "n is 5" in lib.mcgpu_last_error().decode()
    state = training._TrainState(struct_size=C.sizeof(training._TrainState))
    assert lib.mcgpu_segment_train_get_state(handle, C.byref(state)) == 0
    assert state.n_weights == n and state.step == 0
    # the weights, two moments and the gradient; two sets of activations of an 8 x 8 x 8 patch
    assert 4 * 4 * n + 2 * 4 * 512 * (4 + 4 + 4 + 9) < state.planned_device_bytes < 16 * 2 ** 20
    state.weights, state.n_weights = flat.ctypes.data, n - 1
    assert lib.mcgpu_segment_train_get_state(handle, C.byref(state)) == -1 and f"the trainer has {n} values" in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_segment_train_set_state(handle, C.byref(state)) == -1
    assert lib.mcgpu_segment_train_get_state(handle, None) == -1 and "mcgpu_segment_train_state" in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_segment_train_destroy(handle) == 0 and lib.mcgpu_segment_train_destroy(None) == 0


def test_stage_refusals_come_before_any_device_call(engine):
    lib = training._library()
    buf = np.zeros(64, np.float32)
    values = np.zeros(16)
    p = buf.ctypes.data

    def args(shape=(2, 2, 2), **kw):
        a = training._TrainStageArgs(struct_size=C.sizeof(training._TrainStageArgs), **kw)
        a.shape[:] = shape
        return a

    for stage, a, text in [(7, args(in_=p, out=p, c1=1), "unknown stage 7"),
                           (0, args(in_=p, c1=1), "in or out is NULL"),
                           (0, args(shape=(2, 0, 2), in_=p, out=p, c1=1), "shape must be >= 1: 2 x 0 x 2"),
                           (2, args(in_=p, out=p, c1=1), "in2 is NULL"),
                           (0, args(in_=p, out=p, c1=1, c_out=1), "in2 or in3 is NULL"),
                           (0, args(in_=p, out=p, in3=p, c1=1, c2=1, c_out=1), "in2 or in3 is NULL"),
                           (0, args(in_=p, out=p, in3=p, c1=1, c2=-1, c_out=1), "c2 is -1"),
                           (1, args(in_=p, in2=p, out=p, c1=1, c2=1, c_out=1), "out2 is NULL"),
                           (2, args(in_=p, in2=p, out=p, c1=0), "c1 is 0"),
                           (3, args(in_=p, in2=p, out=p, n=1), "values is NULL"),
                           (3, args(in_=p, in2=p, out=p, values=values.ctypes.data, n=0), "n is not 1..65535")]:
        assert lib.mcgpu_segment_train_stage(stage, C.byref(a), None) == -1
        assert text in lib.mcgpu_last_error().decode(), (stage, lib.mcgpu_last_error().decode())
    assert lib.mcgpu_segment_train_stage(0, None, None) == -1
    assert "mcgpu_segment_train_stage_args" in lib.mcgpu_last_error().decode()


def test_ctypes_mirrors_match_the_c_layout(engine, tmp_path):
    """sizeof and every field offset of the four structs as a C compiler lays them out from the header."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    structs = {"mcgpu_segment_train_options": training._TrainOptions, "mcgpu_segment_train_report": training._TrainReport,
               "mcgpu_segment_train_state": training._TrainState, "mcgpu_segment_train_stage_args": training._TrainStageArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "mcgpu_amd.h"}"', "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(f'  printf("{cname} {field} %zu\\n", offsetof({cname}, {field.rstrip("_")}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    seen = 0
    for cname, field, value in re.findall(r"(\w+) (\w+) (\d+)", out):
        mirror = structs[cname]
        assert int(value) == (C.sizeof(mirror) if field == "sizeof" else getattr(mirror, field).offset), (cname, field)
        seen += 1
    assert seen == sum(len(m._fields_) + 1 for m in structs.values())
    header = (ROOT / "include" / "mcgpu_amd.h").read_text()
    for name, code in training.TRAIN_STAGES.items():
        assert f"MCGPU_SEGMENT_TRAIN_STAGE_{name.upper()} = {code}" in header
    assert "MCGPU_TARGET_UINT8 = 0, MCGPU_TARGET_FLOAT32 = 1" in header
    for name in ("create", "step", "gradients", "predict", "get_state", "set_state", "destroy", "stage"):
        assert f"mcgpu_segment_train_{name}" in engine.ABI_SYMBOLS
    assert "segmentation_training" in cases.pkg.__all__
