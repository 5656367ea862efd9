"""The CT segmentation network on the MI355X (csrc/segment_net.hip through mcgpu_segment_stage / mcgpu_segment_run): every operator
against float64 or its numpy statement, the whole network and the whole procedure against the float64 restatement (segment_ref.py,
chained to the reference class by golden/segment_pin.npz), and a CT file turned into a context's geometry through the segmenter.

Measured figures: profiles/segment_ab.md."""
import numpy as np
import pytest

import cases
import segment_ref

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

seg = cases.pkg.segmentation
geo = cases.geometry
recon = cases.pkg.reconstruction
pytestmark = pytest.mark.gpu

CONV_PAIRS = [((1, 0), 32), ((32, 0), 32), ((32, 32), 32), ((32, 0), 9), ((5, 3), 7)]  # ((c1, c2 read through the upsample), c_out)
CONV_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 2, 34), (6, 9, 40), (8, 8, 32)]  # one voxel, below a tile, past a tile along d2, ragged tiles, whole tiles


def _upsampled(a, shape):
    for axis in (1, 2, 3):
        a = np.repeat(a, 2, axis=axis)
    return a[:, :shape[0], :shape[1], :shape[2]]


def _conv64(x, w, b):
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    return F.conv3d(t(x)[None], t(w), t(b), padding=1)[0].numpy()


def _conv_case(rng, c1, c2, c_out, shape, integers):
    draw = (lambda lo, hi, size: rng.integers(lo, hi + 1, size=size).astype(np.float32)) if integers else \
        (lambda lo, hi, size: rng.uniform(lo, hi, size=size).astype(np.float32))
    x1 = draw(-3, 3, (c1,) + shape)
    x2 = draw(-3, 3, (c2,) + tuple((d + 1) // 2 for d in shape)) if c2 else None
    w = draw(-8, 8, (c_out, c1 + c2, 3, 3, 3)) if integers else draw(-1, 1, (c_out, c1 + c2, 3, 3, 3))
    b = draw(-9, 9, (c_out,))
    x = x1 if x2 is None else np.concatenate([x1, _upsampled(x2, shape)])
    return x1, x2, w, b, x


_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else f"{v[0][0]}+{v[0][1]}to{v[1]}")


@pytest.mark.parametrize("shape", CONV_SHAPES, **_ids)
@pytest.mark.parametrize("pair", CONV_PAIRS, **_ids)
def test_conv_of_small_integers_is_bit_equal_to_float64(engine, pair, shape):
    """Random integer inputs (|x| <= 3), weights (|w| <= 8, unrelated across c_out, c_in and tap) and biases: every partial sum is an
    integer below 27 x 64 x 24 + 9 < 2^24, exact in float32 in any order, so the output equals the float64 result bit for bit; a slip
    in the lane map, the tap order, the zero padding, the upsample or the order of the sources gives a wrong integer."""
    (c1, c2), c_out = pair
    x1, x2, w, b, x = _conv_case(np.random.default_rng(c1 * 1000 + c_out + shape[2]), c1, c2, c_out, shape, integers=True)
    got, _ = seg.segment_stage("conv", x1, in2=x2, weight=w, bias=b, upsample=bool(c2))
    want = _conv64(x, w, b)
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("shape", CONV_SHAPES, **_ids)
@pytest.mark.parametrize("pair", CONV_PAIRS, **_ids)
def test_conv_of_float_data_is_within_the_bound_of_a_float32_fma_chain(engine, pair, shape):
    """|got - float64| <= (27 C_in + 1) 2^-24 conv(|x|, |w|, |b|) per output: the bound of a float32 fma chain of 27 C_in products
    and the bias in any order."""
    (c1, c2), c_out = pair
    x1, x2, w, b, x = _conv_case(np.random.default_rng(c1 * 1000 + c_out + shape[1]), c1, c2, c_out, shape, integers=False)
    got, _ = seg.segment_stage("conv", x1, in2=x2, weight=w, bias=b, upsample=bool(c2))
    want = _conv64(x, w, b)
    bound = (27 * (c1 + c2) + 1) * 2.0 ** -24 * _conv64(np.abs(x), np.abs(w), np.abs(b))
    excess = np.abs(got - want) / bound
    print(f"conv {pair} {shape}: max error / bound = {excess.max():.3g}")
    assert excess.max() <= 1.0


@pytest.mark.parametrize("shape", [(6, 10, 12), (3, 5, 7), (8, 8, 32)], **_ids)
def test_identity_weights_give_the_concatenated_sources(engine, shape):
    """Centre tap of channel k -> output k, no bias: the output is cat(in, upsample(in2)) itself."""
    rng = np.random.default_rng(2)
    x1 = rng.normal(size=(2,) + shape).astype(np.float32)
    x2 = rng.normal(size=(5,) + tuple((d + 1) // 2 for d in shape)).astype(np.float32)
    w = np.zeros((7, 7, 3, 3, 3), np.float32)
    w[np.arange(7), np.arange(7), 1, 1, 1] = 1.0
    got, _ = seg.segment_stage("conv", x1, in2=x2, weight=w, bias=np.zeros(7, np.float32), upsample=True)
    assert np.array_equal(got, np.concatenate([x1, _upsampled(x2, shape)]))


def test_conv_reads_past_two_gigabytes(engine):
    """[22][512][512][96], zeros except the last channel, whose centre tap feeds the one output channel: the output is that channel.
    Its bytes lie between 2.11e9 and 2.21e9 of the input, across 2^31."""
    shape = (512, 512, 96)
    x = np.zeros((22,) + shape, np.float32)
    x[21] = np.random.default_rng(6).random(shape, dtype=np.float32)
    assert 21 * x[21].nbytes < 2 ** 31 < x.nbytes
    w = np.zeros((1, 22, 3, 3, 3), np.float32)
    w[0, 21, 1, 1, 1] = 1.0
    got, rep = seg.segment_stage("conv", x, weight=w, bias=np.zeros(1, np.float32))
    assert np.array_equal(got[0], x[21])
    assert rep["ms_conv"] > 0


@pytest.mark.parametrize("shape", [(1, 2, 2, 2), (3, 6, 10, 4), (2, 7, 9, 5), (5, 16, 16, 32)], **_ids)
def test_maxpool3d_is_bit_equal(engine, shape):
    x = np.random.default_rng(1).normal(size=shape).astype(np.float32)
    got, _ = seg.segment_stage("maxpool", x)
    assert np.array_equal(got, F.max_pool3d(torch.as_tensor(x)[None], 2)[0].numpy())


def _norm_inputs():
    rng = np.random.default_rng(3)
    smallest = rng.normal(size=(3, 1, 1, 2)).astype(np.float32)        # two voxels: the bottleneck of the smallest legal patch
    offset = rng.normal(size=(4, 9, 11, 13)).astype(np.float32)
    offset[0] += 1e3                                                   # mean 1e3, spread 1: a float32 sum of squares loses it
    offset[1] *= 1e-3
    segments = rng.normal(2.0, 3.0, size=(2, 40, 32, 40)).astype(np.float32)  # 51200 voxels: four segments of statistics
    return {"1x1x2": smallest, "offset": offset, "segments": segments}


@pytest.mark.parametrize("name", ["1x1x2", "offset", "segments"])
def test_norm_lrelu_is_as_close_to_float64_as_the_float32_operator_of_torch(engine, name):
    """Error against float64 at most 2 x the largest error of torch's float32 CPU instance_norm + leaky_relu in the same channel,
    with a floor of 4 ulp of the output; the same input gives the same bytes."""
    x = _norm_inputs()[name]
    op = lambda t: F.leaky_relu(F.instance_norm(t[None], eps=1e-5), 0.01)[0].numpy()  # noqa: E731
    want = op(torch.as_tensor(x, dtype=torch.float64))
    yard = np.abs(op(torch.as_tensor(x)) - want).max(axis=(1, 2, 3), keepdims=True)
    got, _ = seg.segment_stage("norm_lrelu", x)
    err = np.abs(got - want)
    bound = np.maximum(2 * yard, 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    print(f"norm {name}: max error {err.max():.3g}, yardstick {yard.max():.3g}, max error / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    again, _ = seg.segment_stage("norm_lrelu", x)
    assert np.array_equal(got, again)


def test_both_networks_share_one_instance_norm(engine):
    """speedup_stage on [c, H, W] and segment_stage on the same data as [c, 1, H, W] return the same bytes; 130 x 130 is past the
    16384 elements of a segment, so the fold over segments runs."""
    rng = np.random.default_rng(5)
    for shape in [(3, 5, 7), (2, 130, 130)]:
        x = rng.normal(2.0, 3.0, size=shape).astype(np.float32)
        flat, _ = cases.pkg.speedup.speedup_stage("norm_lrelu", x)
        deep, _ = seg.segment_stage("norm_lrelu", x[:, None])
        assert flat.shape == shape and deep.shape == (shape[0], 1) + shape[1:] and np.ptp(flat) > 0
        assert flat.tobytes() == deep.tobytes()


def test_head_is_as_close_to_float64_as_the_float32_operators_of_torch(engine):
    """softmax over channels 0 .. 7 and sigmoid on channel 8: error at most 2 x torch's float32 CPU error per channel, floor 4 x 2^-24."""
    logits = (np.random.default_rng(5).normal(size=(9, 5, 7, 11)) * 3.0).astype(np.float32)
    op = lambda t: segment_ref.head(t[None])[0].numpy()  # noqa: E731
    want = op(torch.as_tensor(logits, dtype=torch.float64))
    yard = np.abs(op(torch.as_tensor(logits)) - want).max(axis=(1, 2, 3), keepdims=True)
    got, _ = seg.segment_stage("head", logits)
    err = np.abs(got - want)
    bound = np.maximum(2 * yard, 4 * 2.0 ** -24)
    print(f"head: max error {err.max():.3g}, yardstick {yard.max():.3g}, max error / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    np.testing.assert_allclose(got[:8].sum(axis=0), 1.0, rtol=0, atol=8 * 2.0 ** -24)


def test_stitch_and_finalize_are_bit_equal_to_the_numpy_stitcher(engine):
    """Overlapping patches, a repeated one and voxels no patch reaches, in float32 as the reference keeps them; then the labels, with
    a tie between two channels (the first wins) and a vessel mean of exactly 0.5 (not above 0.5)."""
    rng = np.random.default_rng(4)
    volume, patch = (6, 5, 41), (4, 4, 34)
    starts = [(0, 0, 0), (0, 0, 7), (2, 1, 3), (2, 1, 3), (1, 0, 2), (2, 1, 0), (0, 1, 0)]
    data = rng.random((len(starts), 9) + patch).astype(np.float32)
    data[3] = data[2]
    data[0, 8], data[6, 8] = 0.25, 0.75                    # voxel (0, 1, 0) sees exactly these two: mean 0.5
    data[0, 2, 0, 0, 0] = data[0, 5, 0, 0, 0] = 2.0        # voxel (0, 0, 0) sees patch 0 alone: channels 2 and 5 tie at the top
    want = segment_ref.Stitcher((9,) + volume)
    for d, s in zip(data, starts):
        want.add(d, s)
    mean = want.mean()
    assert (want.n == 0).any() and want.n.max() >= 4 and want.n[8, 0, 1, 0] == 2 and mean[8, 0, 1, 0] == 0.5
    got, _ = seg.segment_stage("stitch", data, starts=starts, shape=volume)
    assert got.dtype == np.float32 and got.tobytes() == mean.tobytes()
    labels, _ = seg.segment_stage("finalize", got)
    assert labels.dtype == np.uint8 and np.array_equal(labels, segment_ref.finalize(mean))
    assert labels[:8, 0, 0, 0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and labels[8, 0, 1, 0] == 0
    assert np.all(labels[:8].sum(axis=0) == 1)


# ------------------------------------------------------------------------------------------------------------ whole network
PATCH = (16, 16, 32)
NETWORKS = {"reference": (segment_ref.REFERENCE_FILTERS, 4), "unequal": ((8, 12, 16, 12, 8, 8), 2)}


@pytest.mark.parametrize("name", ["reference", "unequal"])
def test_network_equals_the_float64_restatement(engine, name):
    """One 16 x 16 x 32 patch (the image is the patch: the rule gives its start eight times, one is inferred), seeded_weights(7).
    Allowed error of the raw probabilities, per channel: 4 x the largest error of the float32 CPU run of the restatement against
    float64 (the margin the 2-D network got, which measured 0.8 - 2.8 of it).

    Measured on the MI355X, largest error / yardstick over the channels: see profiles/segment_ab.md."""
    filters, levels = NETWORKS[name]
    weights = segment_ref.seeded_weights(7, filters, levels)
    image = segment_ref.seeded_image(7, PATCH)
    x = segment_ref.rescale(image)
    with torch.no_grad():
        p64 = segment_ref.head(torch.as_tensor(segment_ref.logits_of(weights, x))[None])[0].numpy()
        p32 = segment_ref.head(torch.as_tensor(segment_ref.logits_of(weights, x, torch.float32))[None])[0].numpy()
    yard = np.abs(p32 - p64).max(axis=(1, 2, 3))
    model = seg.MCSegmenter(weights, patch_shape=PATCH)
    labels, raw = model.segment(image)
    assert raw.shape == (9,) + PATCH and labels.shape == raw.shape and labels.dtype == np.uint8
    ratio = np.abs(raw - p64).max(axis=(1, 2, 3)) / yard
    print(f"network {name}: error / yardstick per channel = {np.array2string(ratio, precision=3)}; yardstick {yard.max():.3g}")
    assert np.all(ratio <= 4.0)
    assert model.last_report["patches_run"] == 1 and model.last_report["patches_skipped"] == 7
    assert np.array_equal(labels, segment_ref.finalize(raw))


# ---------------------------------------------------------------------------------------------------------- whole procedure
PROCEDURE_SEED = 8   # seeded_weights(7) leaves label 3 without a voxel on these images; seed 8 gives every label at least 450
PROCEDURE_CASES = {
    "24x20x72-overlap0-int16": ((24, 20, 72), 0.0, np.int16, (12, 0)),
    "24x20x72-overlap0.5-int16": ((24, 20, 72), 0.5, np.int16, (16, 8)),
    "24x20x72-overlap0-float32": ((24, 20, 72), 0.0, np.float32, (12, 0)),
    "24x20x72-overlap0.5-float32": ((24, 20, 72), 0.5, np.float32, (16, 8)),
    "10x16x20-int16": ((10, 16, 20), 0.0, np.int16, (1, 7)),        # smaller than the patch: padded to 16 x 16 x 32
    "10x16x20-float32": ((10, 16, 20), 0.0, np.float32, (1, 7)),
}


def _procedure_image(shape, dtype):
    image = segment_ref.seeded_image(3, shape, dtype)
    if dtype is np.float32 and shape == (10, 16, 20):
        image = image + np.float32(0.375)                               # fractional HU, exact in float32
    return image


@pytest.fixture(scope="module")
def procedure_truth():
    """Per (shape, overlap, fractional): the float64 restatement and the error of its float32 CPU run, computed once."""
    weights, cache = segment_ref.seeded_weights(PROCEDURE_SEED), {}

    def get(shape, overlap, dtype):
        image = _procedure_image(shape, dtype)
        key = (shape, overlap, image.astype(np.float64).tobytes())
        if key not in cache:
            labels, raw = segment_ref.segment(weights, image, PATCH, overlap)
            raw32 = segment_ref.segment(weights, image, PATCH, overlap, dtype=torch.float32)[1]
            allow = 4.0 * np.abs(raw32 - raw).max(axis=(1, 2, 3))
            top = np.sort(raw[:8], axis=0)
            sure = np.stack([top[-1] - top[-2] > 2.0 * allow[:8].max()] * 8 + [np.abs(raw[8] - 0.5) > 2.0 * allow[8]])
            cache[key] = dict(labels=labels, raw=raw, allow=allow, sure=sure)
        return image, cache[key]
    return get


@pytest.fixture(scope="module")
def model8():
    return seg.MCSegmenter(segment_ref.seeded_weights(PROCEDURE_SEED), patch_shape=PATCH)


@pytest.mark.parametrize("case", list(PROCEDURE_CASES))
def test_procedure_equals_the_float64_restatement(engine, procedure_truth, case):
    """Raw within 4 x the float32 CPU error per channel; labels equal at every voxel whose float64 top-two margin (channel 8:
    |p - 0.5|) exceeds twice that allowance, at most 1 % of the voxels left out; all eight softmax labels occur; a second call gives
    the same bytes."""
    shape, overlap, dtype, (run, skipped) = PROCEDURE_CASES[case]
    image, t = procedure_truth(shape, overlap, dtype)
    model = seg.MCSegmenter(segment_ref.seeded_weights(PROCEDURE_SEED), patch_shape=PATCH, patch_overlap=overlap)
    labels, raw = model.segment(image)
    rep = dict(model.last_report)
    assert labels.shape == raw.shape == t["raw"].shape == (9,) + seg.padded_shape(shape, PATCH)
    ratio = np.abs(raw - t["raw"]).max(axis=(1, 2, 3)) / t["allow"]
    left_out = 1.0 - t["sure"].mean(axis=(1, 2, 3))
    print(f"procedure {case}: error / allowance per channel = {np.array2string(ratio, precision=3)}; left out {left_out[0]:.4f} (softmax), "
          f"{left_out[8]:.4f} (vessels); labels that differ anywhere: {int((labels != t['labels']).sum())}; report {rep}")
    assert np.all(ratio <= 1.0)
    assert left_out.max() <= 0.01
    assert np.array_equal(labels[t["sure"]], t["labels"][t["sure"]])
    assert np.all(t["labels"][:8].reshape(8, -1).sum(axis=1) > 0) and np.all(labels[:8].reshape(8, -1).sum(axis=1) > 0)
    assert np.all(labels[:8].sum(axis=0) == 1) and np.array_equal(labels, segment_ref.finalize(raw))
    assert (rep["patches_run"], rep["patches_skipped"]) == (run, skipped)
    assert rep["ms_conv"] > 0 and rep["ms_norm"] > 0 and rep["ms_total"] >= rep["ms_conv"] + rep["ms_norm"]
    assert 0 < rep["peak_device_bytes"] <= rep["planned_device_bytes"] * 1.01 + (1 << 20)
    again = model.segment(image)
    assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == raw.tobytes()


def test_int16_and_float32_images_of_the_same_values_give_the_same_bytes(engine, model8):
    image = segment_ref.seeded_image(3, (24, 20, 72))
    a, b = model8.segment(image), model8.segment(image.astype(np.float32))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = model8.segment(image.astype(np.float64))                        # anything else is read as float32
    assert c[1].tobytes() == a[1].tobytes()


# -------------------------------------------------------------------------------------------------------------- end to end
KW = dict(n_projections=2, angle_between_projections=70.0, n_histories=200_000, **cases.SMALL_DET)
TABLES = ("voxel_mat_dens", "density_max", "mfp_woodcock", "woodcock_coarse", "mfp_a", "mfp_b", "palette")
COUNTERS = ("palette_size", "volume_kind", "brick_shift", "brick_count", "bricks_mixed", "bricks_exterior", "sub_bricks_mixed", "tile_records",
            "tiles_in_mixed_bricks", "num_voxels_x", "num_voxels_y", "num_voxels_z", "num_materials_used")


def _base(tmp_path):
    g = geo.MCBoxGeometry(shape=(12, 10, 8), image_spacing=(20.0, 20.0, 20.0), material="h2o")
    return cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), **KW).prepare_simulation(tmp_path / "base")


def _segmentations(labels):
    out = {"body": (labels[seg.get_label_index("background")] == 0).astype(np.uint8)}
    for name, label in geo.PREDICTED_LABELS.items():
        out[name] = labels[seg.get_label_index(label)]
    return out


def test_ct_file_to_context_geometry_through_the_segmenter(engine, tmp_path, procedure_truth):
    """`Context.set_geometry_from_image(ct.mha, segmenter=...)` and `MCGeometry.from_image(..., segmenter=..., engine_context=...)`:
    the materials and densities of `map_image` on the restatement's labels, at every voxel whose 3 x 3 x 3 neighbourhood holds no
    voxel the margin rule leaves out (the bone outline looks one voxel around); and the installed context is the one `set_geometry`
    builds from those arrays."""
    from scipy import ndimage
    shape, overlap = (24, 20, 72), 0.5
    image, t = procedure_truth(shape, overlap, np.int16)
    spacing = (6.0, 7.0, 8.0)
    recon.write_mha(tmp_path / "ct.mha", image.swapaxes(0, 2), spacing, (0.0, 0.0, 0.0), element_type="MET_SHORT")
    model = seg.MCSegmenter(segment_ref.seeded_weights(PROCEDURE_SEED), patch_shape=PATCH, patch_overlap=overlap)
    with engine.create(_base(tmp_path), device=0) as dev, engine.create(_base(tmp_path), device=0) as host:
        got = geo.MCGeometry.from_image(tmp_path / "ct.mha", segmenter=model, engine_context=dev)
        want_m, want_d = dev.map_image(image, _segmentations(t["labels"]))
        doubtful = ndimage.binary_dilation(~t["sure"].all(axis=0), structure=np.ones((3, 3, 3), bool))
        print(f"end to end: {int((got.materials != want_m).sum())} voxels differ, {doubtful.mean():.4f} of the volume is doubtful")
        assert doubtful.mean() < 0.1 and got.image_spacing == spacing and got.image_shape == shape
        assert np.array_equal(got.materials[~doubtful], want_m[~doubtful]) and np.array_equal(got.densities[~doubtful], want_d[~doubtful])
        assert len(np.unique(got.materials)) >= 8
        host_route = geo.MCGeometry.from_image(tmp_path / "ct.mha", segmenter=model)      # the numpy pipeline on the device's labels
        assert np.array_equal(host_route.materials, got.materials) and np.array_equal(host_route.densities, got.densities)
        dev.set_geometry_from_image(tmp_path / "ct.mha", segmenter=model)
        host.set_geometry(got)
        for key in COUNTERS:
            assert dev.geti(key) == host.geti(key), key
        for name in TABLES:
            assert np.array_equal(dev.host_table(name), host.host_table(name)), name
