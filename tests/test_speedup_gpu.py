"""The speed-up network on the MI355X (csrc/speedup_net.hip through mcgpu_speedup_stage / mcgpu_speedup_run): every operator
against float64, the whole network against the float64 restatement (speedup_ref.py, chained to the reference class by
golden/speedup_pin.npz), the sampler against its numpy restatement, and the file-level step of the scan driver."""
import numpy as np
import pytest

import cases
import speedup_ref

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

speedup = cases.pkg.speedup
recon = cases.pkg.reconstruction
pytestmark = pytest.mark.gpu

CONV_PAIRS = [((2, 0), 64), ((64, 0), 64), ((64, 0), 1), ((1, 0), 16), ((48, 0), 32), ((64, 128), 64)]  # ((c1, c2 upsampled), c_out)
CONV_SHAPES = [(1, 1), (5, 7), (33, 70), (32, 48)]  # rows x columns: one pixel, below a tile, several tiles with ragged edges, whole tiles


def _upsampled(a, H, W):
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)[:, :H, :W]


def _conv64(x, w, b):
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    return F.conv2d(F.pad(t(x)[None], (1, 1, 1, 1), mode="replicate"), t(w), t(b))[0].numpy()


def _conv_case(rng, c1, c2, c_out, H, W, integers):
    draw = (lambda lo, hi, size: rng.integers(lo, hi + 1, size=size).astype(np.float32)) if integers else \
        (lambda lo, hi, size: rng.uniform(lo, hi, size=size).astype(np.float32))
    x1 = draw(-3, 3, (c1, H, W))
    x2 = draw(-3, 3, (c2, (H + 1) // 2, (W + 1) // 2)) if c2 else None
    w = draw(-8, 8, (c_out, c1 + c2, 3, 3)) if integers else draw(-1, 1, (c_out, c1 + c2, 3, 3))
    b = draw(-9, 9, (c_out,))
    x = x1 if x2 is None else np.concatenate([x1, _upsampled(x2, H, W)])
    return x1, x2, w, b, x


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", CONV_PAIRS, ids=lambda p: f"{p[0][0]}+{p[0][1]}to{p[1]}")
def test_conv_of_small_integers_is_bit_equal_to_float64(engine, pair, shape):
    """Random integer inputs (|x| <= 3), weights (|w| <= 8, unrelated across c_out, c_in and tap) and biases: every product and
    partial sum is an integer below 9 x 192 x 24 + 9 < 2^24, exact in float32 in any order, so the output equals the float64 result
    bit for bit; a slip in the lane map, the transposition, the tap order or the order of the sources gives a wrong integer."""
    (c1, c2), c_out = pair
    H, W = shape
    x1, x2, w, b, x = _conv_case(np.random.default_rng(c1 * 1000 + c_out + H), c1, c2, c_out, H, W, integers=True)
    got, _ = speedup.speedup_stage("conv", x1, in2=x2, weight=w, bias=b, upsample=bool(c2))
    want = _conv64(x, w, b)
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pair", CONV_PAIRS, ids=lambda p: f"{p[0][0]}+{p[0][1]}to{p[1]}")
def test_conv_of_float_data_is_within_the_bound_of_a_float32_fma_chain(engine, pair, shape):
    """|got - float64| <= (9 C_in + 1) 2^-24 (sum |a b| + |bias|) per output: the bound of a float32 fma chain of 9 C_in products
    and the bias in any order."""
    (c1, c2), c_out = pair
    H, W = shape
    x1, x2, w, b, x = _conv_case(np.random.default_rng(c1 * 1000 + c_out + W), c1, c2, c_out, H, W, integers=False)
    got, _ = speedup.speedup_stage("conv", x1, in2=x2, weight=w, bias=b, upsample=bool(c2))
    want = _conv64(x, w, b)
    bound = (9 * (c1 + c2) + 1) * 2.0 ** -24 * _conv64(np.abs(x), np.abs(w), np.abs(b))
    excess = np.abs(got - want) / bound
    print(f"conv {pair} {shape}: max error / bound = {excess.max():.3g}")
    assert excess.max() <= 1.0


def test_conv_at_full_size_indexes_every_tile(engine):
    """1024 x 768, C_in 8, C_out 64, integer data: bit-equal (float32 sums of small integers are exact on the CPU too)."""
    rng = np.random.default_rng(5)
    H, W = 768, 1024
    x1, _, w, b, _ = _conv_case(rng, 8, 0, 64, H, W, integers=True)
    got, rep = speedup.speedup_stage("conv", x1, weight=w, bias=b)
    want = F.conv2d(F.pad(torch.as_tensor(x1)[None], (1, 1, 1, 1), mode="replicate"), torch.as_tensor(w), torch.as_tensor(b))[0].numpy()
    assert np.array_equal(got, want)
    assert rep["ms_conv"] > 0


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 6, 10), (2, 7, 9), (5, 64, 96)])
def test_maxpool_is_bit_equal(engine, shape):
    x = np.random.default_rng(1).normal(size=shape).astype(np.float32)
    got, _ = speedup.speedup_stage("maxpool", x)
    assert np.array_equal(got, F.max_pool2d(torch.as_tensor(x)[None], 2)[0].numpy())


@pytest.mark.parametrize("shape", [(6, 10), (5, 7), (32, 48)])
def test_second_source_read_through_the_upsample_is_bit_equal(engine, shape):
    """Identity weights (centre tap of channel k -> output k), no bias: the output is cat(in, upsample(in2)) itself."""
    H, W = shape
    rng = np.random.default_rng(2)
    x1 = rng.normal(size=(2, H, W)).astype(np.float32)
    x2 = rng.normal(size=(5, (H + 1) // 2, (W + 1) // 2)).astype(np.float32)
    w = np.zeros((7, 7, 3, 3), np.float32)
    w[np.arange(7), np.arange(7), 1, 1] = 1.0
    got, _ = speedup.speedup_stage("conv", x1, in2=x2, weight=w, bias=np.zeros(7, np.float32), upsample=True)
    assert np.array_equal(got, np.concatenate([x1, _upsampled(x2, H, W)]))


def _norm_inputs():
    rng = np.random.default_rng(3)
    smallest = rng.normal(size=(3, 2, 2)).astype(np.float32)           # H W = 4: the bottleneck of the smallest legal image
    offset = rng.normal(size=(4, 33, 70)).astype(np.float32)
    offset[0] += 1e3                                                   # mean 1e3, spread 1: a float32 sum of squares loses it
    offset[1] *= 1e-3
    segments = rng.normal(2.0, 3.0, size=(2, 256, 160)).astype(np.float32)  # 40960 pixels: three segments of statistics
    return {"2x2": smallest, "offset": offset, "segments": segments}


@pytest.mark.parametrize("name", ["2x2", "offset", "segments"])
def test_norm_lrelu_is_as_close_to_float64_as_the_float32_operator_of_torch(engine, name):
    """Error against float64 at most 2 x the largest error of torch's float32 CPU instance_norm + leaky_relu in the same channel,
    with a floor of 4 ulp of the output."""
    x = _norm_inputs()[name]
    op = lambda t: F.leaky_relu(F.instance_norm(t[None], eps=1e-5), 0.01)[0].numpy()  # noqa: E731
    want = op(torch.as_tensor(x, dtype=torch.float64))
    yard = np.abs(op(torch.as_tensor(x)) - want).max(axis=(1, 2), keepdims=True)
    got, _ = speedup.speedup_stage("norm_lrelu", x)
    err = np.abs(got - want)
    bound = np.maximum(2 * yard, 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    print(f"norm {name}: max error {err.max():.3g}, yardstick {yard.max():.3g}, max error / bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    again, _ = speedup.speedup_stage("norm_lrelu", x)
    assert np.array_equal(got, again)


def test_preprocess_stage_equals_its_statement(engine):
    low_photon, forward_projection = speedup_ref.seeded_inputs(5, 3, 48, 80)
    forward_projection = forward_projection * 37.0 + 5.0
    got, _ = speedup.speedup_stage("preprocess", low_photon, in2=forward_projection)
    t = lambda a: torch.as_tensor(a[:, None], dtype=torch.float64)  # noqa: E731
    want = speedup_ref.preprocess(t(low_photon), t(forward_projection))[:, 0].numpy()
    # four float32 operations and four statistics rounded to float32, each half an ulp, on values below 8
    assert np.abs(got - want).max() <= 8 * 2.0 ** -24 * 8
    assert np.abs(got - speedup.MCSpeedup.preprocess_inputs(low_photon, forward_projection)[1]).max() <= 8 * 2.0 ** -24 * 8


# ------------------------------------------------------------------------------------------------------------ whole network
NETWORK_SHAPES = [(1, 32, 32), (2, 32, 48), (1, 48, 80)]


@pytest.fixture(scope="module")
def model7():
    return speedup.MCSpeedup(speedup_ref.seeded_weights(7))


@pytest.fixture(scope="module")
def truth7():
    """Per shape: inputs, the float64 restatement and the error of its float32 CPU run (the yardstick), computed once."""
    weights = speedup_ref.seeded_weights(7)
    out = {}
    for shape in NETWORK_SHAPES:
        lp, fp = speedup_ref.seeded_inputs(7, *shape)
        m64, v64 = speedup_ref.predict(weights, lp, fp)
        m32, v32 = speedup_ref.predict(weights, lp, fp, dtype=torch.float32)
        out[shape] = dict(lp=lp, fp=fp, mean=m64, variance=v64, yard=(np.abs(m32 - m64).max(), np.abs(v32 - v64).max()))
    return out


@pytest.mark.parametrize("shape", NETWORK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_network_equals_the_float64_restatement(engine, model7, truth7, shape):
    """Tolerance: 4 x the largest error of the float32 CPU run of the restatement against float64, per shape and output (the order
    of summation differs and a 2 x 2 instance norm amplifies last-bit differences).  The forward projection scaled and shifted
    (x 37 + 5) must give the same within that tolerance: the preprocessing undoes it.

    Measured on the MI355X, error / yardstick (mean, variance) -- yardstick (mean, variance):
      1x32x32  0.78, 0.99 (scaled and shifted forward projection 0.83, 0.91) -- 1.18e-4, 8.3e-6
      2x32x48  2.40, 2.07 (2.54, 1.88) -- 4.8e-5, 4.4e-6
      1x48x80  1.86, 2.60 (2.07, 2.83) -- 2.9e-5, 2.6e-6"""
    t = truth7[shape]
    assert np.mean(t["mean"] == 0) < 0.01  # the head does not saturate
    mean, variance = model7.predict(t["lp"], t["fp"])
    ratios = (np.abs(mean - t["mean"]).max() / t["yard"][0], np.abs(variance - t["variance"]).max() / t["yard"][1])
    mean_s, variance_s = model7.predict(t["lp"], t["fp"] * np.float32(37.0) + np.float32(5.0))
    ratios_s = (np.abs(mean_s - t["mean"]).max() / t["yard"][0], np.abs(variance_s - t["variance"]).max() / t["yard"][1])
    print(f"network {shape}: error / yardstick = {ratios[0]:.3g}, {ratios[1]:.3g}; scaled and shifted fp {ratios_s[0]:.3g}, {ratios_s[1]:.3g}; "
          f"yardstick {t['yard'][0]:.3g}, {t['yard'][1]:.3g}")
    assert max(ratios) <= 4.0
    assert max(ratios_s) <= 4.0
    assert np.all(mean >= 0) and np.all(variance >= 1e-6)


def test_network_is_independent_of_grouping_and_repeats_bit_for_bit(engine, model7, truth7):
    t = truth7[(2, 32, 48)]
    assert not np.array_equal(t["lp"][0], t["lp"][1])
    both = model7.predict(t["lp"], t["fp"])
    again = model7.predict(t["lp"], t["fp"])
    first = model7.predict(t["lp"][:1], t["fp"][:1])
    second = model7.predict(t["lp"][1:], t["fp"][1:])
    for k in range(2):
        assert both[k].tobytes() == again[k].tobytes()
        assert both[k].tobytes() == np.concatenate([first[k], second[k]]).tobytes()


def test_network_trained_without_the_forward_projection(engine):
    tensors = [(n, (64, 1, 3, 3) if n == "mean_net.init_conv.weight" else s) for n, s in speedup_ref.golden_tensors()]
    weights = speedup_ref.seeded_weights(9, tensors)
    lp, _ = speedup_ref.seeded_inputs(9, 1, 32, 48)
    m64, v64 = speedup_ref.predict(weights, lp, None)
    m32, v32 = speedup_ref.predict(weights, lp, None, dtype=torch.float32)
    mean, variance = speedup.MCSpeedup(weights).predict(lp)
    assert np.mean(m64 == 0) < 0.01
    assert np.abs(mean - m64).max() <= 4 * np.abs(m32 - m64).max()
    assert np.abs(variance - v64).max() <= 4 * np.abs(v32 - v64).max()


# ------------------------------------------------------------------------------------------------------------------ sampler
def test_normals_equal_the_numpy_restatement(engine):
    seed = 0xFEDC_BA98_7654_3210
    z, _ = speedup.speedup_stage("normals", shape=(3, 48, 80), seed=seed, first_projection=5)
    want = speedup_ref.normals(seed, 3, 48, 80, first_projection=5)
    assert np.abs(z - want).max() <= 4e-6  # float32 log and cos of the device against float64
    z0, _ = speedup.speedup_stage("normals", shape=(1, 48, 80), seed=seed, first_projection=5)
    z1, _ = speedup.speedup_stage("normals", shape=(2, 48, 80), seed=seed, first_projection=6)
    assert z.tobytes() == np.concatenate([z0, z1]).tobytes()
    other, _ = speedup.speedup_stage("normals", shape=(3, 48, 80), seed=seed + 1, first_projection=5)
    assert not np.array_equal(z, other) and abs(np.corrcoef(z.ravel(), other.ravel())[0, 1]) < 0.05


def test_sample_is_mean_plus_sigma_z(engine, model7, truth7):
    t = truth7[(2, 32, 48)]
    seed = 1234567
    mean, variance, sample = model7.execute(t["lp"], t["fp"], seed=seed)
    assert model7.last_report["seed"] == seed
    m2, v2 = model7.predict(t["lp"], t["fp"])
    assert mean.tobytes() == m2.tobytes() and variance.tobytes() == v2.tobytes()
    z, _ = speedup.speedup_stage("normals", shape=mean.shape, seed=seed)
    term = np.sqrt(variance) * z
    assert np.all(np.abs(sample - (mean + term)) <= 2 * np.spacing(np.maximum(np.abs(mean), np.abs(term))))  # 2 ulp of the larger term
    assert np.abs(sample - model7.sample(mean, variance, seed)).max() <= 2 * np.spacing(np.float32(8))
    again = model7.execute(t["lp"], t["fp"], seed=seed, batch_size=1)[2]
    assert sample.tobytes() == again.tobytes()
    assert not np.array_equal(sample, model7.execute(t["lp"], t["fp"], seed=seed + 1)[2])
    tail = model7.execute(t["lp"][1:], t["fp"][1:], seed=seed, first_projection=1)[2]
    assert sample[1:].tobytes() == tail.tobytes()
    model7.execute(t["lp"], t["fp"])  # seed=None: drawn, and reported
    assert isinstance(model7.last_report["seed"], int)


# ---------------------------------------------------------------------------------------------------------------- full size
def test_one_projection_at_full_size(engine, model7):
    """One 1024 x 768 projection: finite, mean >= 0, variance >= 1e-6, repeatable, report filled in.
    Measured on the MI355X: peak_device_bytes 1,605,255,112 (1531 MiB); ms_conv 10.1, ms_norm 1.7, ms_preprocess 0.04, ms_other 0.11,
    ms_upload 1.8 (the weights), ms_total 15.3."""
    lp, fp = speedup_ref.seeded_inputs(4, 1, 768, 1024)
    mean, variance, sample = model7.execute(lp, fp, seed=1)
    rep = dict(model7.last_report)
    print("full size report:", rep)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(variance)) and np.all(np.isfinite(sample))
    assert mean.min() >= 0 and variance.min() >= 1e-6
    assert np.mean(mean == 0) < 0.01
    for key in ("ms_upload", "ms_preprocess", "ms_conv", "ms_norm", "ms_other", "ms_total", "peak_device_bytes"):
        assert rep[key] > 0, key
    assert rep["ms_total"] >= rep["ms_conv"] + rep["ms_norm"]
    again = model7.execute(lp, fp, seed=1)
    for a, b in zip((mean, variance, sample), again):
        assert a.tobytes() == b.tobytes()


# -------------------------------------------------------------------------------------------------- the scan driver's step
@pytest.mark.parametrize("is_4d", [False, True])
def test_speedup_simulation_writes_the_speedup_stack(engine, tmp_path, model7, is_4d):
    weights = speedup_ref.seeded_weights(7)
    np.savez(tmp_path / "weights.npz", **weights)
    lp, fp = speedup_ref.seeded_inputs(8, 2, 32, 48)
    config = tmp_path / "speedup_20.00x"
    config.mkdir()
    spacing, origin = [0.776, 0.776, 1.0], [-18.0, -12.0, 0.0]
    recon.write_mha(config / "projections_total_normalized.mha", lp, spacing, origin)
    recon.write_mha(config / "density_fp_4d.mha" if is_4d else tmp_path / "density_fp.mha", fp, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    out, report = speedup.speedup_simulation(tmp_path, "speedup_20.00x", tmp_path / "weights.npz", is_4d=is_4d, seed=77)
    assert out == config / "projections_total_normalized_speedup.mha" and report["seed"] == 77
    data, got_spacing, got_origin = recon.read_mha(out)
    assert got_spacing == spacing and got_origin == origin and data.shape == lp.shape and data.dtype == np.float32
    assert data.tobytes() == model7.execute(lp, fp, seed=77)[2].tobytes()
