"""The speed-up network without a GPU (4d-cbct-mc_amd/speedup.py, csrc/speedup_net.hip): the float64 restatement
(speedup_ref.py) against the reference class (recorded in golden/speedup_pin.npz by gen_speedup_golden.py, and directly where a
reference tree is present), the loader of weights, the statement of the preprocessing, every refusal of the C ABI and the
restatement of the sampler."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import speedup_ref

torch = pytest.importorskip("torch")
speedup = cases.pkg.speedup
REFERENCE = Path(os.environ.get("CBCTMC_REFERENCE", "/root/reference"))  # where oracle/Makefile looks for it too


def _golden_names():
    return [(n, s) for n, s in speedup_ref.golden_tensors() if n != "var_scale"]


@pytest.fixture(scope="module")
def weights7():
    return speedup_ref.seeded_weights(7)


def test_state_dict_order_of_the_package_is_the_reference_class_order():
    assert speedup.state_dict_tensors() == _golden_names()
    assert sum(int(np.prod(s)) for _, s in _golden_names()) == 13_401_586
    assert len(speedup_ref.golden_tensors()) == 57


def test_restatement_reproduces_the_reference_class_pin(weights7):
    pin = np.load(speedup_ref.GOLDEN / "speedup_pin.npz")
    low_photon, forward_projection = speedup_ref.seeded_inputs(7, 2, 32, 48)
    mean, variance = speedup_ref.predict(weights7, low_photon, forward_projection)
    assert np.mean(pin["mean"] == 0) < 0.01  # the head does not saturate: a wrong network cannot hide behind the relu
    np.testing.assert_allclose(mean, pin["mean"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(variance, pin["variance"], rtol=1e-9, atol=0)


@pytest.mark.skipif(not (REFERENCE / "cbctmc" / "speedup" / "models.py").exists(), reason="no reference tree")
@pytest.mark.parametrize("in_channels", [2, 1])
def test_restatement_equals_the_reference_class_directly(in_channels):
    import gen_speedup_golden
    tensors = speedup_ref.golden_tensors()
    if in_channels == 1:
        tensors = [(n, (s[0], 1, 3, 3) if n == "mean_net.init_conv.weight" else s) for n, s in tensors]
    weights = speedup_ref.seeded_weights(11, tensors)
    low_photon, forward_projection = speedup_ref.seeded_inputs(11, 1, 48, 32)
    if in_channels == 1:
        forward_projection = None
    want = gen_speedup_golden.reference_predict(REFERENCE, weights, low_photon, forward_projection, in_channels)
    got = speedup_ref.predict(weights, low_photon, forward_projection)
    assert np.mean(want[0] == 0) < 0.01
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------------------------ loader
def test_loader_accepts_pth_and_npz_and_reads_the_architecture(tmp_path, weights7):
    torch.save({"model": {k: torch.as_tensor(v) for k, v in weights7.items()}}, tmp_path / "w.pth")
    np.savez(tmp_path / "w.npz", **weights7)
    a = speedup.MCSpeedup.from_filepath(tmp_path / "w.pth")
    b = speedup.MCSpeedup.from_filepath(tmp_path / "w.npz")
    assert a.mean_net == b.mean_net == (2, 4, 64) and a.var_net == b.var_net == (1, 2, 16)
    assert a.flat.dtype == np.float32 and a.flat.size == 13_401_586 and np.array_equal(a.flat, b.flat)
    want = np.concatenate([weights7[n].ravel() for n, _ in _golden_names()])
    assert np.array_equal(a.flat, want)
    without = {k: v for k, v in weights7.items() if k != "var_scale"}
    assert np.array_equal(speedup.MCSpeedup(without).flat, want)  # var_scale is optional


def test_loader_refuses_each_kind_of_bad_key_by_name(weights7):
    missing = {k: v for k, v in weights7.items() if k != "mean_net.dec_2.convs.3.bias"}
    with pytest.raises(ValueError, match=r"missing key mean_net\.dec_2\.convs\.3\.bias"):
        speedup.MCSpeedup(missing)
    missing = {k: v for k, v in weights7.items() if k != "mean_net.enc_1.convs.0.weight"}
    with pytest.raises(ValueError, match=r"missing key mean_net\.enc_1\.convs\.0\.weight"):
        speedup.MCSpeedup(missing)
    with pytest.raises(ValueError, match=r"unexpected key mean_net\.extra\.weight"):
        speedup.MCSpeedup({**weights7, "mean_net.extra.weight": np.zeros(3, np.float32)})
    with pytest.raises(ValueError, match=r"var_net\.enc_0\.convs\.3\.weight has shape \(16, 16, 3, 2\)"):
        speedup.MCSpeedup({**weights7, "var_net.enc_0.convs.3.weight": np.zeros((16, 16, 3, 2), np.float32)})
    with pytest.raises(ValueError, match=r"missing key var_net\.init_conv\.weight"):
        speedup.MCSpeedup({k: v for k, v in weights7.items() if k != "var_net.init_conv.weight"})


def test_loader_accepts_weights_trained_without_the_forward_projection():
    tensors = [(n, (64, 1, 3, 3) if n == "mean_net.init_conv.weight" else s) for n, s in speedup_ref.golden_tensors()]
    model = speedup.MCSpeedup(speedup_ref.seeded_weights(3, tensors))
    assert model.in_channels == 1 and model.flat.size == 13_401_586 - 64 * 9
    with pytest.raises(ValueError, match="forward_projection=None"):
        model.predict(np.ones((1, 32, 32), np.float32), np.ones((1, 32, 32), np.float32))


def test_preprocess_inputs_matches_the_torch_statement_with_the_unbiased_std():
    low_photon, forward_projection = speedup_ref.seeded_inputs(5, 3, 16, 24)
    forward_projection = forward_projection * 37.0 + 5.0
    lp, got = speedup.MCSpeedup.preprocess_inputs(low_photon, forward_projection)
    assert lp is not None and np.array_equal(lp, low_photon) and got.dtype == np.float32
    t = lambda a: torch.as_tensor(a[:, None], dtype=torch.float64)  # noqa: E731
    want = speedup_ref.preprocess(t(low_photon), t(forward_projection))[:, 0].numpy()
    # four float32 operations and four statistics rounded to float32, each half an ulp, on values below 8
    np.testing.assert_allclose(got, want, rtol=0, atol=8 * 2.0 ** -24 * 8)
    for p in range(3):  # the matched slice has the low-photon slice's mean and unbiased std
        assert abs(got[p].astype(np.float64).mean() - low_photon[p].astype(np.float64).mean()) < 1e-5
        assert abs(got[p].astype(np.float64).std(ddof=1) - low_photon[p].astype(np.float64).std(ddof=1)) < 1e-5
    assert speedup.MCSpeedup.preprocess_inputs(low_photon, None)[1] is None
    with pytest.raises(ValueError, match="zero variance"):
        speedup.MCSpeedup.preprocess_inputs(low_photon, np.ones_like(low_photon))


# ----------------------------------------------------------------------------------------------------- refusals of the C ABI
REFERENCE_N_WEIGHTS = 13_401_586


def _options(n=1, nu=32, nv=32, n_weights=REFERENCE_N_WEIGHTS, weights=None, mean=(2, 4, 64), var=(1, 2, 16)):
    return speedup._SpeedupOptions(C.sizeof(speedup._SpeedupOptions), 0, n, nu, nv, *mean, *var, weights, n_weights, 0, 0)


def _refused(engine, o, low_photon, forward_projection, text):
    lib = speedup._library()
    out = np.zeros((o.n, o.nv, o.nu), np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    assert lib.mcgpu_speedup_run(C.byref(o) if o is not None else None, ptr(low_photon), ptr(forward_projection), out.ctypes.data, None, None, None) == -1
    message = lib.mcgpu_last_error().decode()
    assert text in message, message


def test_abi_refusals_before_any_device_call(engine):
    flat = np.zeros(REFERENCE_N_WEIGHTS, np.float32)
    lp, fp = speedup_ref.seeded_inputs(1, 1, 32, 32)
    w = flat.ctypes.data
    lib = speedup._library()
    assert lib.mcgpu_speedup_run(None, lp.ctypes.data, fp.ctypes.data, None, None, None, None) == -1
    assert "struct_size" in lib.mcgpu_last_error().decode()
    _refused(engine, _options(weights=w), None, fp, "low_photon is NULL")
    _refused(engine, _options(weights=w), lp, None, "forward_projection is NULL")
    _refused(engine, _options(weights=None), lp, fp, "weights is NULL")
    _refused(engine, _options(weights=w, n_weights=REFERENCE_N_WEIGHTS - 1), lp, fp, "n_weights is 13401585 but the architecture has 13401586")
    _refused(engine, _options(weights=w, n_weights=REFERENCE_N_WEIGHTS, mean=(1, 4, 64)), lp, None, "the architecture has 13401010")
    _refused(engine, _options(weights=w, n_weights=REFERENCE_N_WEIGHTS - 64 * 9, mean=(1, 4, 64)), lp, fp, "forward_projection must be NULL")
    lp2, fp2 = speedup_ref.seeded_inputs(1, 1, 32, 40)
    _refused(engine, _options(weights=w, nu=40, nv=32), lp2, fp2, "must be divisible by 16")
    _refused(engine, _options(weights=w, nu=32, nv=40), lp2.reshape(1, 40, 32), fp2.reshape(1, 40, 32), "must be divisible by 16")
    lp3, fp3 = speedup_ref.seeded_inputs(1, 1, 16, 16)
    _refused(engine, _options(weights=w, nu=16, nv=16), lp3, fp3, "fewer than 2 pixels")
    _refused(engine, _options(weights=w, n=0), lp, fp, "n, nu and nv must be >= 1")
    _refused(engine, _options(weights=w, mean=(2, 0, 64)), lp, fp, "bad architecture")
    lp4, fp4 = speedup_ref.seeded_inputs(1, 2, 32, 32)
    fp4[1] = 2.5
    _refused(engine, _options(weights=w, n=2), lp4, fp4, "forward_projection slice 1 has zero variance")


@pytest.mark.parametrize("mean, var", [((1, 1, 4), (1, 1, 4)), ((2, 3, 8), (1, 2, 4)), ((2, 4, 64), (1, 2, 16))])
def test_library_counts_the_weights_as_the_package_does(engine, mean, var):
    """n_weights is checked before divisibility: with the package's total the library goes on to refuse an image side of
    2^levels + 1, with one value less it refuses the count and names the total."""
    n = sum(int(np.prod(s)) for _, s in speedup.state_dict_tensors(mean, var))
    deep = max(mean[1], var[1])
    side = 2 ** deep + 1
    flat = np.zeros(n, np.float32)
    lp, fp = speedup_ref.seeded_inputs(1, 1, side, side)
    fp = fp if mean[0] == 2 else None
    lib = speedup._library()
    _refused(engine, _options(weights=flat.ctypes.data, nu=side, nv=side, n_weights=n, mean=mean, var=var), lp, fp, f"must be divisible by {2 ** deep} ")
    assert "n_weights" not in lib.mcgpu_last_error().decode()
    _refused(engine, _options(weights=flat.ctypes.data, nu=side, nv=side, n_weights=n - 1, mean=mean, var=var), lp, fp,
             f"n_weights is {n - 1} but the architecture has {n} values")


def test_stage_refusals_before_any_device_call(engine):
    lib = speedup._library()
    buf = np.zeros(64, np.float32)
    o = speedup._SpeedupOptions(struct_size=C.sizeof(speedup._SpeedupOptions), n=1, nu=4, nv=4)

    def args(**kw):
        return speedup._SpeedupStageArgs(struct_size=C.sizeof(speedup._SpeedupStageArgs), **kw)

    for stage, a, text in [(9, args(in_=buf.ctypes.data, out=buf.ctypes.data, c1=1), "unknown stage 9"),
                           (0, args(in_=buf.ctypes.data, c1=1), "out is NULL"),
                           (1, args(out=buf.ctypes.data, c1=1), "in is NULL"),
                           (0, args(in_=buf.ctypes.data, out=buf.ctypes.data, c1=1, c_out=1), "weight or bias is NULL"),
                           (0, args(in_=buf.ctypes.data, out=buf.ctypes.data, c1=1, c2=1, c_out=1, weight=buf.ctypes.data, bias=buf.ctypes.data), "in2 is NULL"),
                           (2, args(in_=buf.ctypes.data, out=buf.ctypes.data, c1=0), "c1 must be"),
                           (3, args(in_=buf.ctypes.data, out=buf.ctypes.data), "in2 is NULL")]:
        assert lib.mcgpu_speedup_stage(C.byref(o), stage, C.byref(a), None) == -1
        assert text in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_speedup_stage(C.byref(o), 0, None, None) == -1
    assert "mcgpu_speedup_stage_args" in lib.mcgpu_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ sampler
def test_sampler_restatement_draws_standard_normals_from_philox10():
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
    import fast_rng
    seed = 0x1234_5678_9ABC_DEF0
    z = speedup_ref.normals(seed, 4, 512, 512, first_projection=3)  # 2^20 draws
    n = z.size
    assert n == 2 ** 20 and np.all(np.isfinite(z))  # u1 in (0, 1]: the logarithm is finite
    # one pixel by hand: counter (x, y, projection, 0), key (seed low, seed high), words 0 and 1
    w = fast_rng.philox4x32([5, 7, 3 + 2, 0], [seed & 0xFFFFFFFF, seed >> 32], rounds=10)
    u1, u2 = ((int(w[0]) >> 8) + 1) * 2.0 ** -24, (int(w[1]) >> 8) * 2.0 ** -24
    assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
    assert z[2, 7, 5] == np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    # the known-answer vector of Philox4x32-10 (Random123 kat_vectors: zero counter and key)
    kat = fast_rng.philox4x32([0, 0, 0, 0], [0, 0], rounds=10)
    assert [int(v) for v in kat] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert abs(z.mean()) < 4.0 / np.sqrt(n)                      # standard error of the mean: 1 / sqrt(n)
    assert abs(z.var() - 1.0) < 4.0 * np.sqrt(2.0 / n)           # standard error of the variance of normals: sqrt(2 / n)
    assert not np.array_equal(z[0], z[1])
    assert np.array_equal(z[1:], speedup_ref.normals(seed, 3, 512, 512, first_projection=4))
