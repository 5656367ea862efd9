"""`cbctmc_amd.correspondence.CorrespondenceModel` on the host (no GPU): the reference's correspondence model
(cbctmc/registration/correspondence.py:29-226) -- fit, predict, save, load -- restated with a defined order of operations."""
import hashlib
import pickle

import numpy as np
import pytest

import cases

correspondence = cases.pkg.correspondence
CorrespondenceModel = correspondence.CorrespondenceModel

# the pickle's keys, as data (the reference's save(), correspondence.py:65-77)
REFERENCE_KEYS = ["coefficients", "timesteps", "mean_signal", "signal_n_dims", "mean_vector_field", "spatial_shape", "signals", "reference_phase"]
EPS32 = 2.0 ** -24  # half an ulp of 1 in float32: the relative error of one rounding


def _breathing(T=10):
    """A ten-phase breathing signal and its derivative: well conditioned (the two are 90 degrees apart)."""
    t = np.arange(T)
    s = 0.5 + 0.5 * np.cos(2 * np.pi * t / T)
    ds = -np.pi / T * np.sin(2 * np.pi * t / T)
    return s, ds


def _fields(shape, seed=3, T=10):
    rng = np.random.default_rng(seed)
    s, ds = _breathing(T)
    A, B, C = (rng.normal(scale=sc, size=(3,) + shape).astype(np.float32) for sc in (4.0, 6.0, 1.5))
    fields = np.stack([A.astype(np.float64) * s[t] + B.astype(np.float64) * ds[t] + C for t in range(T)]).astype(np.float32)
    return fields, np.stack([s, ds], axis=1), (A, B, C)


def test_fit_recovers_a_linear_motion_model():
    """Fields generated as A s + B ds + C: fit returns A and B, predict returns the fields, to the float32 rounding of the inputs
    (each field value carries one rounding of relative size 2^-24; the pseudo-inverse spreads it with weights sum_t |P[t,k]|)."""
    shape = (14, 12, 10)
    fields, signals, (A, B, C) = _fields(shape)
    model = CorrespondenceModel()
    assert not model.is_fitted
    model.fit(fields, signals)
    assert model.is_fitted and model.timesteps == 10 and model.signal_n_dims == 2 and model.spatial_shape == shape
    n = 3 * int(np.prod(shape))
    assert model.coefficients.shape == (n, 2) and model.coefficients.dtype == np.float64
    assert model.mean_vector_field.shape == (n, 1) and model.mean_vector_field.dtype == np.float32
    assert model.mean_signal.shape == (2, 1) and model.signals.shape == (2, 10) and model.reference_phase == 2
    _, _, P = CorrespondenceModel.signals_pseudo_inverse(signals)
    umax = float(np.abs(fields).max())
    c = model.coefficients.reshape(3, *shape, 2)
    for k, truth in enumerate((A, B)):
        bound = np.abs(P[:, k]).sum() * (EPS32 * umax + 10 * EPS32 * umax)  # input rounding + the float32 mean the fields are centred on
        err = float(np.abs(c[..., k] - truth).max())
        print(f"coefficient column {k}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    for t in (0, 3, 7):
        got = model.predict(signals[t])
        assert got.shape == (3,) + shape and got.dtype == np.float64
        err = float(np.abs(got - fields[t]).max())
        print(f"predict(t={t}): max error {err:.3e}")
        assert err <= 16 * EPS32 * umax  # the field's own rounding, the mean's, and the two coefficients' errors above times |d| <= 1
        assert np.array_equal(model.predict_field32(signals[t]), got.astype(np.float32))


def test_fit_and_predict_against_the_reference_formulation():
    """The same model stated the way the reference holds its arrays (correspondence.py:170-202, 217-221): float32 fields as a
    (3N, T) matrix, np.mean, float32 centring, `@` for both products.  Bounds from the formats, not from the result: the float32
    mean of T values carries at most T roundings of relative size 2^-24 on values up to max|u|; a coefficient is a sum over t of
    centred values (one more rounding each, 2^-24 max|u - mean|, plus the mean's error) weighted with |P[t,k]|."""
    shape = (64, 60, 52)  # 599 040 elements
    fields, signals, _ = _fields(shape, seed=9)
    T = fields.shape[0]
    model = CorrespondenceModel().fit(fields, signals)
    # the reference's statement
    vf = fields.reshape(T, -1).T
    ref_mean = np.mean(vf, axis=1, keepdims=True)
    sg = signals.reshape(T, -1).T
    ref_mean_signal = np.mean(sg, axis=1, keepdims=True)
    centred_fields, centred_signals = vf - ref_mean, sg - ref_mean_signal
    assert centred_fields.dtype == np.float32
    P = centred_signals.T @ np.linalg.inv(centred_signals @ centred_signals.T)  # well conditioned: no regularisation
    assert np.linalg.cond(centred_signals @ centred_signals.T) < 30
    ref_coefficients = centred_fields @ P
    assert np.array_equal(model.mean_signal, ref_mean_signal) and np.array_equal(model.signals, sg)
    umax = float(np.abs(fields).max())
    cmax = float(np.abs(centred_fields).max())
    err = float(np.abs(model.mean_vector_field.astype(np.float64) - ref_mean).max())
    print(f"mean: max difference {err:.3e}, bound {T * EPS32 * umax:.3e}")
    assert err <= T * EPS32 * umax
    for k in range(2):
        bound = np.abs(P[:, k]).sum() * (EPS32 * cmax + T * EPS32 * umax)
        err = float(np.abs(model.coefficients[:, k] - ref_coefficients[:, k]).max())
        print(f"coefficient column {k}: max difference {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    # predict: the engine's float32 field against float32(mean + coefficients @ d) from the SAME model arrays; a BLAS may fuse the
    # two-term product, which moves the float64 sum by one float64 ulp and -- rarely -- the float32 rounding by one float32 ulp
    for s in (np.array([0.3, -0.2]), signals[4], model.mean_signal[:, 0]):
        d = s[:, None] - model.mean_signal
        want = (model.mean_vector_field + model.coefficients @ d).astype(np.float32).reshape(3, *shape)
        got = model.predict_field32(s)
        differ = got != want
        print(f"predict_field32: {int(differ.sum())} of {got.size} elements differ")
        assert differ.sum() <= 1e-5 * got.size
        assert np.all(np.abs(got[differ].astype(np.float64) - want[differ]) <= np.maximum(np.spacing(np.abs(want[differ])), np.spacing(np.abs(got[differ]))).astype(np.float64))
    assert np.array_equal(model.predict_field32(model.mean_signal[:, 0]), model.mean_vector_field.reshape(3, *shape))  # d = 0: the mean


def test_regularisation_follows_the_reference_loop():
    """The host part of fit (correspondence.py:97-147, 185-200), on a ten-phase signal s = 1/2 + 1/2 cos(2 pi t / 10)."""
    t = np.arange(10)
    s = 0.5 + 0.5 * np.cos(2 * np.pi * t / 10)

    def covariance(signals):
        c = signals.T - signals.T.mean(axis=1, keepdims=True)
        return c @ c.T

    # collinear signals (s, 2 s): rank 1, the Tikhonov loop runs until the condition number is <= 30
    collinear = np.stack([s, 2 * s], axis=1)
    cov = covariance(collinear)
    reg = CorrespondenceModel._regularize_matrix(cov)
    added = float((reg - cov)[0, 0])
    print(f"collinear: added {added:.6f}, condition number {np.linalg.cond(reg):.4f}")
    assert np.allclose(reg - cov, np.eye(2) * added) and abs(added - 0.216) < 1e-9
    assert abs(np.linalg.cond(reg) - 29.94) < 0.01 and np.linalg.cond(cov + np.eye(2) * (added - 1e-3)) > 30
    _, _, P = CorrespondenceModel.signals_pseudo_inverse(collinear)
    c = collinear.T - collinear.T.mean(axis=1, keepdims=True)
    assert np.allclose(P, c.T @ np.linalg.inv(reg), rtol=0, atol=1e-12)
    # the same pair scaled by 10: the added value passes 1.0 before the condition number is reached
    with pytest.raises(RuntimeError):
        CorrespondenceModel.signals_pseudo_inverse(10 * collinear)
    # a well conditioned pair is left alone
    good = np.stack([s, -np.pi / 10 * np.sin(2 * np.pi * t / 10)], axis=1)
    assert np.array_equal(CorrespondenceModel._regularize_matrix(covariance(good)), covariance(good))
    # a constant signal does not raise: one step of 1e-3 gives condition number 1; all coefficients zero, predict = the mean
    fields = np.random.default_rng(1).normal(size=(10, 3, 5, 4, 3)).astype(np.float32)
    model = CorrespondenceModel().fit(fields, np.full((10, 2), 0.75))  # 0.75: np.mean of the ten values is exact, the centred signal is 0
    assert np.array_equal(model.coefficients, np.zeros((180, 2)))
    assert np.array_equal(model.predict_field32(np.array([0.1, 2.0])), model.mean_vector_field.reshape(3, 5, 4, 3))
    # T = 3 time steps of a K = 5 signal: the T x T branch
    sig = np.random.default_rng(2).uniform(0, 1, size=(3, 5))
    signals, mean_signal, P = CorrespondenceModel.signals_pseudo_inverse(sig)
    assert signals.shape == (5, 3) and mean_signal.shape == (5, 1) and P.shape == (3, 5)
    c = sig.T - sig.T.mean(axis=1, keepdims=True)
    gram = c.T @ c
    assert gram.shape == (3, 3) and np.linalg.matrix_rank(gram) < 3  # centring removes one rank: regularised
    reg = CorrespondenceModel._regularize_matrix(gram)
    assert np.linalg.cond(reg) <= 30 and np.allclose(P, np.linalg.inv(reg) @ c.T, rtol=0, atol=1e-12)
    model = CorrespondenceModel().fit(fields[:3], sig)
    assert model.coefficients.shape == (180, 5) and model.timesteps == 3 and model.signal_n_dims == 5


def test_save_and_load_use_the_reference_file_format(tmp_path):
    fields, signals, _ = _fields((6, 5, 4))
    model = CorrespondenceModel().fit(fields, signals, reference_phase=4)
    # the hash, computed here over the documented byte sequence
    h = hashlib.sha256()
    for part in (model.coefficients.tobytes(), bytes([10]), model.mean_signal.tobytes(), model.mean_vector_field.tobytes(),
                 np.ascontiguousarray(model.signals).tobytes(), bytes([4])):
        h.update(part)
    assert model.model_hash == h.hexdigest()
    path = model.save(tmp_path / "model.anything")
    assert path == tmp_path / f"model_{h.hexdigest()[:7]}.pkl" and path.is_file()
    plain = model.save(tmp_path / "plain", include_model_hash=False)
    assert plain == tmp_path / "plain.pkl" and plain.is_file()
    with open(path, "rb") as f:
        data = pickle.load(f)  # a plain dict of arrays and numbers: readable without this package
    assert type(data) is dict and list(data) == REFERENCE_KEYS
    assert data["timesteps"] == 10 and data["signal_n_dims"] == 2 and tuple(data["spatial_shape"]) == (6, 5, 4) and data["reference_phase"] == 4
    loaded = CorrespondenceModel.load(path)
    for key in REFERENCE_KEYS:
        a, b = getattr(model, key), getattr(loaded, key)
        if isinstance(a, np.ndarray):
            assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), key
        else:
            assert a == b, key
    assert loaded.is_fitted and loaded.model_hash == model.model_hash
    s = np.array([0.4, 0.1])
    assert np.array_equal(loaded.predict_field32(s), model.predict_field32(s))
    # a file as the reference writes it (numpy scalars among the values, a float64 mean) loads too
    as_reference = dict(data, timesteps=np.int64(10), mean_vector_field=data["mean_vector_field"].astype(np.float64))
    with open(tmp_path / "ref.pkl", "wb") as f:
        pickle.dump(as_reference, f)
    ref = CorrespondenceModel.load(tmp_path / "ref.pkl")
    assert ref.mean_vector_field.dtype == np.float64 and np.array_equal(ref.predict_field32(s), model.predict_field32(s))

    # a pickle that names any other global is refused before anything of it runs
    class Sneaky:
        def __reduce__(self):
            return (print, ("this must never be printed",))

    for payload in (dict(data, coefficients=Sneaky()), Sneaky()):
        with open(tmp_path / "bad.pkl", "wb") as f:
            pickle.dump(payload, f)
        with pytest.raises(pickle.UnpicklingError):
            CorrespondenceModel.load(tmp_path / "bad.pkl")
    with open(tmp_path / "other.pkl", "wb") as f:
        pickle.dump({"weights": 1}, f)
    with pytest.raises(pickle.UnpicklingError):
        CorrespondenceModel.load(tmp_path / "other.pkl")


def test_predict_checks_state_and_shape():
    model = CorrespondenceModel()
    with pytest.raises(RuntimeError):
        model.predict(np.array([0.1, 0.2]))
    with pytest.raises(RuntimeError):
        model.model_hash
    fields, signals, _ = _fields((4, 4, 4))
    model.fit(fields, signals)
    for bad in (np.array([0.1]), np.array([0.1, 0.2, 0.3]), np.array([[0.1, 0.2]]), np.array(0.1)):
        with pytest.raises(ValueError):
            model.predict(bad)
        with pytest.raises(ValueError):
            model.predict_field32(bad)
    with pytest.raises(ValueError):
        model.fit(fields[:, :2], signals)
    with pytest.raises(ValueError):
        model.fit(fields, signals[:9])


def test_model_is_part_of_the_package_and_the_abi():
    assert "correspondence" in cases.pkg.__all__
    for name in ("mcgpu_correspondence_set", "mcgpu_correspondence_fit", "mcgpu_correspondence_predict", "mcgpu_warp_geometry_signal",
                 "mcgpu_correspondence_clear"):
        assert name in cases.pkg.engine.ABI_SYMBOLS
