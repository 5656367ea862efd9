"""The projection-derived breathing signal on the device (csrc/shroud.hip) against its float64 restatement
(tests/shroud_ref.py).

Stage A: |A_hip - A_ref| <= max(1 float32 ulp of A_ref, 1e-10 x max|D_ref|): a float64 sum of at most 4096 terms plus one float32
rounding.  Stages B and C: costs within 1e-12 relative (float64 sums of at most 4096 non-negative terms), the integer argmin equal and
the refined shift within 1e-6 rows, under the precondition that tests/test_shroud.py asserts of the restatement (runner-up cost > 1.001
x the minimum, den >= 1e-4 x the pair's largest cost) and that is asserted here of every crafted shroud too."""
import numpy as np
import pytest

import cases
import shroud_ref as R

pytestmark = pytest.mark.gpu

shroud = cases.pkg.shroud
recon = cases.pkg.reconstruction
phase_mod = cases.pkg.phase

BATCH = shroud.UPLOAD_BATCH


def _stack(n, nv, nu, seed=0):
    return np.random.default_rng(1000 * n + 10 * nv + nu + seed).normal(size=(n, nv, nu)).astype(np.float32)


def _assert_stage_a(P, unsharp, rows=None, columns=None):
    got, report = shroud.amsterdam_shroud(P, unsharp=unsharp, rows=rows, columns=columns)
    D = R.row_sums(P, rows, columns)
    want = R.unsharp_mask(D, unsharp)
    assert got.dtype == np.float32 and got.shape == want.shape
    bound = np.maximum(np.spacing(np.abs(want)).astype(np.float64), 1e-10 * np.abs(D).max())
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"stage A {P.shape} unsharp {unsharp} rows {rows} columns {columns}: max error {err.max():.3g}, least bound {bound.min():.3g}, "
          f"equal bytes: {np.array_equal(got, want)}")
    assert np.all(err <= bound)
    assert report["peak_device_bytes"] >= min(P.shape[0], BATCH) * P[0].nbytes and report["ms_shroud"] > 0
    return got


# (n, nv, nu, unsharp, rows, columns): the smallest shapes at which the kernel takes another path
STAGE_A_CASES = {
    "nu1": (3, 7, 1, 0, None, None),
    "nu37_scalar_tail": (3, 7, 37, 0, None, None),
    "nu37_columns_3_30": (3, 7, 37, 0, None, (3, 30)),
    "nu40_vector_head1_tail1": (3, 7, 40, 0, None, (3, 30)),           # 16-byte body 4 .. 31, column 3 before and 32 after it
    "nu40_vector_head3_tail3": (3, 7, 40, 0, None, (1, 38)),
    "nu8_no_body": (3, 7, 8, 0, None, (1, 2)),                          # fewer columns than one 16-byte load
    "nu1030_two_spans_scalar": (2, 5, 1030, 0, None, None),            # 6 columns past a workgroup's 1024
    "nu1032_two_spans_vector": (2, 5, 1032, 0, None, None),            # 258 float4: 2 past a workgroup's 256
    "nu1032_one_full_span_head3_tail3": (2, 5, 1032, 0, None, (1, 1030)),
    "nu2060_three_spans": (2, 3, 2060, 0, None, (5, 2051)),
    "nv1": (3, 1, 12, 0, None, None),
    "nv2_both_clamp": (3, 2, 12, 0, None, None),
    "nv3_both_clamp": (3, 3, 12, 0, None, None),
    "rows_interior": (3, 40, 12, 0, (5, 9), None),
    "rows_top_edge": (3, 40, 12, 0, (0, 6), None),
    "rows_bottom_edge": (3, 40, 12, 0, (34, 6), None),
    "rows_three_bands_last_partial": (2, 75, 12, 0, (3, 70), None),    # bands of 32, 32 and 6 rows, 6 no multiple of the 4 reduced together
    "rows_two_bands_whole_image": (2, 33, 9, 0, None, None),
    "n1": (1, 9, 12, 17, None, None),
    "n5_window_wider_than_the_stack": (5, 9, 12, 17, None, None),
    "n_batch_plus_one": (BATCH + 1, 6, 8, 5, None, None),
    "n_two_batches_plus_one_scalar": (2 * BATCH + 1, 4, 7, 3, None, None),
    "unsharp0": (20, 9, 12, 0, None, None),
    "unsharp1_all_zeros": (20, 9, 12, 1, None, None),
    "unsharp17": (20, 9, 12, 17, None, None),
}


@pytest.mark.parametrize("name", list(STAGE_A_CASES))
def test_stage_a_equals_the_restatement(engine, name):
    n, nv, nu, unsharp, rows, columns = STAGE_A_CASES[name]
    got = _assert_stage_a(_stack(n, nv, nu), unsharp, rows, columns)
    if unsharp == 1:
        assert not got.any()
    if rows is not None and columns is None and unsharp == 0:  # the clamp is to the image: an ROI is a slice of the whole shroud
        whole, _ = shroud.amsterdam_shroud(_stack(n, nv, nu), unsharp=0)
        assert np.array_equal(got, whole[:, rows[0]:rows[0] + rows[1]])


def test_stage_a_sums_in_float64(engine):
    """1000 + small structure, 4096 columns: every float32 difference is a multiple of 2^-14 and the sums pass 1024, so the float64 sum
    is exact while a running float32 sum drops bits from there on: it misses the bound on every row (by 2 to 20 x), which is what
    forces the float64 accumulation."""
    rng = np.random.default_rng(7)
    v = np.arange(5)
    P = (1000.0 + 0.37 * v[None, :, None] + rng.uniform(0, 0.01, size=(2, 5, 4096))).astype(np.float32)
    _assert_stage_a(P, 0)
    D = R.row_sums(P)
    t = P[:, np.minimum(v + 1, 4)] - P[:, np.maximum(v - 1, 0)]
    in_float32 = 0.5 * np.cumsum(t, axis=2, dtype=np.float32)[:, :, -1].astype(np.float64)
    bound = np.maximum(np.spacing(np.abs(D.astype(np.float32))).astype(np.float64), 1e-10 * np.abs(D).max())
    assert np.all(np.abs(in_float32 - D) > bound)


# ---------------------------------------------------------------------------------------------------------------- stages B and C
def _bumps(m, centres, width):
    r = np.arange(m)
    return np.exp(-(r[None, :] - np.asarray(centres, dtype=np.float64)[:, None]) ** 2 / width).astype(np.float32)


def _assert_signal(A, S, precondition=True):
    got_x, got_c, report = shroud.shroud_signal(A, max_shift=S)
    want_c = R.costs(A, S)
    k, shift, den = R.shifts(want_c)
    assert got_c.shape == want_c.shape and got_x.shape == (A.shape[0],) and got_x[0] == 0.0
    if want_c.size:
        rel = np.abs(got_c - want_c) / np.where(want_c > 0, want_c, 1.0)
        print(f"stages B, C {A.shape} S {S}: costs max relative error {rel.max():.3g}")
        assert np.all(np.abs(got_c - want_c) <= 1e-12 * want_c)
        if precondition and S > 0:
            ordered = np.sort(want_c, axis=1)
            assert np.all(ordered[:, 1] > 1.001 * ordered[:, 0])
            interior = np.abs(k) < S
            assert np.all(den[interior] >= 1e-4 * want_c.max(axis=1)[interior])
        assert np.array_equal(np.argmin(got_c, axis=1) - S, k)
    assert np.all(np.abs(np.diff(got_x) - shift) <= 1e-6)
    assert np.all(np.abs(got_x - R.signal_from_costs(want_c)) <= 1e-6 * max(A.shape[0] - 1, 1))
    return got_x, got_c


@pytest.mark.parametrize("S", [0, 4, 10])
def test_costs_and_shifts_of_crafted_columns(engine, S):
    """m = 21: S = 10 = (m - 1) // 2 is the largest shift the rule admits; S = 0 leaves nothing to refine."""
    x, _ = _assert_signal(_bumps(21, 10 + np.array([0, 1.3, 2.1, 0.4, -1.2, -0.5]), 8.0), S)
    assert (S == 0) == (not x.any())


def test_costs_of_columns_longer_than_a_wave(engine):
    """m = 150: every lane of the cost kernel takes two or three rows; S = 16, the default."""
    _assert_signal(_bumps(150, 70 + 6 * np.sin(0.9 * np.arange(9)), 50.0), 16)


def test_one_and_two_columns(engine):
    A = _bumps(21, [10.0, 11.3], 8.0)
    x, c, _ = shroud.shroud_signal(A[:1], max_shift=4)
    assert np.array_equal(x, [0.0]) and c.shape == (0, 9)
    x, _ = _assert_signal(A, 4)
    assert x.shape == (2,) and abs(x[1] - 1.3) < 0.5


def test_identical_and_displaced_columns_have_exact_shifts(engine):
    """Identical columns: c(0) = 0 and c(-1) = c(1), shift exactly 0.  The staircase displaced by +3 rows: c(3) = 0 exactly and c(2) =
    c(4) = 0.5 (integer sums, equal rationals), so the refined shift is exactly 3 with den = 1 > 0."""
    before, after = R.displaced_staircase()
    x, c = _assert_signal(np.stack([before, after]), 8, precondition=False)
    assert c[0, 8 + 3] == 0.0 and c[0, 8 + 2] == 0.5 and c[0, 8 + 4] == 0.5 and x[1] == 3.0
    x, c = _assert_signal(np.stack([after, after, after]), 8, precondition=False)
    assert c[0, 8] == 0.0 and c[0, 7] == c[0, 9] > 0 and np.array_equal(x, [0.0, 0.0, 0.0])
    x, _ = _assert_signal(np.stack([before, after]), 3, precondition=False)  # the minimum on the border: not refined
    assert x[1] == 3.0


def test_breathing_through_the_signal_entry(engine):
    _assert_signal(R.shroud(R.breathing(), 9), 8)


# ---------------------------------------------------------------------------------------------------------------- the whole call
def test_two_calls_give_the_same_bytes(engine):
    P = _stack(BATCH + 3, 21, 1032, seed=3)[:, :, :1031]  # not contiguous: the binding copies it; nu = 1031, the scalar path, two spans
    for stack in (P, np.ascontiguousarray(_stack(BATCH + 3, 21, 1032, seed=3))):
        first = shroud._extract(stack, 5, 4, (2, 17), None, 0, True, True)
        second = shroud._extract(stack, 5, 4, (2, 17), None, 0, True, True)
        for a, b in zip(first[:3], second[:3]):
            assert a.tobytes() == b.tobytes()
        assert np.abs(first[2]).max() > 0


@pytest.fixture(scope="module")
def breathing_signals(engine):
    """(device signal, restated signal), both detrended, unsharp 9, max_shift 8."""
    P = R.breathing()
    raw = shroud.extract_signal(P, unsharp=9, max_shift=8, detrend=False)
    want_raw = R.signal(P, 9, 8)
    assert np.all(np.abs(np.diff(raw) - np.diff(want_raw)) <= 1e-6)
    got = shroud.extract_signal(P, unsharp=9, max_shift=8)
    assert np.array_equal(got, phase_mod.detrend_linear(raw)) and np.array_equal(shroud.extract_signal(P, unsharp=9, max_shift=8, invert=True), -got)
    return got, R.detrend_linear(want_raw)


def test_extract_signal_recovers_the_breathing_fixture(breathing_signals):
    got, want = breathing_signals
    assert np.all(np.abs(got - want) <= 1e-6 * got.size)
    pieces = phase_mod.calculate_phase(got)
    assert sum(p.size for p in pieces) == got.size and np.isfinite(np.hstack(pieces)).all()
    peaks = [int(p) for p in phase_mod.find_peaks(got) if 0 < p < got.size - 1]
    print("peaks", peaks, "local maxima", R.local_maxima(got), "correlation", float(np.corrcoef(got, R.breathing_truth())[0, 1]))
    for found in (peaks, R.local_maxima(got)):
        assert len(found) == 4 and all(abs(a - b) <= 1 for a, b in zip(found, R.BREATHING_TRUTH_MAXIMA))
    assert np.corrcoef(got, R.breathing_truth())[0, 1] >= 0.95


def _tiny_geometry(n):
    g = recon.CircularGeometry(300.0, 500.0)
    for k in range(n):
        g.add_projection(17.0 + k * 360.0 / n, 0.0, 0.0)
    return g


def test_rooster4d_takes_the_extracted_phase(engine, breathing_signals):
    """16^3 voxels, one iteration of everything: fed the phase of the extracted signal, rooster4d gives the bytes it gives for the
    restatement's phase whenever the two signals are equal to the last bit; else the phases agree within 1e-6 and the volumes are not
    compared bit for bit (a phase that differs in its last bits moves the interpolation weights, and with them the volume)."""
    got, want = breathing_signals
    ph_got, ph_want = recon._unit_phase(got, None), recon._unit_phase(want, None)
    P, geo = R.breathing(), _tiny_geometry(R.BREATHING_N)
    kwargs = dict(dimension=(16, 16, 16), spacing=(4.0, 4.0, 4.0), frames=3, niter=1, cgiter=1, tviter=1)
    vol, report = recon.rooster4d(P, geo, (3.0, 3.0), None, ph_got, **kwargs)
    assert vol.shape == (3, 16, 16, 16) and np.isfinite(vol).all() and vol.max() > 0
    if np.array_equal(got, want):
        ref, _ = recon.rooster4d(P, geo, (3.0, 3.0), None, ph_want, **kwargs)
        assert vol.tobytes() == ref.tobytes()
    else:
        print(f"signals differ by at most {np.abs(got - want).max():.3g} rows: phases compared, volumes not")
        assert np.all(np.abs(ph_got - ph_want) <= 1e-6)


def test_reconstruct_4d_extracts_its_signal(engine, tmp_path, breathing_signals):
    """The file flow with extract_signal=True: the volume is the one that the extracted amplitude gives, the .yaml records the source of
    the signal and every extraction parameter."""
    import yaml
    P, geo = R.breathing(), _tiny_geometry(R.BREATHING_N)
    gpath = geo.write(tmp_path / "geometry.xml")
    ppath = recon.write_mha(tmp_path / "projections_total_normalized.mha", P, (3.0, 3.0, 1.0), (-(R.BREATHING_NU - 1) / 2 * 3.0, -(R.BREATHING_NV - 1) / 2 * 3.0, 0.0))
    kwargs = dict(dimension=(16, 16, 16), spacing=(4.0, 4.0, 4.0), frames=3, niter=1, cgiter=1, tviter=1)
    out, _ = recon.reconstruct_4d(ppath, gpath, extract_signal=True, shroud=dict(unsharp=9, max_shift=8), **kwargs)
    params = yaml.safe_load(out.with_suffix(".yaml").read_text())
    assert params["signal"] == "shroud"
    assert params["shroud"] == dict(unsharp=9, max_shift=8, rows=None, columns=None, detrend=True, invert=False, gpu_id=0)
    vol = recon.read_mha(out)[0]
    given, _ = recon.reconstruct_4d(ppath, gpath, output_filename="given.mha", amplitude_signal=breathing_signals[0], **kwargs)
    assert vol.tobytes() == recon.read_mha(given)[0].tobytes()
    assert "signal" not in yaml.safe_load(given.with_suffix(".yaml").read_text())
