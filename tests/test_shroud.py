"""The projection-derived breathing signal without a GPU: the C layout of the ABI structs, every refusal of the
entry points (the options are checked before the first device call), the argument check of reconstruct_4d(extract_signal=True), and
the float64 restatement (tests/shroud_ref.py) on the `breathing` fixture and on an integer-valued stack."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_layout
import cases
import shroud_ref as R

pkg = cases.pkg
shroud = pkg.shroud
recon = pkg.reconstruction


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """Field names in the header's order; sizeof and every offsetof / size as the C compiler lays the header out; the entry points are
    declared and exported."""
    mirrors = [("mcgpu_shroud_options", shroud._ShroudOptions), ("mcgpu_shroud_report", shroud._ShroudReport)]
    abi_layout.assert_field_names(mirrors)
    header = abi_layout.HEADER.read_text()
    for name in ("mcgpu_shroud_extract", "mcgpu_shroud_signal", "mcgpu_shroud_rows_device"):
        assert re.search(r"int %s\(" % name, header) and name in pkg.engine.ABI_SYMBOLS, name
    cc = abi_layout.c_compiler()
    if cc is not None:
        abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    print("mirrors:", [m[0] for m in mirrors], "C compiler:", cc)


def _options(**fields):
    o = shroud._ShroudOptions(C.sizeof(shroud._ShroudOptions), n_proj=3, nu=8, nv=10, u_first=0, u_count=0, v_first=0, v_count=0, unsharp=3, max_shift=2, device=0)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def test_every_refusal_comes_without_a_device():
    """A bad size, an ROI outside the image, an even unsharp, 2 max_shift >= m, null pointers, a report too short to hold its size: each
    returns -1 with a message, and none of them reaches a HIP call (this test runs without a GPU)."""
    engine, lib = shroud._library()
    P = np.zeros((3, 10, 8), dtype=np.float32)
    A = np.zeros((3, 10), dtype=np.float32)
    costs, signal = np.zeros((2, 5)), np.zeros(3)

    def extract(o, p=P.ctypes.data, sig=signal.ctypes.data, report=None):
        return lib.mcgpu_shroud_extract(C.byref(o) if o is not None else None, p, A.ctypes.data, costs.ctypes.data, sig, report)

    def from_shroud(o, a=A.ctypes.data, sig=signal.ctypes.data, report=None):
        return lib.mcgpu_shroud_signal(C.byref(o) if o is not None else None, a, costs.ctypes.data, sig, report)

    def rows_device(o, p=1 << 20, d=1 << 20):
        return lib.mcgpu_shroud_rows_device(C.byref(o), p, d, None)

    bad_options = [dict(struct_size=0), dict(n_proj=0), dict(nu=0), dict(nv=-1), dict(u_first=-1), dict(u_first=8), dict(u_first=4, u_count=5), dict(u_count=-1),
                   dict(v_first=-1), dict(v_first=10), dict(v_first=6, v_count=5), dict(v_count=-2), dict(unsharp=4), dict(unsharp=-1), dict(max_shift=-1),
                   dict(max_shift=5), dict(v_first=2, v_count=4, max_shift=2), dict(device=-1)]
    for fields in bad_options:
        assert extract(_options(**fields)) == -1, fields
        message = lib.mcgpu_last_error().decode()
        assert "mcgpu_shroud_extract" in message, (fields, message)
    assert extract(None) == -1
    assert extract(_options(), p=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert extract(_options(), sig=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    short = shroud._ShroudReport(4)
    assert extract(_options(), report=C.byref(short)) == -1 and "struct_size" in lib.mcgpu_last_error().decode()

    # stages B and C alone: the shape is (n_proj, v_count); the other fields are not read
    for fields in (dict(struct_size=0), dict(n_proj=0, v_count=10), dict(v_count=0), dict(v_count=10, max_shift=5), dict(v_count=10, max_shift=-1),
                   dict(v_count=4, max_shift=2), dict(v_count=10, device=-1)):
        assert from_shroud(_options(**fields)) == -1, fields
        assert "mcgpu_shroud_signal" in lib.mcgpu_last_error().decode()
    assert from_shroud(_options(v_count=10), a=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert from_shroud(_options(v_count=10), sig=None) == -1 and "null pointer" in lib.mcgpu_last_error().decode()
    assert from_shroud(_options(v_count=10), report=C.byref(short)) == -1

    # the row sums of a resident stack
    for fields in (dict(struct_size=0), dict(nu=0), dict(u_first=8), dict(v_first=6, v_count=5), dict(unsharp=2)):
        assert rows_device(_options(**fields)) == -1, fields
    assert rows_device(_options(), p=None) == -1 and rows_device(_options(), d=None) == -1


def test_python_checks_its_arguments():
    P = np.zeros((3, 10, 8), dtype=np.float32)
    for kwargs, match in ((dict(unsharp=4), "unsharp"), (dict(max_shift=5), "max_shift"), (dict(rows=(6, 5)), "rows"), (dict(columns=(-1, 4)), "columns"),
                          (dict(columns=(0, 0)), "columns"), (dict(rows=(2, 4), max_shift=2), "max_shift")):
        with pytest.raises(ValueError, match=match):
            shroud.extract_signal(P, **{"unsharp": 3, "max_shift": 2, **kwargs})
    with pytest.raises(ValueError, match="stack"):
        shroud.amsterdam_shroud(np.zeros((10, 8)))
    with pytest.raises(ValueError, match="max_shift"):
        shroud.shroud_signal(np.zeros((3, 10)), max_shift=5)
    with pytest.raises(ValueError, match="shroud of shape"):
        shroud.shroud_signal(np.zeros(10))
    assert shroud.check_parameters((3, 10, 8), 17, 4, None, (3, 4)) == (3, 8, 10, 3, 4, 0, 10, 17, 4)
    x = np.array([0.0, 2.0, 1.0, 5.0])
    assert np.array_equal(shroud.finish_signal(x, detrend=False, invert=True), -x)
    assert np.allclose(shroud.finish_signal(x), R.detrend_linear(x), atol=1e-12)


def test_reconstruct_4d_refuses_a_signal_beside_extract_signal(tmp_path):
    with pytest.raises(ValueError, match="extract_signal"):
        recon.reconstruct_4d(tmp_path / "p.mha", tmp_path / "g.xml", extract_signal=True, amplitude_signal=np.ones(4))
    with pytest.raises(ValueError, match="extract_signal"):
        recon.reconstruct_4d(tmp_path / "p.mha", tmp_path / "g.xml", extract_signal=True, phase_signal=np.ones(4))
    with pytest.raises(ValueError, match="unknown extraction parameters"):
        recon.reconstruct_4d(tmp_path / "p.mha", tmp_path / "g.xml", extract_signal=True, shroud=dict(width=9))
    with pytest.raises(ValueError, match="exactly one"):  # the default stays as it is
        recon.reconstruct_4d(tmp_path / "p.mha", tmp_path / "g.xml")


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_recovers_the_breathing_fixture():
    """unsharp 9, max_shift 8: the detrended signal correlates with the truth at >= 0.95 (0.972 here), its local maxima (8, 38, 68, 98)
    lie within one projection of the truth's (8, 38, 67, 98), and every pair's minimum is well defined: the runner-up cost is > 1.001 x
    the minimum (1.18 at the least) and den >= 1e-4 x the pair's largest cost -- the precondition under which the device test compares
    shifts exactly.  The amplitude is 1.4 to 2.3 x the truth's with the mask and 0.87 x without: it is not calibrated."""
    P, truth = R.breathing(), R.breathing_truth()
    assert P.shape == (120, 48, 40) and P.dtype == np.float32
    assert R.local_maxima(truth) == R.BREATHING_TRUTH_MAXIMA
    c = R.costs(R.shroud(P, 9), 8)
    k, _, den = R.shifts(c)
    x = R.detrend_linear(R.signal_from_costs(c))
    correlation = float(np.corrcoef(x, truth)[0, 1])
    ordered = np.sort(c, axis=1)
    runner_up = float((ordered[:, 1] / ordered[:, 0]).min())
    print(f"correlation {correlation:.4f}, maxima {R.local_maxima(x)}, runner-up ratio {runner_up:.4f}, least den / max cost {np.nanmin(den / c.max(axis=1)):.4g}")
    assert correlation >= 0.95
    maxima = R.local_maxima(x)
    assert len(maxima) == len(R.BREATHING_TRUTH_MAXIMA) and all(abs(a - b) <= 1 for a, b in zip(maxima, R.BREATHING_TRUTH_MAXIMA))
    assert runner_up > 1.001
    assert np.all(np.abs(k) < 8) and np.all(den >= 1e-4 * c.max(axis=1))
    # the figures without the mask, as recorded
    x0 = R.detrend_linear(R.signal(P, 0, 8))
    assert abs(np.corrcoef(x0, truth)[0, 1] - 0.981) < 2e-3 and abs(x0.std() / truth.std() - 0.87) < 0.01
    assert 1.4 <= x.std() / truth.std() <= 2.3


def test_row_sums_commute_with_the_difference_on_integers():
    """On an integer-valued stack every float32 difference and every float64 sum is exact, so D equals half the central difference of
    the float64 row sums exactly: the rule's sum of differences is the difference of sums wherever rounding does not stand between."""
    rng = np.random.default_rng(5)
    P = rng.integers(-1000, 1000, size=(4, 9, 37)).astype(np.float32)
    sums = P.astype(np.float64)[:, :, 3:33].sum(axis=2)
    v = np.arange(9)
    want = 0.5 * (sums[:, np.minimum(v + 1, 8)] - sums[:, np.maximum(v - 1, 0)])
    assert np.array_equal(R.row_sums(P, columns=(3, 30)), want)
    assert np.array_equal(R.row_sums(P, rows=(2, 5), columns=(3, 30)), want[:, 2:7])  # the clamp is to the image, not to the ROI
    assert np.array_equal(R.unsharp_mask(want, 0), want.astype(np.float32)) and not R.unsharp_mask(want, 1).any()


def test_crafted_columns_have_exact_answers():
    """Identical columns: shift exactly 0 (c(-1) = c(1)).  A staircase displaced by +3 rows: c(3) = 0 and c(2) = c(4), so the refined
    shift is exactly 3 with den > 0.  A minimum on the border of the search range is not refined."""
    before, after = R.displaced_staircase()
    c = R.costs(np.stack([before, after]), 8)
    k, shift, den = R.shifts(c)
    assert k[0] == 3 and c[0, 8 + 3] == 0.0 and c[0, 8 + 2] == c[0, 8 + 4] == 0.5 and den[0] == 1.0 and shift[0] == 3.0
    k, shift, den = R.shifts(R.costs(np.stack([after, after]), 8))
    assert k[0] == 0 and shift[0] == 0.0 and den[0] > 0
    k, shift, den = R.shifts(R.costs(np.stack([before, after]), 3))
    assert k[0] == 3 and shift[0] == 3.0 and np.isnan(den[0])
    assert np.array_equal(R.signal_from_costs(np.zeros((0, 5))), [0.0])
    assert R.shifts(np.array([[1.0, 0.5, 0.5, 2.0, 3.0]]))[0][0] == -1  # a tie goes to the lowest s
