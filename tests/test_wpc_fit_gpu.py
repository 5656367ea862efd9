"""mcgpu_wpc_fit (csrc/wpc_fit.hip) and water_precorrection.fit_wpc on the GPU, against the float64 restatement (tests/wpc_ref.py, on
oracle/fdk_oracle.py).  The slab means fbar_n are held to TOL = 2e-4 x max|oracle fbar_n| per power -- the project's FDK tolerance
(tests/test_fdk_configs.py) -- outside the pixels with a voxel of their slab column within 1e-3 pixel of a detector edge
(fdk_oracle.ambiguous_voxels; at most 5 % per case, tests/test_wpc_fit.py).

  centred          chunks 32 + 8; orders 1, 3, 5; the reduction, the coefficients, the public chain, determinism
  half_fan         offset -80 mm, pad 0.5, n = 41: chunks 32 + 9 and a last batch of one projection; slabs (0, 1), (0, 30), (27, 3);
                   orders 1 and 7; both ramp routes; the parent's route (N + 1 fdk() calls) beside the fused one; one slice of
                   the fused call against the same slice of fdk(), bit for bit
  wide             nx = 300 (a partial second x-block), ny = 1, off-centre origin; order 2
  varying_offsets  per-projection off_x and off_y; order 3"""
import numpy as np
import pytest

import cases
import wpc_ref as W

pkg = cases.pkg
wp = pkg.water_precorrection
recon = pkg.reconstruction

pytestmark = pytest.mark.gpu


def _route(monkeypatch, direct):
    if direct:
        monkeypatch.setenv("MCGPU_FDK_DIRECT_RAMP", "1")
    else:
        monkeypatch.delenv("MCGPU_FDK_DIRECT_RAMP", raising=False)


def _call(name, slab, order, layout=0):
    p = W.problem(name)
    return wp.normal_equations(*p.fdk_args(), p.weight, p.template, slab, order, p.origin, p.hann, p.hann_y, p.pad, channel_layout=layout)


def _errors(got, want, out):
    """max |got - want| per power outside the left-out pixels, as a fraction of max |want| of that power."""
    diff = np.where(out[None], 0.0, np.asarray(got, dtype=np.float64) - want)
    return np.abs(diff).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))


def _compare(name, slab, order, basis, label=""):
    want, out = W.oracle_basis(name, slab, max(o for n, s, o in W.GPU_CASES if (n, s) == (name, slab)))
    err = _errors(basis, want[: order + 1], out)
    print(f"{name} slab {slab} order {order}{label}: max |hip - oracle| / max |oracle| per power = {np.array2string(err, precision=2)} "
          f"outside {int(out.sum())} of {out.size} pixels")
    assert basis.shape == want[: order + 1].shape and basis.dtype == np.float32
    assert (err < W.TOL_REL).all(), err
    return err


# ---------------------------------------------------------------------------------------------------------------- basis means
@pytest.mark.parametrize("order", [1, 3, 5])
def test_centred(engine, order, monkeypatch):
    _route(monkeypatch, False)
    _compare("centred", W.CENTRED_SLAB, order, _call("centred", W.CENTRED_SLAB, order)[2])


@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
@pytest.mark.parametrize("order", [1, 7])
@pytest.mark.parametrize("slab", [(0, 1), (0, 30), (27, 3)], ids=["first", "all", "last3"])
def test_half_fan(engine, slab, order, direct, monkeypatch):
    _route(monkeypatch, direct)
    _compare("half_fan", slab, order, _call("half_fan", slab, order)[2], " direct" if direct else " fft")


def test_wide(engine, monkeypatch):
    _route(monkeypatch, False)
    _compare("wide", (0, 1), 2, _call("wide", (0, 1), 2)[2])


def test_varying_offsets(engine, monkeypatch):
    _route(monkeypatch, False)
    _compare("varying_offsets", (11, 8), 3, _call("varying_offsets", (11, 8), 3)[2])


@pytest.mark.parametrize("order", [1, 4, 7])
def test_both_channel_layouts_give_the_same_bytes(engine, order, monkeypatch):
    """Planes per power and powers interleaved per pixel feed the same arithmetic."""
    _route(monkeypatch, False)
    planes, interleaved = _call("half_fan", (27, 3), order, layout=1), _call("half_fan", (27, 3), order, layout=2)
    for x, y in zip(planes[:3], interleaved[:3]):
        assert x.tobytes() == y.tobytes()
    _compare("half_fan", (27, 3), order, planes[2], " planes")


# ---------------------------------------------------------------------------------------------------------------- the parent's route
def test_fused_route_against_the_composed_one(engine, monkeypatch):
    """fbar_n from N + 1 reconstruction.fdk(..., water_pre_correction=e_n) calls and a mean over the slab, beside the fused call:
    both within TOL of the oracle, and the fused error at most twice the composed one per power -- both are float32 sums of the
    same terms in another order, so they differ by rounding, not by a bias."""
    _route(monkeypatch, False)
    name, slab, order = "half_fan", (0, 30), 7
    p = W.problem(name)
    want, out = W.oracle_basis(name, slab, order)
    composed = np.stack([recon.fdk(*p.fdk_args(), p.origin, p.hann, p.hann_y, W.unit(n), pad=p.pad)[0][:, slab[0]: slab[0] + slab[1], :].mean(1)
                         for n in range(order + 1)])
    fused = _call(name, slab, order)[2]
    e_composed, e_fused = _errors(composed, want, out), _errors(fused, want, out)
    print(f"composed: {np.array2string(e_composed, precision=2)}\nfused:    {np.array2string(e_fused, precision=2)}")
    assert (e_composed < W.TOL_REL).all() and (e_fused < W.TOL_REL).all()
    assert (e_fused <= 2.0 * e_composed).all()


@pytest.mark.parametrize("layout", [1, 2], ids=["planes", "interleaved"])
@pytest.mark.parametrize("y", [0, 29])
def test_one_slice_equals_the_fdk_slice_bit_for_bit(engine, y, layout, monkeypatch):
    """A slab of one slice, order 1, direct ramp (so that hipFFT's batch size plays no part): basis_mean[n] has the bytes of
    fdk(..., water_pre_correction=e_n)[0][:, y, :].  Both routes cut the 41 projections into batches of 8, 8, 8, 8, 8, 1 in order and
    add one accumulator per launch; the division by y_count = 1 is exact; row filters, detector weight, power chain, column setup and
    detector sample are the same functions (csrc/backproject_column.inc, csrc/fdk_common.inc)."""
    _route(monkeypatch, True)
    p = W.problem("half_fan")
    basis = _call("half_fan", (y, 1), 1, layout)[2]
    for n in range(2):
        want = recon.fdk(*p.fdk_args(), p.origin, p.hann, p.hann_y, W.unit(n), pad=p.pad)[0][:, y, :]
        differing = int((basis[n].view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())
        print(f"y {y} layout {layout} power {n}: {differing} of {want.size} words differ")
        assert differing == 0


# ---------------------------------------------------------------------------------------------------------------- reduction, coefficients
def test_normal_equations_from_the_returned_basis(engine, monkeypatch):
    """B and a recomputed in float64 numpy from the basis the call returned: any order of summation of n terms in double stays
    within n 2^-52 sum |terms|."""
    _route(monkeypatch, False)
    p = W.problem("centred")
    B, a, basis, _ = _call("centred", W.CENTRED_SLAB, 5)
    f, w, t = basis.astype(np.float64), p.weight.astype(np.float64), p.template.astype(np.float64)
    B_ref, a_ref = W.normal_equations(f, w, t)
    eps = w.size * 2.0 ** -52
    B_bound = eps * np.einsum("zx,izx,jzx->ij", w, np.abs(f), np.abs(f))
    a_bound = eps * np.einsum("zx,izx,zx->i", w, np.abs(f), np.abs(t))
    print(f"max |B - B_ref| / bound = {(np.abs(B - B_ref) / B_bound).max():.3g}, max |a - a_ref| / bound = {(np.abs(a - a_ref) / a_bound).max():.3g}")
    assert (np.abs(B - B_ref) <= B_bound).all() and (np.abs(a - a_ref) <= a_bound).all()
    assert (B == B.T).all() and (np.diag(B) > 0).all()


def test_order_one_coefficients(engine, monkeypatch):
    """|c - c_ref| <= 4 TOL cond(B_ref) |c_ref|: the basis is within TOL per power, B and a are bilinear in it (a factor of 2
    each), and a relative perturbation of a linear system grows by at most the condition number.  cond = 47: 3.8 %."""
    _route(monkeypatch, False)
    p = W.problem("centred")
    fit = wp.fit_wpc(*p.fdk_args(), p.weight, p.template, W.CENTRED_SLAB, order=1, origin=p.origin, hann=p.hann, hann_y=p.hann_y, pad=p.pad)
    fbar, _ = W.oracle_basis("centred", W.CENTRED_SLAB, 5)
    B_ref, a_ref = W.normal_equations(fbar[:2], p.weight, p.template)
    c_ref = W.solve(B_ref, a_ref)
    bound = 4.0 * W.TOL_REL * np.linalg.cond(B_ref) * np.linalg.norm(c_ref)
    print(f"c = {fit.coefficients}, c_ref = {c_ref}, |c - c_ref| = {np.linalg.norm(fit.coefficients - c_ref):.3e}, bound {bound:.3e}; cond {fit.condition:.4g}")
    assert np.linalg.norm(fit.coefficients - c_ref) <= bound
    assert fit.condition == pytest.approx(np.linalg.cond(B_ref), rel=4.0 * W.TOL_REL * np.linalg.cond(B_ref))


# ---------------------------------------------------------------------------------------------------------------- the public chain
def test_fit_then_reconstruct_flattens_the_water(engine, monkeypatch):
    """fit_wpc at order 3, then reconstruction.fdk with the fitted polynomial: both water regions of the slab within 0.5 % of 0.02
    (float64: 0.04 % and 0.03 %; uncorrected 5.6 % and 1.6 %; float32 adds about sum |c_n| max |f_n| 2e-4 = 0.02 %)."""
    _route(monkeypatch, False)
    p = W.problem("centred")
    fit = wp.fit_wpc(*p.fdk_args(), p.weight, p.template, W.CENTRED_SLAB, order=3, origin=p.origin, hann=p.hann, hann_y=p.hann_y, pad=p.pad)
    assert fit.residual_fit <= fit.residual_identity
    assert fit.coefficients.shape == (4,) and fit.B.shape == (4, 4) and fit.basis_mean.shape == (4, 40, 40)
    assert fit.report["ms_total"] > 0 and fit.report["peak_device_bytes"] > p.proj[:32].nbytes
    first, count = W.CENTRED_SLAB
    plain = recon.fdk(*p.fdk_args(), p.origin, p.hann, p.hann_y, None, pad=p.pad)[0][:, first: first + count, :].mean(1)
    fixed = recon.fdk(*p.fdk_args(), p.origin, p.hann, p.hann_y, fit.coefficients, pad=p.pad)[0][:, first: first + count, :].mean(1)
    for region, off in ((p.r < 20.0, 0.056), ((p.r > 35.0) & (p.r < 48.0), 0.016)):
        before, after = plain[region].mean(), fixed[region].mean()
        print(f"water mean {before:.6f} -> {after:.6f}; residual {fit.residual_identity:.3e} -> {fit.residual_fit:.3e}; cond {fit.condition:.3g}")
        assert abs(before - 0.02) / 0.02 == pytest.approx(off, abs=0.002)
        assert abs(after - 0.02) <= 0.005 * 0.02


def test_fit_wpc_phantom_reads_files_and_writes_the_record(engine, monkeypatch, tmp_path):
    """Files in, WPCFit and wpc.yaml out, on a small water phantom whose projections are the two-energy chords of `centred`'s kind."""
    import yaml
    _route(monkeypatch, False)
    phantom = pkg.geometry.MCWaterPhantomGeometry(shape=(40, 40, 12), image_spacing=(4.0, 4.0, 4.0), radius=60.0, length=48.0)
    p = W.problem("centred")
    recon.write_mha(tmp_path / "projections_total_normalized.mha", p.proj, (p.du, p.dv, 1.0), (p.u0, p.v0, 0.0))
    recon.save_geometry(p.geo, tmp_path / "geometry.xml")
    fit = wp.fit_wpc_phantom(tmp_path / "projections_total_normalized.mha", tmp_path / "geometry.xml", phantom, order=3, n_average_slices=4,
                             edge_erosion=2, mu_water=0.02, mu_air=0.0, pad=0.0)
    record = yaml.safe_load((tmp_path / "wpc.yaml").read_text())
    assert record["wpc"] == [float(v) for v in fit.coefficients] and record["order"] == 3 and record["slab"] == [4, 4] and record["dimension"] == [40, 12, 40]
    assert record["condition"] == fit.condition and record["rel_diff_after"] == fit.rel_diff_after
    print(f"rel_diff {fit.rel_diff_before:.4f} -> {fit.rel_diff_after:.4f}; residual {fit.residual_identity:.3e} -> {fit.residual_fit:.3e}")
    assert fit.residual_fit <= fit.residual_identity
    assert abs(fit.rel_diff_after) < abs(fit.rel_diff_before)      # the two-energy beam leaves the water 5 % low; the fit sees that region
    weight, template, slab = wp.phantom_weight_and_template(phantom, 4, 2, 0.02, 0.0)
    assert fit.residual_fit == wp.residual(fit.coefficients, fit.basis_mean, weight, template) and slab == (4, 4)


# ---------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
def test_two_calls_give_the_same_bytes(engine, direct, monkeypatch):
    _route(monkeypatch, direct)
    first, second = _call("half_fan", (0, 30), 5), _call("half_fan", (0, 30), 5)
    for x, y in zip(first[:3], second[:3]):
        assert x.tobytes() == y.tobytes()
    assert np.isfinite(first[0]).all() and np.isfinite(first[2]).all() and np.abs(first[2]).max() > 0
