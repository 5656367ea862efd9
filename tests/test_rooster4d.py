"""4-D ROOSTER reconstruction (csrc/rooster4d.hip, reconstruction.rooster4d / reconstruct_4d; the reference's `rtkfourdrooster`
call in cbctmc/reconstruction/reconstruction.py: reconstruct_4d) and the respiratory phase it is sorted by (phase.py).
CPU: peaks and phase against recorded reference outputs, the float64 restatement (rooster_ref.py) against itself, argument handling
and the 4-D MetaImage.  GPU: every operator against the restatement, the adjoint pair, the whole loop, reproducibility, a static
and a moving phantom, the file flow of reconstruct_4d.  Parity against RTK itself is unpinned (RTK is absent here).

Regenerate the phase fixtures from a reference tree:  python tests/test_rooster4d.py <reference tree>"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import joseph_ref as jr
import rooster_ref as rr

pkg = cases.pkg
recon = pkg.reconstruction
phase_mod = pkg.phase
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_phase_cases.npz"


# ---------------------------------------------------------------------------------------------------------------- phase
def _phase_curves():
    """Breathing curves: sin^4 pieces of irregular periods with seeded noise (RespiratorySignal.create_sin4 builds every piece)."""
    sig = pkg.respiratory.RespiratorySignal
    rng = np.random.default_rng(20261016)
    curves = []
    for case in range(5):
        pieces = [sig.create_sin4(total_seconds=float(p), period=float(p), sampling_frequency=15.0).signal for p in rng.uniform(3.0, 6.5, size=6 + case)]
        x = np.concatenate(pieces)
        x = x[int(rng.integers(0, 30)):]  # start anywhere in a cycle
        curves.append(x + rng.normal(scale=0.01 * case, size=x.size))
    return curves


def test_find_peaks_and_phase_equal_the_reference():
    """Peaks exactly, phase within 1e-6 (float32), on the recorded reference outputs."""
    ref = np.load(GOLDEN)
    curves = _phase_curves()
    assert int(ref["n"]) == len(curves)
    for i, x in enumerate(curves):
        np.testing.assert_array_equal(x, ref[f"curve_{i}"])
        np.testing.assert_array_equal(phase_mod.find_peaks(x), ref[f"peaks_{i}"])
        got = phase_mod.calculate_phase(x)
        assert all(p.dtype == np.float32 for p in got)
        assert len(got) == int(ref[f"n_pieces_{i}"])
        np.testing.assert_allclose(np.hstack(got), ref[f"phase_{i}"], rtol=0, atol=1e-6)


def test_edge_peak_rule_is_if_elif():
    """A curve with peaks on both ends: calculate_phase drops the first only; the pieces start at the remaining peaks."""
    t = np.arange(301)
    x = np.cos(2 * np.pi * t / 50.0) ** 2 + 1e-3 * np.sin(t)  # maxima at both ends
    pk = phase_mod.find_peaks(x)
    assert pk[0] == 0 and pk[-1] == len(x) - 1
    pieces = phase_mod.calculate_phase(x)
    assert len(pieces) == len(pk)  # split at len(pk) - 1 peaks
    assert np.hstack(pieces)[-1] == 0.0  # the last sample is a kept peak: phase 0


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_div_is_minus_grad_transpose():
    rng = np.random.default_rng(1)
    u, p = rng.normal(size=(5, 6, 7)), [rng.normal(size=(5, 6, 7)) for _ in range(3)]
    lhs = sum((g * q).sum() for g, q in zip(rr.grad_space(u), p))
    assert lhs == pytest.approx(-(u * rr.div_space(*p)).sum(), rel=1e-12)
    u4, p4 = rng.normal(size=(4, 3, 2, 5)), rng.normal(size=(4, 3, 2, 5))
    assert (rr.grad_time(u4) * p4).sum() == pytest.approx(-(u4 * rr.div_time(p4)).sum(), rel=1e-12)


def test_tv_identity_constant_and_decrease():
    rng = np.random.default_rng(2)
    f = rng.normal(size=(6, 7, 8))
    np.testing.assert_array_equal(rr.tv_space(f, 10, 0.0), f)
    f4 = rng.normal(size=(5, 3, 4, 2))
    np.testing.assert_array_equal(rr.tv_time(f4, 10, 0.0), f4)
    c = np.full((6, 7, 8), 0.7)
    np.testing.assert_allclose(rr.tv_space(c, 10, 0.3), c, rtol=0, atol=1e-15)
    np.testing.assert_allclose(rr.tv_time(np.full((4, 2, 2, 2), 0.7), 10, 0.3), 0.7, rtol=0, atol=1e-15)
    u = rr.tv_space(f, 20, 0.2)
    assert rr.total_variation_space(u) < 0.8 * rr.total_variation_space(f)
    tvt = lambda v: np.abs(rr.grad_time(v)).sum()  # noqa: E731
    assert tvt(rr.tv_time(f4, 20, 0.2)) < 0.8 * tvt(f4)


def test_interpolation_weights():
    N = 10
    phi = np.linspace(0.0, 1.0, 101)
    l, h, wl, wh = rr.weights(phi, N)
    np.testing.assert_allclose(wl + wh, 1.0, rtol=0, atol=1e-15)
    assert ((h - l) % N == 1).all() and (l >= 0).all() and (l < N).all()
    l1, h1, wl1, wh1 = rr.weights([1.0, 0.0, 0.95], N)
    assert (l1[0], wl1[0], wh1[0]) == (0, 1.0, 0.0)  # phi = 1 is frame 0
    assert (l1[1], h1[1]) == (0, 1)
    assert (l1[2], h1[2]) == (9, 0) and wh1[2] == pytest.approx(0.5)  # wraps periodically


def test_restated_cg_solves_a_small_least_squares_system():
    rng = np.random.default_rng(3)
    M = rng.normal(size=(30, 8))
    y = rng.normal(size=30)
    A = lambda v: M.T @ (M @ v)  # noqa: E731
    res = []
    x = rr.cg(A, M.T @ y, np.zeros(8), 8, res)
    np.testing.assert_allclose(x, np.linalg.lstsq(M, y, rcond=None)[0], rtol=1e-8, atol=1e-10)
    assert res[-1] < 1e-8 * res[0]


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_reconstruct_4d_needs_exactly_one_signal(tmp_path):
    with pytest.raises(ValueError):
        recon.reconstruct_4d(tmp_path / "p.mha", tmp_path / "g.xml", amplitude_signal=np.ones(4), phase_signal=np.ones(4))
    with pytest.raises(ValueError):
        recon.reconstruct_4d(tmp_path / "p.mha", tmp_path / "g.xml")


def _options(**over):
    geo = recon.create_geometry(4, start_angle=0.0, detector_offset_x=0.0)
    lib, o, keep = recon._rooster_call(4, 8, 6, geo, (2.0, 2.0), None, np.zeros(4), (4, 5, 6), (1.0, 1.0, 1.0), None, 2, 1, 1, 1, 0.0, 0.0,
                                       None, True, 0)
    for k, v in over.items():
        setattr(o, k, v)
    return lib, o, keep


@pytest.mark.parametrize("field, value, text", [("struct_size", 0, "struct_size"), ("n_frames", 0, "n_frames"), ("n_frames", 33, "n_frames"),
                                                ("nu", 1, "geometry"), ("sx", 0.0, "volume"), ("tviter", -1, "tviter")])
def test_bad_options_are_refused_before_any_hip_call(engine, field, value, text):
    lib, o, keep = _options(**{field: value})
    lib.mcgpu_last_error.restype = C.c_char_p
    buf = np.zeros(1 << 12, np.float32)
    assert lib.mcgpu_rooster4d_reconstruct(C.byref(o), buf.ctypes.data, buf.ctypes.data, None) == -1
    assert text in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_rooster4d_stage(C.byref(o), 0, buf.ctypes.data, buf.ctypes.data, None) == -1


def test_phase_outside_unit_interval_and_unknown_stage_are_refused(engine):
    lib, o, keep = _options()
    keep["phase"][2] = 1.5
    buf = np.zeros(1 << 12, np.float32)
    assert lib.mcgpu_rooster4d_reconstruct(C.byref(o), buf.ctypes.data, buf.ctypes.data, None) == -1
    assert "phase[2]" in lib.mcgpu_last_error().decode()
    keep["phase"][2] = 0.5
    assert lib.mcgpu_rooster4d_stage(C.byref(o), 7, buf.ctypes.data, buf.ctypes.data, None) == -1
    assert "unknown stage" in lib.mcgpu_last_error().decode()


def test_mha_4d_round_trip_and_header(tmp_path):
    v = np.random.default_rng(4).normal(size=(3, 4, 5, 6)).astype(np.float32)
    p = recon.write_mha(tmp_path / "v.mha", v, (1.5, 2.0, 2.5, 1.0), (-3.0, -4.0, -5.0, 0.0))
    head = p.read_bytes().split(b"ElementDataFile")[0].decode()
    assert "NDims = 4" in head and "DimSize = 6 5 4 3" in head
    assert "ElementSpacing = 1.5 2 2.5 1" in head and "Offset = -3 -4 -5 0" in head
    got, sp, org = recon.read_mha(p)
    np.testing.assert_array_equal(got, v)
    assert sp == [1.5, 2.0, 2.5, 1.0] and org == [-3.0, -4.0, -5.0, 0.0]
    v3 = v[0]
    got3, sp3, _ = recon.read_mha(recon.write_mha(tmp_path / "v3.mha", v3, (1, 2, 3), (0, 0, 0)))
    np.testing.assert_array_equal(got3, v3)
    assert b"NDims = 3" in (tmp_path / "v3.mha").read_bytes()[:200]


# ---------------------------------------------------------------------------------------------------------------- GPU
# small problem: 24 x 16 x 20 voxels of 2 mm, 3 frames, 12 projections of 32 x 24 pixels (3.5 mm), sid 300, sdd 500
DIM, SPACING, FRAMES, NU, NV, PIX = (24, 16, 20), (2.0, 2.0, 2.0), 3, 32, 24, 3.5
SID, SDD = 300.0, 500.0


def _geometry(n=12, offset=0.0):
    g = recon.CircularGeometry(SID, SDD)
    for k in range(n):
        g.add_projection(17.0 + k * 360.0 / n, offset, 0.0)
    return g


def _phase(n=12):
    ph = np.mod(0.13 + 0.29 * np.arange(n), 1.0)
    ph[0], ph[1], ph[2] = 0.0, 1.0, 0.5  # the ends of the range and a pair of neighbours that share a frame pair
    ph[3] = 0.55
    return ph


def _ref_geometry(geo, phase):
    return rr.Geometry(geo.gantry_angles, SID, SDD, NU, NV, PIX, PIX, DIM, SPACING, phase, FRAMES, geo.projection_offsets_x, geo.projection_offsets_y)


def _smooth4(seed=5):
    """A smooth positive 4-D field (frames differ)."""
    nx, ny, nz = DIM
    z, y, x = np.meshgrid(np.linspace(-1, 1, nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    rng = np.random.default_rng(seed)
    out = []
    for f in range(FRAMES):
        a = rng.uniform(0.5, 1.5, size=4)
        out.append(a[0] * np.exp(-((x - 0.3 * a[1] + 0.3) ** 2 + (y * a[2]) ** 2 + (z - 0.2 * a[3]) ** 2) / 0.3) + 0.2 * np.cos(2 * x + z))
    return np.stack(out)


def _stage(stage, data, geo, phase, **kw):
    return recon.rooster4d_stage(stage, data, geo, (NU, NV), (PIX, PIX), None, phase, DIM, SPACING, frames=FRAMES, **kw)[0]


def _rel(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


@pytest.mark.gpu
def test_forward_stage_equals_the_restatement(engine):
    geo, ph = _geometry(), _phase()
    x = _smooth4()
    ref = rr.forward(_ref_geometry(geo, ph), x)
    got = _stage("forward", x, geo, ph)
    amb = jr.ambiguous_main_axis(geo.gantry_angles, geo.projection_offsets_x, geo.projection_offsets_y, SID, SDD, NU, NV, PIX, PIX,
                                 -(NU - 1) / 2 * PIX, -(NV - 1) / 2 * PIX, SPACING)
    assert _rel(np.where(amb, 0, got), np.where(amb, 0, ref)) <= 1e-5


@pytest.mark.gpu
def test_back_stage_equals_the_restatement(engine):
    geo, ph = _geometry(), _phase()
    q = rr.forward(_ref_geometry(geo, ph), _smooth4())  # smooth projections
    ref = rr.back(_ref_geometry(geo, ph), q)
    got = _stage("back", q, geo, ph)
    assert _rel(got, ref) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("stage, gamma", [("tv_space", 0.05), ("tv_time", 0.05)])
def test_tv_stages_equal_the_restatement(engine, stage, gamma):
    geo, ph = _geometry(), _phase()
    x = _smooth4() + np.random.default_rng(6).normal(scale=0.1, size=(FRAMES,) + DIM[::-1])
    if stage == "tv_space":
        ref = np.stack([rr.tv_space(x[f], 7, gamma) for f in range(FRAMES)])
        got = _stage(stage, x, geo, ph, tviter=7, gamma_space=gamma)
    else:
        ref = rr.tv_time(x, 7, gamma)
        got = _stage(stage, x, geo, ph, tviter=7, gamma_time=gamma)
    assert _rel(got, ref) <= 1e-5
    assert _rel(got, x) > 1e-3  # it did something


@pytest.mark.gpu
def test_forward_and_back_are_close_to_an_adjoint_pair(engine):
    """<R S x, y> vs <x, S^T B y> on smooth fields.  B is only approximately R^T (voxel-driven bilinear gather vs ray-driven
    Joseph); the float64 restatement gives a relative gap of a few per cent here (printed), the kernels must give the same gap
    within 1e-4 and stay below 10 %."""
    geo, ph = _geometry(), _phase()
    g = _ref_geometry(geo, ph)
    x = _smooth4(7)
    y = rr.forward(g, _smooth4(8))
    ref_gap = (rr.forward(g, x) * y).sum() / (x * rr.back(g, y)).sum() - 1.0
    gap = (_stage("forward", x, geo, ph).astype(np.float64) * y).sum() / (x * _stage("back", y, geo, ph).astype(np.float64)).sum() - 1.0
    print(f"adjoint gap: restatement {ref_gap:.4e}, kernels {gap:.4e}")
    assert abs(ref_gap) < 0.1
    assert abs(gap - ref_gap) < 1e-4


def _projections(geo, ph, seed=9):
    return rr.forward(_ref_geometry(geo, ph), _smooth4(seed)).astype(np.float32)


@pytest.mark.gpu
def test_rooster4d_equals_the_restated_loop_and_repeats_bit_for_bit(engine):
    """niter 2, cgiter 3, tviter 5 against rooster_ref.rooster: 1e-3 relative (float32 CG against float64 CG).  A second run is
    bit-identical; the residual falls over every main iteration (|r| of CG need not fall at every step)."""
    geo, ph = _geometry(), _phase()
    p = _projections(geo, ph)
    kw = dict(frames=FRAMES, niter=2, cgiter=3, tviter=5, gamma_space=0.002, gamma_time=0.002)
    vol, rep = recon.rooster4d(p, geo, (PIX, PIX), None, ph, DIM, SPACING, **kw)
    res_ref = []
    ref = rr.rooster(_ref_geometry(geo, ph), p.astype(np.float64), 2, 3, 5, 0.002, 0.002, True, res_ref)
    assert _rel(vol, ref) <= 1e-3
    np.testing.assert_allclose(rep["residuals"].ravel(), res_ref, rtol=1e-3)
    vol2, rep2 = recon.rooster4d(p, geo, (PIX, PIX), None, ph, DIM, SPACING, **kw)
    assert vol.tobytes() == vol2.tobytes()
    assert rep["residuals"].tobytes() == rep2["residuals"].tobytes()
    for row in rep["residuals"]:  # |r| of CG is not monotone step by step; over a main iteration it falls
        assert row[-1] < row[0], row
    assert rep["peak_device_bytes"] > 0 and rep["ms_forward"] > 0 and rep["ms_back"] > 0


@pytest.mark.gpu
def test_static_phantom_gives_equal_frames(engine):
    """A phantom that does not move: the frames agree inside the volume (3 voxels in from every face; the corners are reached by few
    projections and differ per frame).  Measured on the float64 restatement: inter-frame spread 0.85 % RMS of the phantom, error
    against the phantom 2.8 %; asserted: spread <= 2 % and below half the error."""
    n = 48
    geo = _geometry(n)
    ph = np.mod(0.37 * np.arange(n), 1.0)
    g = rr.Geometry(geo.gantry_angles, SID, SDD, NU, NV, PIX, PIX, DIM, SPACING, ph, FRAMES)
    x = np.repeat(_smooth4(10)[:1], FRAMES, axis=0)
    p = rr.forward(g, x).astype(np.float32)
    vol, _ = recon.rooster4d(p, geo, (PIX, PIX), None, ph, DIM, SPACING, frames=FRAMES, niter=3, cgiter=3, tviter=5)
    c = (slice(None), slice(3, -3), slice(3, -3), slice(3, -3))
    scale = np.sqrt((x[c] ** 2).mean())
    spread = np.sqrt(((vol - vol.mean(axis=0))[c] ** 2).mean()) / scale
    err = np.sqrt(((vol - x)[c] ** 2).mean()) / scale
    print(f"static phantom: spread {spread:.4f}, error {err:.4f}")
    assert spread <= 0.02 and spread <= 0.5 * err, (spread, err)


def _sphere(center_z, radius=7.0):
    nx, ny, nz = DIM
    X = (np.arange(nx) - (nx - 1) / 2) * SPACING[0]
    Y = (np.arange(ny) - (ny - 1) / 2) * SPACING[1]
    Z = (np.arange(nz) - (nz - 1) / 2) * SPACING[2]
    z, y, x = np.meshgrid(Z, Y, X, indexing="ij")
    # 4^3 sub-samples per voxel: a partial-volume sphere (its centroid is the true centre)
    s = np.zeros(z.shape)
    for o in (np.arange(4) + 0.5) / 4 - 0.5:
        for q in (np.arange(4) + 0.5) / 4 - 0.5:
            for r in (np.arange(4) + 0.5) / 4 - 0.5:
                s += (((x + o * SPACING[0]) ** 2 + (y + q * SPACING[1]) ** 2 + (z + r * SPACING[2] - center_z) ** 2) <= radius ** 2)
    return s / 64.0


@pytest.mark.gpu
def test_moving_sphere_is_found_in_every_frame_and_beats_fdk(engine):
    """A sphere moves along z with the phase (3 states, the scan sees each in a third of its 72 projections).  Each frame's
    centroid lies within one voxel of that state's centre, and the per-frame RMS error is at least 2x below fdk() of all
    projections (which averages the motion)."""
    n = 72
    geo = _geometry(n)
    ph = np.array([(k % 3) / 3.0 for k in range(n)])
    centers = [-6.0, 0.0, 6.0]
    truth = np.stack([_sphere(c) for c in centers])
    p = np.zeros((n, NV, NU), np.float32)
    for k in range(n):
        p[k] = jr.project(truth[k % 3], SPACING, -(np.array(DIM) - 1) / 2 * SPACING, [geo.gantry_angles[k]], [0.0], [0.0], SID, SDD, NU, NV, PIX, PIX,
                          -(NU - 1) / 2 * PIX, -(NV - 1) / 2 * PIX)[0]
    vol, _ = recon.rooster4d(p, geo, (PIX, PIX), None, ph, DIM, SPACING, frames=3, niter=4, cgiter=4, tviter=10)
    fdk, _ = recon.fdk(p, geo, (PIX, PIX), None, DIM, SPACING)
    Z = (np.arange(DIM[2]) - (DIM[2] - 1) / 2) * SPACING[2]
    for f, c in enumerate(centers):
        w = np.clip(vol[f], 0, None)
        cz = (w.sum(axis=(1, 2)) * Z).sum() / w.sum()
        assert abs(cz - c) <= SPACING[2], (f, cz, c)
        rms = np.sqrt(((vol[f] - truth[f]) ** 2).mean())
        rms_fdk = np.sqrt(((fdk - truth[f]) ** 2).mean())
        print(f"frame {f}: centroid z {cz:+.2f} mm (true {c:+.1f}), rms {rms:.4f}, fdk rms {rms_fdk:.4f}")
        assert 2 * rms <= rms_fdk, (f, rms, rms_fdk)


@pytest.mark.gpu
def test_reconstruct_4d_file_flow(engine, tmp_path):
    """An .mha projection stack, geometry.xml from create_geometry and an amplitude signal -> recon_rooster4d.mha (4-D) + .yaml."""
    import yaml
    n = 60
    geo = recon.create_geometry(n, start_angle=90.0, source_to_isocenter=SID, source_to_detector=SDD, detector_offset_x=0.0)
    gpath = recon.save_geometry(geo, tmp_path / "geometry.xml")
    amp = pkg.respiratory.RespiratorySignal.create_sin4(total_seconds=n / 5.0, period=3.0, sampling_frequency=5.0).signal
    ph = np.hstack(phase_mod.calculate_phase(amp)).astype(np.float64)
    ph = (ph - ph.min()) / (ph.max() - ph.min())
    g = rr.Geometry(geo.gantry_angles, SID, SDD, NU, NV, PIX, PIX, DIM, SPACING, ph, FRAMES)
    p = rr.forward(g, _smooth4(11)).astype(np.float32)
    ppath = recon.write_mha(tmp_path / "projections_total_normalized.mha", p, (PIX, PIX, 1.0), (-(NU - 1) / 2 * PIX, -(NV - 1) / 2 * PIX, 0.0))
    out, rep = recon.reconstruct_4d(ppath, gpath, dimension=DIM, spacing=SPACING, amplitude_signal=amp, frames=FRAMES, niter=1, cgiter=2, tviter=2)
    assert out == tmp_path / "reconstructions" / "recon_rooster4d.mha"
    vol, sp, org = recon.read_mha(out)
    assert vol.shape == (FRAMES,) + DIM[::-1]
    assert sp == [2.0, 2.0, 2.0, 1.0]
    assert org == [-(d - 1) / 2 * s for d, s in zip(DIM, SPACING)] + [0.0]
    assert np.isfinite(vol).all() and vol.max() > 0
    params = yaml.safe_load(out.with_suffix(".yaml").read_text())
    for key in ("niter", "cgiter", "tviter", "gamma_time", "gamma_space", "dimension", "spacing", "wpc", "geometry", "path", "regexp", "output_filepath"):
        assert key in params, key
    assert params["fp"] == "Joseph" and params["bp"] == "VoxelBased" and params["cgiter"] == 2
    direct, _ = recon.rooster4d(p, geo, (PIX, PIX), (-(NU - 1) / 2 * PIX, -(NV - 1) / 2 * PIX), ph, DIM, SPACING, frames=FRAMES, niter=1, cgiter=2, tviter=2)
    assert vol.tobytes() == direct.tobytes()


if __name__ == "__main__":  # regenerate the fixtures: python tests/test_rooster4d.py <reference tree>
    sys.path.insert(0, str(Path(sys.argv[1]).resolve()))
    from cbctmc.peaks import find_peaks as ref_find_peaks  # noqa: E402
    from cbctmc.reconstruction.respiratory import calculate_phase as ref_calculate_phase  # noqa: E402
    out = {}
    curves = _phase_curves()
    out["n"] = np.array(len(curves))
    for i, x in enumerate(curves):
        pieces = ref_calculate_phase(x.copy())
        out[f"curve_{i}"] = x
        out[f"peaks_{i}"] = np.asarray(ref_find_peaks(x.copy()))
        out[f"phase_{i}"] = np.hstack(pieces).astype(np.float32)
        out[f"n_pieces_{i}"] = np.array(len(pieces))
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, GOLDEN.stat().st_size, "bytes")
