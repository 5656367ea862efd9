"""4-D ROOSTER (csrc/rooster4d.hip) at the launch shapes and branches the reference's settings take, against the float64
restatement (rooster_ref.py).  test_rooster4d.py pins every operator on one small centred configuration; the configurations here
reach what that one does not:
  half_fan     N = 10, 37 projections (forward batches 16 + 16 + 5), a displaced detector (offset_x = -0.4026 nu du, the
               reference's half-fan ratio, so the detector's inner edge cuts the volume), a small per-projection offset_y, and the
               pixel origin -n d / 2 of the stacks written by this project (not the default -(n - 1) d / 2)
  sorted_runs  N = 2, one run of 17 projections of one frame pair (back-projection batches 8 + 8 + 1) and runs of 1
  odd          N = 1 (frames l == h), 23 x 17 x 19 voxels (4-D size not a multiple of 4) at an explicit off-centre origin
  wide         300 voxels in x (two bp4 x-blocks), N = 16 (tv_time_kernel<16> at full use)
  many17/32    the tv_time_kernel<32> instantiation
and the whole loop with water pre-correction and with and without positivity, the zero-input guards of CG, no iterations, the
grid-stride loop of tv_space on a frame of more than 65536 x 256 voxels and the pixel origin reconstruct_4d reads from the stack.
CPU: the ctypes mirrors of the C ABI against the layout the C compiler gives include/mcgpu_amd.h."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import abi_layout
import cases
import joseph_ref as jr
import rooster_ref as rr

pkg = cases.pkg
recon = pkg.reconstruction
phase_mod = pkg.phase

SID, SDD, PIX = 300.0, 500.0, 3.5
HALF_FAN = 0.4026  # detector offset over detector width of the reference's half-fan scan (create_geometry's default)
GAMMA_SPACE, GAMMA_TIME = 0.00007, 0.0002  # reconstruct_4d's (the reference's) defaults
WPC = (0.0, 1.05, 0.01)


class Config:
    """One problem: geometry (CircularGeometry and its restatement), phase, grid; stage() runs one kernel operator on it."""

    def __init__(self, name, dim, frames, phase, spacing=(2.0, 2.0, 2.0), nu=32, nv=24, half_fan=False, origin=None):
        self.name, self.dim, self.frames, self.spacing, self.nu, self.nv, self.origin = name, tuple(dim), frames, tuple(spacing), nu, nv, origin
        self.phase = np.asarray(phase, dtype=np.float64)
        n = self.phase.size
        self.geo = recon.CircularGeometry(SID, SDD)
        for k in range(n):
            self.geo.add_projection(17.0 + k * 360.0 / n, -HALF_FAN * nu * PIX if half_fan else 0.0, 0.6 * np.sin(0.7 * k) if half_fan else 0.0)
        self.pixel_origin = (-nu * PIX / 2, -nv * PIX / 2) if half_fan else None
        self.u0, self.v0 = self.pixel_origin or (-(nu - 1) / 2 * PIX, -(nv - 1) / 2 * PIX)
        self.ref = rr.Geometry(self.geo.gantry_angles, SID, SDD, nu, nv, PIX, PIX, self.dim, self.spacing, self.phase, frames,
                               self.geo.projection_offsets_x, self.geo.projection_offsets_y, self.u0, self.v0, origin)

    def stage(self, stage, data, **kw):
        return recon.rooster4d_stage(stage, data, self.geo, (self.nu, self.nv), (PIX, PIX), self.pixel_origin, self.phase, self.dim, self.spacing,
                                     self.origin, frames=self.frames, **kw)[0]

    def rooster4d(self, projections, **kw):
        return recon.rooster4d(projections, self.geo, (PIX, PIX), self.pixel_origin, self.phase, self.dim, self.spacing, self.origin,
                               frames=self.frames, **kw)

    def field(self, seed):
        """A smooth positive 4-D field whose frames differ."""
        nx, ny, nz = self.dim
        z, y, x = np.meshgrid(np.linspace(-1, 1, nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(self.frames):
            a = rng.uniform(0.5, 1.5, size=4)
            out.append(a[0] * np.exp(-((x - 0.3 * a[1] + 0.3) ** 2 + (y * a[2]) ** 2 + (z - 0.2 * a[3]) ** 2) / 0.3) + 0.2 * np.cos(2 * x + z))
        return np.stack(out)


def _spread(n, step=0.29):
    ph = np.mod(0.13 + step * np.arange(n), 1.0)
    ph[0], ph[1] = 0.0, 1.0  # both ends of the range
    return ph


def _sorted_runs():
    """N = 2: 17 projections between frames 0 and 1 (one frame pair: back-projection batches 8 + 8 + 1), then alternating pairs
    (1, 0) and (0, 1) (batches of 1)."""
    return np.concatenate([0.05 + 0.4 * np.arange(17) / 16, [0.6, 0.2, 0.7, 0.3, 0.8]])


@lru_cache(maxsize=None)
def config(name):
    if name == "half_fan":
        return Config(name, (24, 16, 20), 10, _spread(37), half_fan=True)
    if name == "sorted_runs":
        return Config(name, (24, 16, 20), 2, _sorted_runs())
    if name == "odd":
        return Config(name, (23, 17, 19), 1, _spread(12), origin=(-19.0, -17.5, -16.0))
    if name == "wide":
        return Config(name, (300, 6, 8), 16, _spread(12, 0.41), spacing=(0.25, 2.0, 2.0), nu=48, nv=16)
    if name in ("many17", "many32"):
        return Config(name, (12, 10, 8), int(name[4:]), _spread(16, 0.37))
    raise KeyError(name)


CONFIGS = ["half_fan", "sorted_runs", "odd", "wide", "many17", "many32"]


def _rel(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_configurations_reach_the_launch_shapes():
    """What each configuration is for, restated from the kernel's launch rules (rooster4d.hip: kFpBatch 16, kBpBatch 8, bp4 x-blocks
    of 256, tv_time_kernel<16> for N <= 16)."""
    def bp_batches(g):
        sizes, k = [], 0
        while k < len(g.angles):
            m = 0
            while k + m < len(g.angles) and m < 8 and g.l[k + m] == g.l[k] and g.h[k + m] == g.h[k]:
                m += 1
            sizes.append(m)
            k += m
        return sizes
    hf, sr, odd, wide = config("half_fan"), config("sorted_runs"), config("odd"), config("wide")
    assert len(hf.phase) == 37 and hf.frames == 10 and hf.u0 == -hf.nu * PIX / 2 and hf.v0 == -hf.nv * PIX / 2
    # the detector's inner edge (last column, rotated frame, scaled to the isocentre) lies inside the volume's x extent
    edge = (hf.u0 + (hf.nu - 1) * PIX + hf.geo.projection_offsets_x[0]) * SID / SDD
    assert 0 < edge < hf.dim[0] * hf.spacing[0] / 2
    assert bp_batches(sr.ref) == [8, 8, 1, 1, 1, 1, 1, 1]
    assert (odd.ref.l == odd.ref.h).all() and np.prod(odd.dim) % 4 != 0
    assert (wide.dim[0] + 255) // 256 == 2 and wide.frames == 16
    assert config("many17").frames == 17 and config("many32").frames == 32


def test_restated_water_precorrection():
    p = np.array([0.0, 0.5, 2.0, 13.0])
    np.testing.assert_array_equal(rr.water_precorrection(p, WPC), 1.05 * p + 0.01 * p * p)
    np.testing.assert_array_equal(rr.water_precorrection(p, (0.0, 1.0)), p)


def _mirrors():
    return [("mcgpu_scan_options", pkg.engine.ScanOptions), ("mcgpu_scan_report", pkg.engine.ScanReport),
            ("mcgpu_fdk_options", recon._FdkOptions), ("mcgpu_fdk_report", recon._FdkReport),
            ("mcgpu_fp_options", pkg.forward_projection._FpOptions), ("mcgpu_fp_report", pkg.forward_projection._FpReport),
            ("mcgpu_rooster4d_options", recon._RoosterOptions), ("mcgpu_rooster4d_report", recon._RoosterReport)]


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """Every struct Python hands to or reads from the C ABI: the header's field names in order, and sizeof plus each field's
    offsetof and size as the C compiler lays them out, equal the ctypes mirror's (tests/abi_layout.py).  A swap of two fields of one
    type (ox / oy, wpc / residuals) keeps the size and is caught only by the names."""
    mirrors = _mirrors()
    abi_layout.assert_field_names(mirrors)
    cc = abi_layout.c_compiler()
    if cc is None:
        pytest.skip("no C compiler")
    c_side = abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    assert c_side["mcgpu_rooster4d_options"] == "232"


# ---------------------------------------------------------------------------------------------------------------- GPU operators
def _fv_edge(cfg, tol=1e-4):
    """[nz][ny][nx] voxels whose float64 detector row fv lies within `tol` pixel of the inclusion limits 0 and nv - 1 for some
    projection: bp4 computes fv in float32 (rooster4d.hip: av_a Y + av_b), so there the kernel and the restatement may legitimately
    disagree about whether the sample counts."""
    g = cfg.ref
    nx, ny, nz = g.dim
    zz, yy, xx = np.meshgrid(g.org[2] + g.sp[2] * np.arange(nz), g.org[1] + g.sp[1] * np.arange(ny), g.org[0] + g.sp[0] * np.arange(nx), indexing="ij")
    out = np.zeros(xx.shape, dtype=bool)
    for k, a in enumerate(g.angles):
        t = np.deg2rad(a)
        mag = g.sdd / (g.sid - (xx * np.sin(t) + zz * np.cos(t)))
        fv = (mag * yy - g.offy[k] - g.v0) / g.dv
        out |= (np.abs(fv) < tol) | (np.abs(fv - (g.nv - 1)) < tol)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_forward_stage_equals_the_restatement(engine, name):
    cfg = config(name)
    x = cfg.field(5)
    ref = rr.forward(cfg.ref, x)
    got = cfg.stage("forward", x)
    amb = jr.ambiguous_main_axis(cfg.geo.gantry_angles, cfg.geo.projection_offsets_x, cfg.geo.projection_offsets_y, SID, SDD, cfg.nu, cfg.nv,
                                 PIX, PIX, cfg.u0, cfg.v0, cfg.spacing)
    assert _rel(np.where(amb, 0, got), np.where(amb, 0, ref)) <= 1e-5
    for k in range(len(cfg.phase)):  # every projection, in every forward batch, saw the volume
        assert np.abs(got[k]).max() > 0.1 * np.abs(ref[k]).max() > 0, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_back_stage_equals_the_restatement(engine, name):
    cfg = config(name)
    q = rr.forward(cfg.ref, cfg.field(6)).astype(np.float32)  # smooth projections
    ref = rr.back(cfg.ref, q.astype(np.float64))
    got = cfg.stage("back", q)
    edge = _fv_edge(cfg)
    print(f"{name}: {int(edge.sum())} of {edge.size} voxels within 1e-4 pixel of a row limit")
    assert edge.mean() < 0.01
    assert _rel(np.where(edge, 0, got), np.where(edge, 0, ref)) <= 1e-5
    for f in range(cfg.frames):  # every frame that a projection touches
        if (cfg.ref.wl[cfg.ref.l == f] > 0).any() or (cfg.ref.wh[cfg.ref.h == f] > 0).any():
            assert _rel(np.where(edge, 0, got[f]), np.where(edge, 0, ref[f])) <= 1e-5, f


def _noisy(cfg, seed):
    return cfg.field(seed) + np.random.default_rng(seed).normal(scale=0.1, size=(cfg.frames,) + cfg.dim[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_tv_space_stage_equals_the_restatement(engine, name):
    cfg = config(name)
    x = _noisy(cfg, 11).astype(np.float32).astype(np.float64)
    ref = np.stack([rr.tv_space(x[f], 7, 0.05) for f in range(cfg.frames)])
    got = cfg.stage("tv_space", x, tviter=7, gamma_space=0.05)
    assert _rel(got, ref) <= 1e-5
    assert _rel(got, x) > 1e-3  # it did something


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_tv_time_stage_equals_the_restatement(engine, name):
    cfg = config(name)
    x32 = _noisy(cfg, 12).astype(np.float32)
    x = x32.astype(np.float64)
    ref = rr.tv_time(x, 7, 0.05)
    got = cfg.stage("tv_time", x32, tviter=7, gamma_time=0.05)
    if cfg.frames == 1:  # one frame is its own neighbour: temporal TV is the identity
        np.testing.assert_array_equal(ref, x)
        assert got.tobytes() == x32.tobytes()
        return
    assert _rel(got, ref) <= 1e-5
    assert _rel(got, x) > 1e-3
    assert _rel(got[-1], ref[-1]) <= 1e-5  # the last frame (the periodic neighbour of frame 0)


@pytest.mark.gpu
def test_adjoint_gap_at_half_fan(engine):
    """<R S x, y> / <x, S^T B y> - 1 of the kernels equals the restatement's within 1e-4 on the half-fan detector."""
    cfg = config("half_fan")
    x = cfg.field(7)
    y = rr.forward(cfg.ref, cfg.field(8)).astype(np.float32).astype(np.float64)
    ref_gap = (rr.forward(cfg.ref, x) * y).sum() / (x * rr.back(cfg.ref, y)).sum() - 1.0
    gap = (cfg.stage("forward", x).astype(np.float64) * y).sum() / (x * cfg.stage("back", y).astype(np.float64)).sum() - 1.0
    print(f"half-fan adjoint gap: restatement {ref_gap:.4e}, kernels {gap:.4e}")
    assert abs(ref_gap) < 0.1
    assert abs(gap - ref_gap) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["odd", "many17"])
def test_tv_with_gamma_zero_is_the_identity(engine, name):
    """gamma = 0 projects the dual onto {0}: both TV stages return their input bit for bit (N = 1 and N = 17)."""
    cfg = config(name)
    x = np.random.default_rng(13).normal(size=(cfg.frames,) + cfg.dim[::-1]).astype(np.float32)
    assert cfg.stage("tv_space", x, tviter=5, gamma_space=0.0).tobytes() == x.tobytes()
    assert cfg.stage("tv_time", x, tviter=5, gamma_time=0.0).tobytes() == x.tobytes()


@pytest.mark.gpu
def test_tv_space_on_a_frame_beyond_one_grid(engine):
    """256 x 256 x 257 voxels = 16,842,752 > 65536 blocks x 256 threads: the voxels past 65536 x 256 are reached only by the grid-stride
    loop of tv_space_div / tv_space_grad.  One frame, two iterations (the float64 side holds about 2 GB for a few seconds)."""
    dim = (256, 256, 257)
    cfg = Config("large", dim, 1, [0.0], spacing=(1.0, 1.0, 1.0))
    x = np.random.default_rng(14).normal(scale=0.1, size=(1,) + dim[::-1]).astype(np.float32)
    got = cfg.stage("tv_space", x, tviter=2, gamma_space=0.05)
    ref = rr.tv_space(x[0].astype(np.float64), 2, 0.05)
    assert _rel(got[0], ref) <= 1e-5
    tail = 65536 * 256
    g, r, x0 = got.ravel()[tail:], ref.ravel()[tail:], x.ravel()[tail:]
    assert (g != x0).mean() > 0.9  # the grid-stride share changed ...
    assert _rel(g, r) <= 1e-5      # ... as the restatement did


# ---------------------------------------------------------------------------------------------------------------- GPU whole loop
def _moving_sphere(cfg, radius=7.0):
    """Partial-volume sphere (4^3 sub-samples per voxel) whose centre moves along z with the frame: sharp edges, so the
    unconstrained least-squares solution has negative lobes."""
    nx, ny, nz = cfg.dim
    X, Y, Z = ((np.arange(n) - (n - 1) / 2) * s for n, s in zip(cfg.dim, cfg.spacing))
    z, y, x = np.meshgrid(Z, Y, X, indexing="ij")
    sub = (np.arange(4) + 0.5) / 4 - 0.5
    out = np.zeros((cfg.frames, nz, ny, nx))
    for f in range(cfg.frames):
        cz = 5.0 * np.sin(2 * np.pi * f / cfg.frames)
        for o in sub:
            for q in sub:
                for r in sub:
                    out[f] += ((x + o * cfg.spacing[0]) ** 2 + (y + q * cfg.spacing[1]) ** 2 + (z + r * cfg.spacing[2] - cz) ** 2) <= radius ** 2
    return out / 64.0


@lru_cache(maxsize=None)
def _breathing_scan():
    """The half-fan geometry with 60 projections whose phase comes from a breathing curve as reconstruct_4d derives it
    (RespiratorySignal.create_sin4 -> phase.calculate_phase -> min-max scaling), and an off-centre volume."""
    amp = pkg.respiratory.RespiratorySignal.create_sin4(total_seconds=12.0, period=3.0, sampling_frequency=5.0).signal
    ph = np.hstack(phase_mod.calculate_phase(amp)).astype(np.float64)
    ph = (ph - ph.min()) / (ph.max() - ph.min())
    assert ph.size == 60
    cfg = Config("breathing", (24, 16, 20), 10, ph, half_fan=True, origin=(-21.0, -16.5, -17.0))
    p = rr.forward(cfg.ref, _moving_sphere(cfg)).astype(np.float32)
    return cfg, p


@pytest.mark.gpu
@pytest.mark.parametrize("positivity", [True, False])
def test_rooster4d_at_the_reference_settings_equals_the_restatement(engine, positivity):
    """niter 2, cgiter 3, tviter 5 with the reference's gammas, wpc (0, 1.05, 0.01), half-fan, N = 10: 1e-3 relative against
    rooster_ref.rooster (float32 CG against float64 CG), residuals at rtol 1e-3.  Without positivity the result has negative
    values, which shows that the branch ran."""
    cfg, p = _breathing_scan()
    kw = dict(niter=2, cgiter=3, tviter=5, gamma_space=GAMMA_SPACE, gamma_time=GAMMA_TIME, water_pre_correction=WPC, positivity=positivity)
    vol, rep = cfg.rooster4d(p, **kw)
    res_ref = []
    ref = rr.rooster(cfg.ref, p.astype(np.float64), 2, 3, 5, GAMMA_SPACE, GAMMA_TIME, positivity, res_ref, wpc=WPC)
    print(f"positivity {positivity}: rel {_rel(vol, ref):.2e}, min {vol.min():.4f} (restatement {ref.min():.4f})")
    assert _rel(vol, ref) <= 1e-3
    np.testing.assert_allclose(rep["residuals"].ravel(), res_ref, rtol=1e-3)
    if positivity:
        assert vol.min() >= 0.0
    else:
        assert vol.min() < 0.0 and ref.min() < 0.0


@pytest.mark.gpu
def test_rooster4d_at_odd_sizes_equals_the_restatement(engine):
    """The whole loop on the `odd` configuration: N = 1 and 23 x 17 x 19 voxels, so the last float4 group of every CG vector holds
    one voxel and three floats of padding that the dot products and updates must leave at zero; off-centre volume.  Without
    positivity, so that the last voxel (a corner, reached by few rays) is not clamped to 0 and shows whether its group was updated."""
    cfg = config("odd")
    p = rr.forward(cfg.ref, cfg.field(17)).astype(np.float32)
    vol, rep = cfg.rooster4d(p, niter=2, cgiter=3, tviter=5, gamma_space=0.002, gamma_time=0.002, positivity=False)
    res_ref = []
    ref = rr.rooster(cfg.ref, p.astype(np.float64), 2, 3, 5, 0.002, 0.002, False, res_ref)
    assert _rel(vol, ref) <= 1e-3
    np.testing.assert_allclose(rep["residuals"].ravel(), res_ref, rtol=1e-3)
    last, scale = ref.ravel()[-1], np.abs(ref).max()
    assert abs(last) > 0.05 * scale
    assert abs(float(vol.ravel()[-1]) - last) <= 1e-3 * scale  # the voxel of the last, padded group


@pytest.mark.gpu
def test_zero_projections_give_an_exact_zero_volume(engine):
    """All-zero projections: b = 0, so |r| = 0 and the guards rr > 0 / dAd > 0 skip every CG step: the volume is exactly 0, the
    residuals are exactly 0 and the report is finite."""
    cfg = config("half_fan")
    p = np.zeros((len(cfg.phase), cfg.nv, cfg.nu), np.float32)
    vol, rep = cfg.rooster4d(p, niter=2, cgiter=2, tviter=3, water_pre_correction=WPC)
    assert (vol == 0.0).all()
    assert rep["residuals"].shape == (2, 3) and (rep["residuals"] == 0.0).all()
    for key, value in rep.items():
        assert np.isfinite(value).all(), key


@pytest.mark.gpu
def test_no_iterations_give_an_exact_zero_volume(engine):
    """niter = 0: nothing runs.  cgiter = 0: every main iteration only restarts (r = b), so x stays 0 and each residual row is |b|,
    equal to the restatement's within 1e-5."""
    cfg = config("half_fan")
    p = rr.forward(cfg.ref, cfg.field(15)).astype(np.float32)
    vol, rep = cfg.rooster4d(p, niter=0, cgiter=3, tviter=3)
    assert (vol == 0.0).all() and rep["residuals"].shape == (0, 4)
    vol, rep = cfg.rooster4d(p, niter=2, cgiter=0, tviter=3)
    assert (vol == 0.0).all() and rep["residuals"].shape == (2, 1)
    b = np.linalg.norm(rr.back(cfg.ref, p.astype(np.float64)))
    np.testing.assert_allclose(rep["residuals"].ravel(), [b, b], rtol=1e-5)


@pytest.mark.gpu
def test_reconstruct_4d_takes_the_pixel_origin_from_the_stack(engine, tmp_path):
    """A stack whose .mha origin is (-nu du / 2, -nv dv / 2), as the stacks written here are, and a half-fan create_geometry:
    reconstruct_4d equals rooster4d with that pixel origin bit for bit, and differs from the default origin."""
    n, nu, nv, dim, spacing = 60, 32, 24, (24, 16, 20), (2.0, 2.0, 2.0)
    geo = recon.create_geometry(n, start_angle=90.0, source_to_isocenter=SID, source_to_detector=SDD, detector_offset_x=-HALF_FAN * nu * PIX)
    gpath = recon.save_geometry(geo, tmp_path / "geometry.xml")
    amp = pkg.respiratory.RespiratorySignal.create_sin4(total_seconds=n / 5.0, period=3.0, sampling_frequency=5.0).signal
    ph = np.hstack(phase_mod.calculate_phase(amp)).astype(np.float64)
    ph = (ph - ph.min()) / (ph.max() - ph.min())
    origin = (-nu * PIX / 2, -nv * PIX / 2)
    g = rr.Geometry(geo.gantry_angles, SID, SDD, nu, nv, PIX, PIX, dim, spacing, ph, 10, geo.projection_offsets_x, geo.projection_offsets_y, *origin)
    p = rr.forward(g, config("half_fan").field(16)).astype(np.float32)
    ppath = recon.write_mha(tmp_path / "projections_total_normalized.mha", p, (PIX, PIX, 1.0), origin + (0.0,))
    kw = dict(frames=10, niter=1, cgiter=2, tviter=2)
    out, _ = recon.reconstruct_4d(ppath, gpath, dimension=dim, spacing=spacing, amplitude_signal=amp, **kw)
    vol = recon.read_mha(out)[0]
    direct, _ = recon.rooster4d(p, geo, (PIX, PIX), origin, ph, dim, spacing, **kw)
    default, _ = recon.rooster4d(p, geo, (PIX, PIX), None, ph, dim, spacing, **kw)
    assert vol.tobytes() == direct.tobytes()
    assert vol.tobytes() != default.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _tiny_call(struct_size=None, **over):
    """mcgpu_rooster4d_reconstruct on the smallest valid problem (one projection of 2 x 2 pixels, one voxel, one frame, one CG step);
    -> (rc, volume, residuals, message).  struct_size: what the caller says its struct holds; the memory holds every field."""
    geo = recon.CircularGeometry(SID, SDD)
    geo.add_projection(30.0, 0.0, 0.0)
    lib, o, keep = recon._rooster_call(1, 2, 2, geo, (PIX, PIX), None, [0.0], (1, 1, 1), (4.0, 4.0, 4.0), None, 1, 1, 1, 0, 0.0, 0.0, None, True, 0)
    for k, v in over.items():
        setattr(o, k, v)
    if struct_size is not None:
        o.struct_size = struct_size
    p, vol = np.full((1, 2, 2), 3.0, np.float32), np.full((1, 1, 1, 1), -1.0, np.float32)
    rc = lib.mcgpu_rooster4d_reconstruct(C.byref(o), p.ctypes.data, vol.ctypes.data, None)
    return rc, vol, keep["residuals"].copy(), lib.mcgpu_last_error().decode(errors="replace")


def test_abi_a_device_that_does_not_exist_is_an_error_return(engine):
    """Device 9999: the runtime's refusal comes back as -1 with the failing call in the message (no GPU is needed to be refused)."""
    rc, vol, _, msg = _tiny_call(device=9999)
    assert rc == -1 and "!!HIP ERROR!! hipSetDevice" in msg and np.all(vol == -1.0)


@pytest.mark.gpu
def test_abi_a_valid_call_follows_a_refused_device(engine):
    assert _tiny_call(device=9999)[0] == -1
    rc, vol, res, msg = _tiny_call()
    assert rc == 0, msg
    assert np.isfinite(vol).all() and vol[0, 0, 0, 0] > 0 and res[0] > 0


@pytest.mark.gpu
def test_abi_old_header_reads_residuals_as_null(engine):
    """A caller built against a header that ends before `residuals` passes a shorter struct: the pointer that lies beyond reads as
    NULL, so nothing is written through it and the volume is bit for bit the one of the full struct with residuals = NULL."""
    full, cut = C.sizeof(recon._RoosterOptions), recon._RoosterOptions.residuals.offset
    assert cut + 8 == full
    rc0, want, _, msg = _tiny_call(residuals=C.POINTER(C.c_double)())
    assert rc0 == 0, msg
    rc1, got, res, msg = _tiny_call(struct_size=cut)
    assert rc1 == 0, msg
    assert got.tobytes() == want.tobytes() and (res == 0.0).all()
    assert (_tiny_call()[2] != 0.0).any()  # the full struct does write them
