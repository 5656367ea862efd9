"""Row f16: motion-aware 4-D ROOSTER (csrc/rooster4d.hip: warp4_kernel and the temporal step y = W x; c = TVtime(y) - y; x += U c;
reconstruction.rooster4d_motion / rooster4d_motion_stage / reconstruct_4d_mc / frame_signals).
CPU: frame_signals against hand-computed weights, the float64 restatement (rooster_motion_ref.py) against array shifts, the C ABI's
refusals before any HIP call, the ctypes mirrors against the C compiler's layout, the Python refusals.
GPU: the three stages against the restatement, the whole loop, a moving sphere against plain ROOSTER, the file flow.
Parity against RTK's rtkfourdrooster --dvf --idvf is unpinned (RTK is absent here), and RTK's replace form is not what runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import abi_layout
import cases
import joseph_ref as jr
import rooster_motion_ref as mr
import rooster_ref as rr
import test_rooster4d as base  # the small problem of the plain ROOSTER tests: grid, geometry, phase, phantoms

pkg = cases.pkg
recon = pkg.reconstruction
DIM, SPACING, FRAMES, NU, NV, PIX = base.DIM, base.SPACING, base.FRAMES, base.NU, base.NV, base.PIX
STAGE_TOLERANCE = 1e-5   # the project's figure for one float32 operator against its float64 restatement (test_rooster4d.py)
FLOOR_CAP = 2.5e-6       # the float32-coordinate floor up to which STAGE_TOLERANCE is kept; beyond it the bound is 4 x the floor


def _rel(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


# ---------------------------------------------------------------------------------------------------------------- models and fields
def _smooth_model(dim, spacing, K, reach_voxels, seed):
    """(mean [3, nz, ny, nx], coefficients [K, 3, nz, ny, nx]) float32 in mm: smooth trigonometric fields whose displacement at
    |delta| <= 1 reaches `reach_voxels` voxels along every axis, with both signs near every face."""
    nx, ny, nz = dim
    z, y, x = np.meshgrid(np.linspace(-1, 1, nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    rng = np.random.default_rng(seed)
    sp = np.asarray(spacing, dtype=np.float64)

    def field(scale):
        a = rng.uniform(0.6, 1.0, size=(3, 3))
        ph = rng.uniform(0, 2 * np.pi, size=3)
        return np.stack([scale * sp[c] * (a[c, 0] * np.sin(2.2 * x + ph[c]) * np.cos(1.7 * y) + a[c, 1] * np.sin(2.9 * z + ph[c]) + 0.3 * a[c, 2] * x * y * z)
                         for c in range(3)])

    share = reach_voxels / (K + 1)
    return field(share).astype(np.float32), np.stack([field(share) for _ in range(K)]).astype(np.float32)


def _field4(dim, frames, seed):
    """A 4-D field whose frames differ: smooth plus 5 % noise, exact in float32."""
    nx, ny, nz = dim
    z, y, x = np.meshgrid(np.linspace(-1, 1, nz), np.linspace(-1, 1, ny), np.linspace(-1, 1, nx), indexing="ij")
    rng = np.random.default_rng(seed)
    out = [rng.uniform(0.5, 1.5) * np.exp(-((x - rng.uniform(-0.4, 0.4)) ** 2 + y ** 2 + (z - rng.uniform(-0.4, 0.4)) ** 2) / 0.4) + 0.2 * np.cos(2 * x + z + f)
           + rng.normal(scale=0.05, size=x.shape) for f in range(frames)]
    return np.stack(out).astype(np.float32)


def _states(frames, K, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(frames, K))


def _stage_tolerance(floor):
    return STAGE_TOLERANCE if floor <= FLOOR_CAP else 4.0 * floor


# ---------------------------------------------------------------------------------------------------------------- CPU: frame_signals
def test_frame_signals_equal_hand_computed_weights():
    """N = 2, phases 0, 1, 0.25, 0.75: phase 0 and phase 1 both give frame 0 the weight 1 and frame 1 the weight 0; 0.25 gives
    (0.5, 0.5); 0.75 lies between frame 1 (l) and frame 0 (h) with (0.5, 0.5).  Frame 0: weights 1, 1, 0.5, 0.5; frame 1: 0, 0, 0.5, 0.5."""
    phase = [0.0, 1.0, 0.25, 0.75]
    s1 = np.array([1.0, 2.0, 3.0, 4.0])
    want = np.array([[(1.0 + 2.0 + 1.5 + 2.0) / 3.0], [(1.5 + 2.0) / 1.0]])
    got = recon.frame_signals(phase, s1, 2)
    assert got.shape == (2, 1) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-15)
    s2 = np.stack([s1, 10.0 * s1 - 3.0], axis=1)
    got2 = recon.frame_signals(phase, s2, 2)
    np.testing.assert_allclose(got2, np.hstack([want, 10.0 * want - 3.0]), rtol=1e-14)
    np.testing.assert_allclose(mr.frame_signals(phase, s2, 2), got2, rtol=1e-14)
    ph = base._phase()
    s = np.stack([np.cos(2 * np.pi * ph), np.sin(2 * np.pi * ph)], axis=1)
    np.testing.assert_allclose(recon.frame_signals(ph, s, FRAMES), mr.frame_signals(ph, s, FRAMES), rtol=1e-13)
    assert recon.frame_signals([0.3, 0.9], [5.0, 7.0], 1).tolist() == [[6.0]]  # one frame is its own neighbour: the plain mean


def test_frame_signals_refuse_an_untouched_frame_and_a_wrong_length():
    with pytest.raises(ValueError, match="frame"):
        recon.frame_signals([0.0, 0.1], [1.0, 2.0], 3)      # frames 0 and 1 only
    with pytest.raises(ValueError, match="frame"):
        recon.frame_signals([0.0, 1.0], [1.0, 2.0], 2)      # frame 1 is named by both projections, with weight 0
    with pytest.raises(ValueError):
        recon.frame_signals([0.0, 0.5, 0.7], [1.0, 2.0], 2)


# ---------------------------------------------------------------------------------------------------------------- CPU: the restatement
def test_restated_warp_of_a_whole_voxel_translation_is_a_shift():
    """(+2, -1, +1) voxels along x, y, z at spacing (2, 1.5, 3) mm: the interior equals the shifted array, outside it the border is
    replicated."""
    dim, sp = (9, 6, 7), (2.0, 1.5, 3.0)
    x = np.random.default_rng(1).normal(size=(2, dim[2], dim[1], dim[0]))
    mean = np.zeros((3,) + x.shape[1:])
    coef = np.broadcast_to(np.array([2 * sp[0], -1 * sp[1], 1 * sp[2]])[None, :, None, None, None], (1, 3) + x.shape[1:])
    got = mr.warp(x, mean, coef, [[1.0], [0.0]], sp)
    np.testing.assert_array_equal(got[1], x[1])
    iz, iy, ix = np.meshgrid(np.arange(dim[2]), np.arange(dim[1]), np.arange(dim[0]), indexing="ij")
    want = x[0][np.clip(iz + 1, 0, dim[2] - 1), np.clip(iy - 1, 0, dim[1] - 1), np.clip(ix + 2, 0, dim[0] - 1)]
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[0][:-1, 1:, :-2], x[0][1:, :-1, 2:])        # the interior: a plain shift
    np.testing.assert_array_equal(got[0][:, :, -1], got[0][:, :, -3])             # replicated along x


def test_restated_zero_model_is_the_identity_and_gamma_zero_returns_the_input():
    dim, sp = (6, 5, 4), (2.0, 1.5, 3.0)
    x = np.random.default_rng(2).normal(size=(3, dim[2], dim[1], dim[0]))
    zero = (np.zeros((3,) + x.shape[1:]), np.zeros((2, 3) + x.shape[1:]))
    delta = _states(3, 2, 3)
    np.testing.assert_array_equal(mr.warp(x, *zero, delta, sp), x)
    model = _smooth_model(dim, sp, 2, 1.5, 4)
    np.testing.assert_array_equal(mr.motion_tv_time(x, model, model, delta, -delta, sp, 5, 0.0), x)
    np.testing.assert_allclose(mr.motion_tv_time(x, zero, zero, delta, delta, sp, 5, 0.3), rr.tv_time(x, 5, 0.3), rtol=0, atol=1e-15)
    assert _rel(mr.motion_tv_time(x, model, model, delta, -delta, sp, 5, 0.3), rr.tv_time(x, 5, 0.3)) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- CPU: the C ABI
def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    """mcgpu_rooster4d_motion and mcgpu_rooster4d_motion_report: the header's field names in order, sizeof and every offsetof as the
    C compiler lays them out, against the ctypes mirrors (tests/abi_layout.py).  The report begins with the fields of
    mcgpu_rooster4d_report."""
    mirrors = [("mcgpu_rooster4d_motion", recon._RoosterMotion), ("mcgpu_rooster4d_motion_report", recon._RoosterMotionReport)]
    abi_layout.assert_field_names(mirrors)
    n_plain = len(recon._RoosterReport._fields_)
    assert recon._RoosterMotionReport._fields_[:n_plain] == recon._RoosterReport._fields_
    assert [f[0] for f in recon._RoosterMotionReport._fields_[n_plain:]] == ["ms_warp", "ms_upload_model"]
    cc = abi_layout.c_compiler()
    assert cc is not None, "no C compiler"
    c_side = abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    assert c_side["mcgpu_rooster4d_motion"] == "56" and c_side["mcgpu_rooster4d_motion_report"] == "80"


class _Tiny:
    """The two motion entry points through ctypes on a small valid problem (2 x 2 x 2 voxels, 2 frames, K = 2)."""

    def __init__(self):
        geo = recon.CircularGeometry(300.0, 500.0, [30.0], [0.0], [0.0])
        self.lib, self.o, self.keep = recon._rooster_call(1, 2, 2, geo, (PIX, PIX), None, [0.25], (2, 2, 2), (4.0, 4.0, 4.0), None, 2, 1, 1, 1, 0.1, 0.0,
                                                          None, True, 0)
        zero = recon.MotionModel(np.zeros((3, 2, 2, 2)), np.zeros((2, 3, 2, 2, 2)), [0.0, 0.0])
        recon._rooster_motion(self.lib, 2, (2, 2, 2), (4.0, 4.0, 4.0), zero, zero, np.zeros((2, 2)))  # sets the argtypes
        self.lib.mcgpu_last_error.restype = C.c_char_p
        self.mean = np.zeros(3 * 8, np.float32)
        self.coefficients = np.full(2 * 3 * 8, 0.1, np.float32)
        self.delta_to = np.array([[0.5, -0.5], [1.0, 0.25]])
        self.delta_from = -self.delta_to
        self.proj = np.full((1, 2, 2), 3.0, np.float32)

    def motion(self, **fields):
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        m = recon._RoosterMotion(C.sizeof(recon._RoosterMotion), 2, self.mean.ctypes.data_as(fp), self.coefficients.ctypes.data_as(fp),
                                 self.mean.ctypes.data_as(fp), self.coefficients.ctypes.data_as(fp), self.delta_to.ctypes.data_as(dp),
                                 self.delta_from.ctypes.data_as(dp))
        for k, v in fields.items():
            setattr(m, k, v)
        return m

    def reconstruct(self, m):
        """(rc, message) of mcgpu_rooster4d_reconstruct_motion; a refused call leaves the volume untouched."""
        vol = np.full((2, 2, 2, 2), -1.0, np.float32)
        rc = self.lib.mcgpu_rooster4d_reconstruct_motion(C.byref(self.o), C.byref(m), self.proj.ctypes.data, vol.ctypes.data, None)
        assert rc == 0 or np.all(vol == -1.0)
        return rc, self.lib.mcgpu_last_error().decode(errors="replace")

    def stage(self, m, stage=0):
        """(rc, message) of mcgpu_rooster4d_motion_stage; a refused call leaves the output untouched."""
        src, out = np.full((2, 2, 2, 2), 0.5, np.float32), np.full((2, 2, 2, 2), -1.0, np.float32)
        rc = self.lib.mcgpu_rooster4d_motion_stage(C.byref(self.o), C.byref(m), stage, src.ctypes.data, out.ctypes.data, None)
        assert rc == 0 or np.all(out == -1.0)
        return rc, self.lib.mcgpu_last_error().decode(errors="replace")

    def both(self, m):
        return [self.reconstruct(m), self.stage(m)]


_NULL_F = C.POINTER(C.c_float)()
_REFUSALS = {
    "struct_size": (dict(struct_size=0), "set mcgpu_rooster4d_motion.struct_size = sizeof(mcgpu_rooster4d_motion)"),
    "K=0": (dict(n_signal_dims=0), "n_signal_dims must lie in 1..4"),
    "K=5": (dict(n_signal_dims=5), "n_signal_dims must lie in 1..4"),
    "to_reference_mean": (dict(to_reference_mean=_NULL_F), "a motion model array is NULL"),
    "to_reference_coefficients": (dict(to_reference_coefficients=_NULL_F), "a motion model array is NULL"),
    "from_reference_mean": (dict(from_reference_mean=_NULL_F), "a motion model array is NULL"),
    "from_reference_coefficients": (dict(from_reference_coefficients=_NULL_F), "a motion model array is NULL"),
}


@pytest.mark.parametrize("what", list(_REFUSALS))
def test_a_bad_motion_struct_is_refused_before_any_hip_call(engine, what):
    """-1 and a message from both entry points, outputs untouched; no GPU is needed to be refused."""
    t = _Tiny()
    fields, text = _REFUSALS[what]
    for fn, (rc, msg) in zip(("mcgpu_rooster4d_reconstruct_motion", "mcgpu_rooster4d_motion_stage"), t.both(t.motion(**fields))):
        assert rc == -1 and msg == f"!!ERROR!! {fn}: {text}", msg


@pytest.mark.parametrize("which, value", [("delta_to", np.nan), ("delta_from", np.nan), ("delta_to", np.inf), ("delta_from", 1e39)])
def test_a_delta_that_is_not_finite_is_refused_before_any_hip_call(engine, which, value):
    t = _Tiny()
    getattr(t, which)[1, 0] = value
    for rc, msg in t.both(t.motion()):
        assert rc == -1 and msg.endswith("delta is not finite"), msg


def test_an_unknown_motion_stage_is_refused_before_any_hip_call(engine):
    t = _Tiny()
    for stage in (-1, 3, 7):
        rc, msg = t.stage(t.motion(), stage=stage)
        assert rc == -1 and msg == f"!!ERROR!! mcgpu_rooster4d_motion_stage: unknown stage {stage}"
    t.o.n_frames = 33
    assert all(rc == -1 and "n_frames" in msg for rc, msg in t.both(t.motion()))  # the options are checked as the plain calls check them


# ---------------------------------------------------------------------------------------------------------------- CPU: Python refusals
def test_python_refuses_mismatched_models_grids_and_signal_counts():
    geo, ph = base._geometry(), base._phase()
    p = np.zeros((12, NV, NU), np.float32)
    shape = DIM[::-1]
    k1 = recon.MotionModel(np.zeros((3,) + shape), np.zeros((1, 3) + shape), [0.0], spacing=SPACING)
    k2 = recon.MotionModel(np.zeros((3,) + shape), np.zeros((2, 3) + shape), [0.0, 0.0], spacing=SPACING)
    other = recon.MotionModel(np.zeros((3, 20, 16, 23)), np.zeros((1, 3, 20, 16, 23)), [0.0])
    args = (p, geo, (PIX, PIX), None, ph)
    with pytest.raises(ValueError, match="signal dimensions"):
        recon.rooster4d_motion(*args, k1, k2, np.zeros((12, 1)), DIM, SPACING, frames=FRAMES)
    with pytest.raises(ValueError, match="resample the model"):
        recon.rooster4d_motion(*args, k1, other, np.zeros((12, 1)), DIM, SPACING, frames=FRAMES)
    with pytest.raises(ValueError, match="resample the model"):
        recon.rooster4d_motion(*args, other, k1, np.zeros((12, 1)), DIM, SPACING, frames=FRAMES)
    with pytest.raises(ValueError, match="resample the model"):
        recon.rooster4d_motion(*args, k1, k1, np.zeros((12, 1)), DIM, (2.0, 2.0, 2.5), frames=FRAMES)
    with pytest.raises(ValueError, match="12 projections but 11 signals"):
        recon.rooster4d_motion(*args, k1, k1, np.zeros((11, 1)), DIM, SPACING, frames=FRAMES)
    with pytest.raises(ValueError, match="signals of shape"):
        recon.rooster4d_motion(*args, k2, k2, np.zeros((12, 1)), DIM, SPACING, frames=FRAMES)   # K = 1 signals for K = 2 models
    with pytest.raises(ValueError, match="frame states"):
        recon.rooster4d_motion_stage("warp", np.zeros((FRAMES,) + shape, np.float32), k1, k1, np.zeros((FRAMES + 1, 1)), DIM, SPACING)
    with pytest.raises(ValueError, match="input shape"):
        recon.rooster4d_motion_stage("warp", np.zeros((FRAMES, 3, 3, 3), np.float32), k1, k1, np.zeros((FRAMES, 1)), DIM, SPACING)


# ---------------------------------------------------------------------------------------------------------------- GPU: the stages
SMALL_DIM, SMALL_SPACING = (13, 5, 7), (2.0, 1.5, 3.0)


@functools.lru_cache(maxsize=None)
def _small_case(K):
    """13 x 5 x 7 voxels of (2, 1.5, 3) mm, 4 frames, a smooth model that reaches 4 voxels (past every face, both ways) and whose
    planes ix = nx - 2, iy = ny - 2, iz = nz - 2 carry an exact +1 voxel displacement along their own axis: the cell i0 = n - 1,
    t = 0.  -> (x float32, mean, coefficients, states, W x restated in float64, the float32-coordinate floor)."""
    mean, coef = _smooth_model(SMALL_DIM, SMALL_SPACING, K, 4.0, 10 + K)
    for c, sl in enumerate((np.s_[:, :, -2], np.s_[:, -2, :], np.s_[-2, :, :])):
        mean[c][sl] = SMALL_SPACING[c]
        coef[:, c][(slice(None),) + sl] = 0.0
    states = _states(4, K, 20 + K)
    x = _field4(SMALL_DIM, 4, 30 + K)
    want = mr.warp(x, mean, coef, states, SMALL_SPACING)
    floor = _rel(mr.warp(x, mean, coef, states, SMALL_SPACING, dtype=np.float32), want)
    return x, mean, coef, states, want, floor


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_small_case_reaches_every_face_and_the_last_cell(K):
    """Checked without a GPU: what _small_case promises, and the float32-coordinate floor that sets the GPU tolerance."""
    x, mean, coef, states, want, floor = _small_case(K)
    n = np.array(SMALL_DIM)
    sp = np.array(SMALL_SPACING)
    idx = np.stack(np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")[::-1])  # ix, iy, iz
    exact, lo, hi = 0, np.zeros(3), np.zeros(3)
    for f in range(4):
        d = mean.astype(np.float64) + sum(coef[k].astype(np.float64) * states[f, k] for k in range(K))
        pos = idx + d / sp[:, None, None, None]
        lo, hi = np.minimum(lo, pos.min(axis=(1, 2, 3))), np.maximum(hi, pos.max(axis=(1, 2, 3)))
        exact += sum(int((pos[c] == n[c] - 1).sum()) for c in range(3))
    assert (lo < -0.5).all() and (hi > n - 1 + 0.5).all(), (lo, hi)  # past all six faces
    assert exact >= 3 * 4 * 5
    print(f"K = {K}: float32-coordinate floor {floor:.2e}")
    assert floor <= FLOOR_CAP


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_warp_and_unwarp_equal_the_restatement_on_the_small_grid(engine, K):
    """13 x 5 x 7 voxels of (2, 1.5, 3) mm, displacements past all six faces and exact whole voxels, K = 1 .. 4, W and U (the same
    operator on the other model).  Tolerance 1e-5 relative: the restatement evaluated with float32 coordinates stays within 1e-7
    of the float64 one (K = 1: 9.3e-8, K = 2: 8.7e-8, K = 3: 8.4e-8, K = 4: 9.2e-8), below the 2.5e-6 up to which the project's 1e-5 is kept.
    Measured on an MI355X: 1.0e-7, 8.9e-8, 9.8e-8."""
    x, mean, coef, states, want, floor = _small_case(K)
    tol = _stage_tolerance(floor)
    model = recon.MotionModel(mean, coef, np.zeros(K), spacing=SMALL_SPACING)
    zero = recon.MotionModel(np.zeros_like(mean), np.zeros_like(coef), np.zeros(K))
    got, rep = recon.rooster4d_motion_stage("warp", x, model, zero, states, SMALL_DIM, SMALL_SPACING)
    print(f"K = {K}: warp rel {_rel(got, want):.2e} (floor {floor:.2e}, bound {tol:.1e})")
    assert _rel(got, want) <= tol and _rel(got, x) > 0.05
    assert rep["ms_warp"] > 0 and rep["ms_upload_model"] > 0
    mean_signal = np.linspace(0.3, -0.2, K)  # U takes its own model, with its own mean signal
    other = recon.MotionModel(mean, coef, mean_signal)
    back, _ = recon.rooster4d_motion_stage("unwarp", x, zero, other, states + mean_signal, SMALL_DIM, SMALL_SPACING)
    assert _rel(back, want) <= tol


@pytest.mark.gpu
def test_warp_and_unwarp_take_32_frames_with_their_own_deltas(engine):
    """N = 32 (the bound of the kernel's argument array) on 5 x 4 x 3 voxels: every frame has its own state and equals the
    restatement on its own (float32-coordinate floor per frame: at most 1.2e-7, so 1e-5 holds)."""
    dim, sp, K = (5, 4, 3), (2.0, 1.5, 3.0), 2
    mean, coef = _smooth_model(dim, sp, K, 2.0, 40)
    states = _states(32, K, 41)
    x = _field4(dim, 32, 42)
    want = mr.warp(x, mean, coef, states, sp)
    floor = _rel(mr.warp(x, mean, coef, states, sp, dtype=np.float32), want)
    tol = _stage_tolerance(floor)
    model = recon.MotionModel(mean, coef, np.zeros(K))
    zero = recon.MotionModel(np.zeros_like(mean), np.zeros_like(coef), np.zeros(K))
    for stage, pair in (("warp", (model, zero)), ("unwarp", (zero, model))):
        got, _ = recon.rooster4d_motion_stage(stage, x, *pair, states, dim, sp)
        for f in range(32):
            assert _rel(got[f], want[f]) <= tol, (stage, f)
    assert len({want[f].tobytes() for f in range(32)}) == 32


@pytest.mark.gpu
def test_warp_with_a_zero_model_returns_the_input_bit_for_bit(engine):
    x = _field4(SMALL_DIM, 5, 50)
    shape = SMALL_DIM[::-1]
    zero = recon.MotionModel(np.zeros((3,) + shape), np.zeros((4, 3) + shape), np.zeros(4))
    for stage in ("warp", "unwarp"):
        got, _ = recon.rooster4d_motion_stage(stage, x, zero, zero, _states(5, 4, 51), SMALL_DIM, SMALL_SPACING)
        assert got.tobytes() == x.tobytes()


@pytest.mark.gpu
def test_warp_with_a_model_of_nan_and_inf_stays_on_the_grid(engine):
    """The clamp rule: fminf(fmaxf(fx, 0), n - 1) puts every index on the grid for any float, so a model full of NaN and +-Inf
    returns normally and every output value is one of the input's values (t = 0 at a clamped position) or NaN."""
    dim, sp, K = (5, 4, 3), (2.0, 1.5, 3.0), 2
    shape = dim[::-1]
    rng = np.random.default_rng(60)
    pool = np.array([np.nan, np.inf, -np.inf], np.float32)
    mean = pool[rng.integers(0, 3, size=(3,) + shape)]
    coef = pool[rng.integers(0, 3, size=(K, 3) + shape)]
    x = _field4(dim, 3, 61)
    bad = recon.MotionModel(mean, coef, np.zeros(K))
    states = np.array([[0.0, 0.0], [1.0, -1.0], [-0.5, 2.0]])
    for stage in ("warp", "unwarp"):
        got, _ = recon.rooster4d_motion_stage(stage, x, bad, bad, states, dim, sp)
        assert got.shape == x.shape
        for f in range(3):
            assert (np.isnan(got[f]) | np.isin(got[f], x[f])).all(), (stage, f)
    both, _ = recon.rooster4d_motion_stage("tv_time_motion", x, bad, bad, states, dim, sp, tviter=3, gamma_time=0.05)
    assert both.shape == x.shape


@functools.lru_cache(maxsize=None)
def _k2_models():
    """The K = 2 pair on the 24 x 16 x 20 grid: a smooth model of up to 1.5 voxels to the reference and its negative from it (an
    inverse to first order; nothing here needs more).  -> (to, from) as (mean, coefficients)."""
    mean, coef = _smooth_model(DIM, SPACING, 2, 1.5, 70)
    return (mean, coef), (-mean, -coef)


def _motion_models(pair):
    return tuple(recon.MotionModel(m, c, np.zeros(c.shape[0]), spacing=SPACING) for m, c in pair)


@pytest.mark.gpu
def test_tv_time_motion_stage_equals_the_restatement(engine):
    """24 x 16 x 20 voxels, 3 frames, K = 2, up to 1.5 voxels, 7 iterations at gamma 0.05: within the stage tolerance of the
    restatement (the float32-coordinate floor of the whole step measures 1.2e-7; an MI355X gives 1.2e-7), more than 1e-3 away from
    the plain tv_time stage (0.175), and with gamma_time = 0 the input comes back bit for bit."""
    to, frm = _k2_models()
    states = _states(FRAMES, 2, 71)
    x = (base._smooth4() + np.random.default_rng(6).normal(scale=0.1, size=(FRAMES,) + DIM[::-1])).astype(np.float32)
    want = mr.motion_tv_time(x, to, frm, states, states, SPACING, 7, 0.05)
    y32 = mr.warp(x, *to, states, SPACING, dtype=np.float32)
    floor = _rel(x + mr.warp(rr.tv_time(y32, 7, 0.05) - y32, *frm, states, SPACING, dtype=np.float32), want)
    tol = _stage_tolerance(floor)
    m_to, m_from = _motion_models((to, frm))
    got, rep = recon.rooster4d_motion_stage("tv_time_motion", x, m_to, m_from, states, DIM, SPACING, tviter=7, gamma_time=0.05)
    plain = base._stage("tv_time", x, base._geometry(), base._phase(), tviter=7, gamma_time=0.05)
    print(f"tv_time_motion: rel {_rel(got, want):.2e} (floor {floor:.2e}, bound {tol:.1e}), against plain tv_time {_rel(got, plain):.2e}")
    assert _rel(got, want) <= tol
    assert _rel(got, plain) > 1e-3 and _rel(got, x) > 1e-3
    assert rep["ms_warp"] > 0 and rep["ms_tv_time"] > 0
    same, _ = recon.rooster4d_motion_stage("tv_time_motion", x, m_to, m_from, states, DIM, SPACING, tviter=7, gamma_time=0.0)
    assert same.tobytes() == x.tobytes()


# ---------------------------------------------------------------------------------------------------------------- GPU: the loop
def _signals(ph):
    return np.stack([0.8 * np.cos(2 * np.pi * ph), 0.8 * np.sin(2 * np.pi * ph)], axis=1)


@pytest.mark.gpu
def test_rooster4d_motion_equals_the_restated_loop_and_repeats_bit_for_bit(engine):
    """niter 2, cgiter 3, tviter 5, gammas 0.002 / 0.002, the K = 2 pair: 1e-3 relative against rooster_motion_ref.rooster_motion,
    residuals at rtol 1e-3 (the project's loop tolerances; an MI355X gives 6.2e-7); a second run gives the same bytes; the warp
    kernels were timed."""
    geo, ph = base._geometry(), base._phase()
    p = base._projections(geo, ph)
    to, frm = _k2_models()
    m_to, m_from = _motion_models((to, frm))
    signals = _signals(ph)
    kw = dict(frames=FRAMES, niter=2, cgiter=3, tviter=5, gamma_space=0.002, gamma_time=0.002)
    vol, rep = recon.rooster4d_motion(p, geo, (PIX, PIX), None, ph, m_to, m_from, signals, DIM, SPACING, **kw)
    states = mr.frame_signals(ph, signals, FRAMES)
    np.testing.assert_allclose(rep["frame_signals"], states, rtol=1e-13)
    res_ref = []
    ref = mr.rooster_motion(base._ref_geometry(geo, ph), p.astype(np.float64), 2, 3, 5, 0.002, 0.002, to, frm, states, states, True, res_ref)
    print(f"loop: rel {_rel(vol, ref):.2e}")
    assert _rel(vol, ref) <= 1e-3
    np.testing.assert_allclose(rep["residuals"].ravel(), res_ref, rtol=1e-3)
    vol2, rep2 = recon.rooster4d_motion(p, geo, (PIX, PIX), None, ph, m_to, m_from, signals, DIM, SPACING, **kw)
    assert vol.tobytes() == vol2.tobytes() and rep["residuals"].tobytes() == rep2["residuals"].tobytes()
    assert rep["ms_warp"] > 0 and rep["ms_upload_model"] > 0 and rep["ms_forward"] > 0
    assert rep["peak_device_bytes"] > 4 * vol[0].size * (5 * FRAMES + 2 * 3 * 3)  # five 4-D vectors and the two K = 2 models


@pytest.mark.gpu
def test_zero_models_agree_with_plain_rooster(engine):
    """With zero models W and U are the identity and x + (TVtime(x) - x) is TVtime(x) up to one float32 rounding per voxel: 1e-5
    relative against rooster4d."""
    geo, ph = base._geometry(), base._phase()
    p = base._projections(geo, ph)
    shape = DIM[::-1]
    zero = recon.MotionModel(np.zeros((3,) + shape), np.zeros((2, 3) + shape), [0.0, 0.0], spacing=SPACING)
    kw = dict(frames=FRAMES, niter=2, cgiter=3, tviter=5, gamma_space=0.002, gamma_time=0.002)
    vol, _ = recon.rooster4d_motion(p, geo, (PIX, PIX), None, ph, zero, zero, _signals(ph), DIM, SPACING, **kw)
    plain, _ = recon.rooster4d(p, geo, (PIX, PIX), None, ph, DIM, SPACING, **kw)
    print(f"zero models against plain ROOSTER: rel {_rel(vol, plain):.2e}")
    assert _rel(vol, plain) <= 1e-5


@pytest.mark.gpu
def test_a_moving_sphere_gains_from_a_strong_temporal_tv_along_the_model(engine):
    """A 7 mm sphere that moves by 5 mm (2.5 voxels) per signal unit along IEC Z, signals -1, 0, 1, 36 projections of 32 x 24 pixels,
    3 frames; the models are the exact translations (K = 1): to_reference (0, 0, 5) mm, from_reference (0, 0, -5) mm per unit.
    gamma_time 0.1, gamma_space 0.002, niter 4, cgiter 4, tviter 10.  Asserted: the frame-mean RMS error of rooster4d_motion is at
    most 0.5 x that of rooster4d on the same data (the float64 restatement gives 0.35; no benefit is 1.0; swapped or sign-flipped
    models land above 1).  Measured per frame on an MI355X: plain 0.0546 0.0408 0.0541, motion-aware 0.0157 0.0212 0.0153, ratio of
    the frame means 0.349 (profiles/rooster4d_motion.md)."""
    n = 36
    geo = base._geometry(n)
    ph = np.array([(k % 3) / 3.0 for k in range(n)])
    signals = np.array([[-1.0, 0.0, 1.0][k % 3] for k in range(n)])[:, None]
    truth = np.stack([base._sphere(c) for c in (-5.0, 0.0, 5.0)])
    p = np.zeros((n, NV, NU), np.float32)
    for k in range(n):
        p[k] = jr.project(truth[k % 3], SPACING, -(np.array(DIM) - 1) / 2 * SPACING, [geo.gantry_angles[k]], [0.0], [0.0], base.SID, base.SDD, NU, NV, PIX, PIX,
                          -(NU - 1) / 2 * PIX, -(NV - 1) / 2 * PIX)[0]
    shape = DIM[::-1]

    def translation(mm):
        coef = np.zeros((1, 3) + shape, np.float32)
        coef[0, 2] = mm
        return recon.MotionModel(np.zeros((3,) + shape, np.float32), coef, [0.0], spacing=SPACING)

    kw = dict(frames=3, niter=4, cgiter=4, tviter=10, gamma_time=0.1, gamma_space=0.002)
    plain, _ = recon.rooster4d(p, geo, (PIX, PIX), None, ph, DIM, SPACING, **kw)
    moved, rep = recon.rooster4d_motion(p, geo, (PIX, PIX), None, ph, translation(5.0), translation(-5.0), signals, DIM, SPACING, **kw)
    np.testing.assert_allclose(rep["frame_signals"].ravel(), [-1.0, 0.0, 1.0], atol=1e-12)
    rms_plain = np.sqrt(((plain - truth) ** 2).mean(axis=(1, 2, 3)))
    rms_moved = np.sqrt(((moved - truth) ** 2).mean(axis=(1, 2, 3)))
    print("moving sphere, rms per frame: plain", " ".join(f"{v:.4f}" for v in rms_plain), "| motion-aware", " ".join(f"{v:.4f}" for v in rms_moved),
          f"| ratio of the frame means {rms_moved.mean() / rms_plain.mean():.3f}")
    assert rms_moved.mean() <= 0.5 * rms_plain.mean(), (rms_plain, rms_moved)


# ---------------------------------------------------------------------------------------------------------------- GPU: the file flow
@pytest.mark.gpu
def test_reconstruct_4d_mc_file_flow(engine, tmp_path):
    """Stack + geometry.xml + two fitted correspondence models + an amplitude signal in, recon_rooster4d_mc.mha (4-D) + .yaml with both
    hashes, K and the temporal update out; equal to rooster4d_motion on the converted models, and not to reconstruct_4d."""
    import yaml
    n = 60
    geo = recon.create_geometry(n, start_angle=90.0, source_to_isocenter=base.SID, source_to_detector=base.SDD, detector_offset_x=0.0)
    gpath = recon.save_geometry(geo, tmp_path / "geometry.xml")
    amp = pkg.respiratory.RespiratorySignal.create_sin4(total_seconds=n / 5.0, period=3.0, sampling_frequency=5.0).signal
    ph = np.hstack(pkg.phase.calculate_phase(amp)).astype(np.float64)
    ph = (ph - ph.min()) / (ph.max() - ph.min())
    g = rr.Geometry(geo.gantry_angles, base.SID, base.SDD, NU, NV, PIX, PIX, DIM, SPACING, ph, FRAMES)
    p = rr.forward(g, base._smooth4(11)).astype(np.float32)
    origin = (-(NU - 1) / 2 * PIX, -(NV - 1) / 2 * PIX)
    ppath = recon.write_mha(tmp_path / "projections_total_normalized.mha", p, (PIX, PIX, 1.0), origin + (0.0,))
    # MCGeometry arrays [x, y, z] of 24 x 20 x 16 voxels -> the FDK grid (24, 16, 20); fields in voxels
    shape, voxel = (24, 20, 16), (2.0, 2.0, 2.0)
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, shape[2]), np.linspace(-1, 1, shape[1]), np.linspace(-1, 1, shape[0]), indexing="ij")
    bump = np.exp(-(xx ** 2 + yy ** 2 + zz ** 2) / 0.5).transpose(2, 1, 0)
    unit = np.stack([0.2 * bump, 1.2 * bump, -0.4 * bump])
    model_signals = np.array([[-1.0], [0.0], [1.0]])
    CorrespondenceModel = pkg.correspondence.CorrespondenceModel
    to_model = CorrespondenceModel().fit(np.stack([unit * s[0] for s in model_signals]).astype(np.float32), model_signals, reference_phase=1)
    from_model = CorrespondenceModel().fit(np.stack([-unit * s[0] for s in model_signals]).astype(np.float32), model_signals, reference_phase=1)
    signals = np.asarray(amp, dtype=np.float64)[:, None] * 2.0 - 1.0
    kw = dict(frames=FRAMES, niter=1, cgiter=2, tviter=2, gamma_time=0.01)
    out, rep = recon.reconstruct_4d_mc(ppath, gpath, to_model, from_model, signals, voxel, amplitude_signal=amp, dimension=DIM, spacing=SPACING, **kw)
    assert out == tmp_path / "reconstructions" / "recon_rooster4d_mc.mha"
    assert rep["ms_warp"] > 0 and rep["ms_upload_model"] > 0 and rep["frame_signals"].shape == (FRAMES, 1)
    vol, sp, org = recon.read_mha(out)
    assert vol.shape == (FRAMES,) + DIM[::-1] and sp == [2.0, 2.0, 2.0, 1.0]
    assert org == [-(d - 1) / 2 * s for d, s in zip(DIM, SPACING)] + [0.0]
    assert b"NDims = 4" in out.read_bytes()[:200]
    record = yaml.safe_load(out.with_suffix(".yaml").read_text())
    for key in ("niter", "cgiter", "tviter", "gamma_time", "gamma_space", "dimension", "spacing", "wpc", "geometry", "path", "regexp", "output_filepath"):
        assert key in record, key
    assert record["motion_to_reference"] == to_model.model_hash[:7] and record["motion_from_reference"] == from_model.model_hash[:7]
    assert record["motion_to_reference"] != record["motion_from_reference"]
    assert record["signal_n_dims"] == 1 and record["temporal_update"] == "increment" and record["cgiter"] == 2 and record["fp"] == "Joseph"
    m_to = recon.MotionModel.from_correspondence_model(to_model, voxel, dimension=DIM, spacing=SPACING)
    m_from = recon.MotionModel.from_correspondence_model(from_model, voxel, dimension=DIM, spacing=SPACING)
    direct, _ = recon.rooster4d_motion(p, geo, (PIX, PIX), origin, ph, m_to, m_from, signals, DIM, SPACING, **kw)
    assert vol.tobytes() == direct.tobytes()
    plain_out, _ = recon.reconstruct_4d(ppath, gpath, dimension=DIM, spacing=SPACING, amplitude_signal=amp, **kw)
    assert _rel(vol, recon.read_mha(plain_out)[0]) > 1e-4
    with pytest.raises(ValueError):
        recon.reconstruct_4d_mc(ppath, gpath, to_model, from_model, signals, voxel, dimension=DIM, spacing=SPACING)  # no phase or amplitude signal
    with pytest.raises(ValueError, match="resample the model"):
        recon.reconstruct_4d_mc(ppath, gpath, to_model, from_model, signals, voxel, amplitude_signal=amp, dimension=(24, 20, 16), spacing=SPACING)
