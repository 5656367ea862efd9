"""CPU tests of the ray-traced primary's rule as tests/primary_ref.py restates it (the HIP kernel is then held to the restatement by
tests/test_primary_gpu.py): the ray is the inverse of tally_image, the mass thickness against closed forms and a brute-force sampler,
the normalisation against an independent solid-angle quadrature, the energy quadrature against a finer one, and the plane as the
expectation of the reference's own Monte Carlo (the libm oracle) -- plus the layout of the ctypes mirrors."""
import os
import re
import time

import numpy as np
import pytest

import abi_layout
import oracle_lib as ol
import parity
import primary_ref as pr

POSES = {"slab_angles": (0, 1, 2), "water": (0,)}      # 270, 300.5, 45.25 degrees (rotation_flag 1); the unrotated single pose


@pytest.fixture(scope="module")
def host(engine, case_dir):
    """Host-only contexts and their restatements, one per case, shared by the tests of this module and never changed."""
    made = {}

    def get(name):
        if name not in made:
            ctx = engine.create(case_dir(name), device=-1)
            made[name] = (ctx, pr.Primary(ctx))
        return made[name]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def test_mirrors_match_the_header(engine, tmp_path):
    mirrors = [("mcgpu_primary_options", engine.PrimaryOptions), ("mcgpu_primary_report", engine.PrimaryReport)]
    abi_layout.assert_field_names(mirrors)
    cc = abi_layout.c_compiler()
    if cc is None:
        pytest.skip("no C compiler")
    abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    header = abi_layout.HEADER.read_text()
    assert re.search(r"int mcgpu_primary_project\(mcgpu_ctx \*ctx, const mcgpu_primary_options \*options, float \*planes, mcgpu_primary_report \*report\);", header)


# ---- 1: geometry of the ray ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["slab_angles", "water"])
def test_ray_through_a_pixel_centre_scores_in_that_pixel(host, name):
    ctx, P = host(name)
    tables = parity.tables_from_context(ctx)
    for p in POSES[name]:
        assert int(P.detector[p]["rotation_flag"]) == (1 if name == "slab_angles" else 0)
        pose = P.pose(p)
        q = P.sub_points(pose, 1, 1).reshape(-1, 3) - pose["src"]
        d = q / np.linalg.norm(q, axis=1)[:, None]
        word, _ = tables.tally_events(p, np.broadcast_to(pose["src"], d.shape), d, 60000.0, 0)
        pz, px = np.divmod(np.arange(P.nz * P.nx), P.nx)
        assert np.array_equal(word, px + pz * P.nx), (name, p, int(np.count_nonzero(word != px + pz * P.nx)))
        # the pixel pitch of the map is the tally's: U and V are orthogonal, of the pitch's length, and normal to the detector normal
        pitch = 1.0 / np.array([ctx.getf("inv_pixel_size_x"), ctx.getf("inv_pixel_size_z")])
        assert abs(np.linalg.norm(pose["u"]) - pitch[0]) < 1e-6 * pitch[0] and abs(np.linalg.norm(pose["v"]) - pitch[1]) < 1e-6 * pitch[1]
        assert abs(pose["u"] @ pose["v"]) < 1e-6 * pitch[0] * pitch[1] and abs(pose["u"] @ pose["nrm"]) < 1e-6 and abs(pose["v"] @ pose["nrm"]) < 1e-6


# ---- 2: closed form, one material ------------------------------------------------------------------------------------------
def slab_chord(src, d, bbox):
    """Chord of the box [0, bbox] along rays src + t d, t >= 0, by the slab method in float64 (0: a miss)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, hi = (0.0 - src) / d, (bbox - src) / d
    par = d == 0.0
    near = np.where(par, -np.inf, np.minimum(lo, hi)).max(axis=1)
    far = np.where(par, np.inf, np.maximum(lo, hi)).min(axis=1)
    ok = np.all(~par | ((src >= 0.0) & (src <= bbox)), axis=1)
    return np.where(ok, np.maximum(far - np.maximum(near, 0.0), 0.0), 0.0)


def test_water_thickness_is_the_chord_times_the_density(host):
    ctx, P = host("water")
    assert tuple(P.n) == (24, 24, 24) and np.allclose(P.vs, 1.0)
    pose = P.pose(0)
    src, bbox = pose["src"], P.n * P.vs
    q = P.sub_points(pose, 1, 1).reshape(-1, 3) - src
    rays = [q / np.linalg.norm(q, axis=1)[:, None]]
    k = np.arange(25, dtype=np.float64)
    corners = np.stack(np.meshgrid(k[::3], k[::4], k[::3], indexing="ij"), axis=-1).reshape(-1, 3)          # through voxel corners
    edges = np.array([[0, 0, z] for z in k] + [[24, 0, z] for z in k] + [[x, 0, 0] for x in k] + [[x, 24, 24] for x in k] + [[0, y, 24] for y in k], dtype=np.float64)
    for target in (corners, edges):
        v = target - src
        rays.append(v / np.linalg.norm(v, axis=1)[:, None])
    rays.append(np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0],         # along an axis (the source sits at x = z = 12)
                          [0.6, 0.8, 0.0], [0.0, 0.8, 0.6], [0.0, 0.6, -0.8],                            # parallel to one axis
                          [0.995, 0.0998749, 0.0], [0.0, 0.01, 0.99995], [-0.5, -0.5, 0.7071]]))        # misses
    d = np.concatenate(rays)
    d /= np.linalg.norm(d, axis=1)[:, None]
    t = P.thickness(src, d)
    chord = slab_chord(src[None, :], d, bbox[None, :])
    h2o = int(P.vox_material[0, 0, 0])
    rho = float(P.vox_density[0, 0, 0])
    assert np.count_nonzero(chord == 0.0) >= 3 and np.count_nonzero(chord > 0.0) > 10000 and chord.max() > 24.0
    assert np.all(np.delete(t, h2o, axis=1) == 0.0)
    err = np.abs(t[:, h2o] - rho * chord)
    print("water: largest |t - rho chord| =", err.max(), "g/cm^2 of", (rho * chord).max())
    assert err.max() <= 1e-12 * (rho * chord).max()
    assert np.all(t[-3:] == 0.0) and np.all(chord[-3:] == 0.0)            # the three plain misses; a grazing ray may keep a chord of 1e-15


# ---- 3: closed form, several materials -------------------------------------------------------------------------------------
def test_slab_thickness_against_a_brute_force_sampler(host):
    ctx, P = host("slab_angles")
    n_points = 100_000
    rng = np.random.default_rng(20261020)
    bbox = P.n * P.vs
    for p in POSES["slab_angles"]:
        pose = P.pose(p)
        px, pz = rng.integers(0, 128, 40), rng.integers(0, P.nz, 40)
        q = (pose["o"] + (px + rng.random(40))[:, None] * pose["u"] + (pz + rng.random(40))[:, None] * pose["v"]) - pose["src"]
        d = q / np.linalg.norm(q, axis=1)[:, None]
        t = P.thickness(pose["src"], d)
        with np.errstate(divide="ignore"):
            lo, hi = (0.0 - pose["src"]) / d, (bbox - pose["src"]) / d
        tmin, tmax = np.maximum(np.minimum(lo, hi).max(axis=1), 0.0), np.maximum(lo, hi).min(axis=1)
        assert np.count_nonzero(tmax > tmin) >= 20
        materials_seen = set()
        for r in np.nonzero(tmax > tmin)[0]:
            step = (tmax[r] - tmin[r]) / n_points
            s = tmin[r] + (np.arange(n_points) + 0.5) * step
            idx = np.clip(np.floor((pose["src"][None, :] + s[:, None] * d[r][None, :]) / P.vs[None, :]).astype(np.int64), 0, P.n - 1)
            mat, rho = P.vox_material[idx[:, 2], idx[:, 1], idx[:, 0]], P.vox_density[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float64)
            brute = np.bincount(mat, weights=rho * step, minlength=pr.MAXMAT)
            # the sampler misplaces at most one step per interface; a ray crosses at most 8 of them in this phantom (box, two inserts)
            tol = 8.0 * step * float(P.vox_density.max())
            assert np.all(np.abs(t[r] - brute) <= tol), (p, r, np.abs(t[r] - brute).max(), tol)
            materials_seen |= set(np.nonzero(brute)[0].tolist())
        assert len(materials_seen) == 3, materials_seen
    assert np.all(P.thickness(pose["src"], -d) == 0.0)                # flying away from the volume


# ---- 4: normalisation ------------------------------------------------------------------------------------------------------
def detector_share(P, pose, n_phi=400_001):
    """The share of the aperture's solid angle that the detector subtends (rotation_flag 0), independently of the projector: for
    every azimuth phi (dense midpoint rule) the accepted interval of z = cos(theta) cut with the interval that lands on the
    detector's rows, where the column x(phi) is on the detector."""
    d0 = P.detector[0]
    src, cmin = pose["src"], d0["corner_min_rotated_to_Y"].astype(np.float64)
    Y = float(d0["center"][1]) - src[1]
    width, height = float(d0["width_X"]), float(d0["height_Z"])
    phi = pose["phi_lo"] + (np.arange(n_phi) + 0.5) * pose["d_phi"] / n_phi
    g = pose["h"] * np.abs(np.sin(phi)) / np.sqrt(1.0 + (pose["h"] * np.sin(phi)) ** 2)
    a_lo, a_hi = np.maximum(pose["z_lo"], -g), np.minimum(pose["z_hi"], g)
    x = src[0] + Y / np.tan(phi)
    on = (x >= cmin[0]) & (x <= cmin[0] + width)
    # rows: z_det = src.z + Y cot(theta) / sin(phi), cot(theta) = z / sqrt(1 - z^2), monotone in z
    c_lo, c_hi = (cmin[2] - src[2]) * np.sin(phi) / Y, (cmin[2] + height - src[2]) * np.sin(phi) / Y
    z_of = lambda c: c / np.sqrt(1.0 + c * c)
    accepted = np.maximum(a_hi - a_lo, 0.0)
    seen = np.where(on, np.maximum(np.minimum(a_hi, z_of(c_hi)) - np.maximum(a_lo, z_of(c_lo)), 0.0), 0.0)
    return float(seen.sum() / accepted.sum()), float(accepted.sum() * pose["d_phi"] / n_phi)


def test_plane_integrates_to_the_mean_energy_in_vacuum(host):
    """Measured here: residual 5.9e-9 at su = sv = 4 (the half-fan edge of the test detector falls on a pixel boundary, so no sub-point
    straddles it; what is left is the smoothness of cos(psi) / r^2 over a sixteenth of a pixel)."""
    ctx, P0 = host("air")
    P = pr.Primary(ctx)
    P.set_voxels(P0.vox_material, np.full(P0.vox_density.shape, 1.0e-9, dtype=np.float32))
    pose = P.pose(0)
    share, omega = detector_share(P, pose)
    assert abs(omega - pose["omega"]) <= 1e-9 * omega, (omega, pose["omega"])      # the solid angle itself, by another quadrature
    assert abs(P.mean_energy() - ctx.getf("mean_energy_spectrum")) <= 1e-6 * P.mean_energy()
    area = 1.0 / (ctx.getf("inv_pixel_size_x") * ctx.getf("inv_pixel_size_z"))
    total = float(P.plane(0, (4, 4), 2).sum()) * area
    _, W, _ = P.spectrum(2)
    assert abs(W.sum() - P.mean_energy()) <= 1e-12 * W.sum()
    want = P.mean_energy() * share
    residual = abs(total - want) / want
    print("normalisation: total", total, "want", want, "share", share, "residual", residual)
    measured = 5.9e-9
    assert residual <= min(4.0 * measured, 1.0e-3)


# ---- 5: quadrature ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water", "slab_angles", "tissue22"])
def test_two_point_quadrature_against_eight(host, name):
    """Measured: largest relative difference of a ray 2.2e-8 (water), 2.4e-8 (slab_angles), 2.8e-8 (tissue22; its two poses cross 18 of
    the 22 materials inside the half-fan): four orders below the bound, the default stays 2."""
    ctx, P = host(name)
    worst = 0.0
    for p in range(len(P.source)):
        pose = P.pose(p)
        q = P.sub_points(pose, 1, 1).reshape(-1, 3) - pose["src"]
        d = q / np.linalg.norm(q, axis=1)[:, None]
        d = d[P.inside(pose, d)]
        t = P.thickness(pose["src"], d)
        s2, s8 = P.transmitted(t, 2), P.transmitted(t, 8)
        worst = max(worst, float(np.max(np.abs(s2 - s8) / s8)))
        seen = int(np.count_nonzero(np.any(t > 0, axis=0)))
    print(name, "Qn 2 against 8: largest relative difference", worst, "materials crossed in the last pose", seen)
    assert worst <= 1e-4


# ---- 6: against the reference's own Monte Carlo ----------------------------------------------------------------------------
MC_HISTORIES = 20_000_000    # per projection: about 3 s of the oracle on 8 threads, 3 s of restatement
MC_SUBSAMPLES = (2, 2)


@pytest.mark.parametrize("name,p", [("water", 0), ("slab_angles", 0), ("slab_angles", 1), ("slab_angles", 2)])
def test_plane_is_the_expectation_of_the_oracle_monte_carlo(host, name, p):
    ctx, P = host(name)
    tables = parity.tables_from_context(ctx)
    hpt, threads = 1000, min(8, os.cpu_count() or 1)
    nbatches = MC_HISTORIES // hpt
    t0 = time.time()
    image, w2, _ = tables.track_with_variance(p, 20261020, 0, nbatches, hpt, ol.MATH_LIBM, threads)
    t_mc = time.time() - t0
    n = float(nbatches * hpt)
    mc = image.reshape(4, P.nz, P.nx)[0].astype(np.float64)
    var = np.maximum(w2.reshape(4, P.nz, P.nx)[0] - mc * mc / n, 0.0)
    scale = 100.0 * n / (ctx.getf("inv_pixel_size_x") * ctx.getf("inv_pixel_size_z"))     # plane value -> tally units of n histories
    tested = P.plane(p, MC_SUBSAMPLES, 2, flip=False) * scale
    fine = P.plane(p, (8, 8), 2, flip=False) * scale
    print(f"{name} p{p}: {int(n)} histories in {t_mc:.1f} s, restatements in {time.time() - t0 - t_mc:.1f} s")
    pr.expectation_statement(mc, var, tested, fine, f"{name} p{p}")
