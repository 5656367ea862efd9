"""CPU tests of the noise of the ray-traced primary as tests/primary_noise_ref.py restates it (the HIP code is then held to the
restatement by tests/test_primary_noise_gpu.py): the moment planes against closed forms, the sampler's mean, variance and zero
fraction on constant planes, the inputs of the GPU comparisons against the caps the issue leaves to the builder (ambiguous pixels,
aperture-edge blocks) -- plus the layout of the ctypes mirrors.  Every test prints its figures before it asserts."""
import re

import numpy as np
import pytest

import abi_layout
import primary_noise_ref as nr
import primary_ref as pr


@pytest.fixture(scope="module")
def host(engine, case_dir):
    """Host-only contexts and their restatements, one per case, shared by the tests of this module."""
    made = {}

    def get(name):
        if name not in made:
            ctx = engine.create(case_dir(name), device=-1)
            made[name] = (ctx, nr.MomentPrimary(ctx))
        return made[name]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def test_mirrors_match_the_header(engine, tmp_path):
    mirrors = [("mcgpu_primary_options", engine.PrimaryOptions), ("mcgpu_primary_report", engine.PrimaryReport),
               ("mcgpu_primary_noisy_options", engine.PrimaryNoisyOptions)]
    abi_layout.assert_field_names(mirrors)
    header = abi_layout.HEADER.read_text()
    for name in ("mcgpu_primary_moments", "mcgpu_primary_noisy", "mcgpu_sample_compound_poisson", "mcgpu_sample_gaussian"):
        assert re.search(r"int %s\(" % name, header) and name in engine.ABI_SYMBOLS, name
    cc = abi_layout.c_compiler()
    if cc is not None:
        abi_layout.assert_sizes_and_offsets(mirrors, cc, tmp_path)
    print("mirrors:", [m[0] for m in mirrors], "C compiler:", cc)


# ---- 1: moment planes ----------------------------------------------------------------------------------------------------------
def test_monoenergetic_spectrum_gives_powers_of_the_energy(host):
    ctx, P = host("slab_angles")
    E0 = 61234.5
    keep = P.prob.copy(), P.espc.copy()
    try:
        b = int(np.searchsorted(P.espc, E0)) - 1
        P.prob = np.zeros_like(P.prob)
        P.prob[b] = 1.0
        P.espc = P.espc.copy()
        P.espc[b], P.espc[b + 1] = E0, E0                       # a bin of no width: every node is E0
        planes = P.moment_planes(1, (1, 1), (2,), moments=(0, 1, 2))
    finally:
        P.prob, P.espc = keep
    m0, m1, m2 = (planes[(k, 2, "f64")] for k in (0, 1, 2))
    lit = m0 > 0
    worst = max(float(np.max(np.abs(m1[lit] / (E0 * m0[lit]) - 1.0))), float(np.max(np.abs(m2[lit] / (E0 * E0 * m0[lit]) - 1.0))))
    print(f"monoenergetic {E0} eV: lit {int(lit.sum())}, largest relative deviation of M_k from E^k M_0: {worst:.2e}")
    assert lit.sum() > 1000 and worst <= 1e-12
    assert np.all(m1[~lit] == 0) and np.all(m2[~lit] == 0)


def test_a_path_without_matter_gives_the_moments_of_the_spectrum(host):
    ctx, P = host("water")
    keep = P.vox_material, P.vox_density
    try:
        P.set_voxels(P.vox_material, np.zeros_like(P.vox_density))      # nothing attenuates
        P._kept.clear()
        planes = P.moment_planes(0, (1, 1), (2,), moments=(0, 1, 2), flip=False)
    finally:
        P.set_voxels(*keep)
        P._kept.clear()
    pose = P.pose(0)
    q = P.sub_points(pose, 1, 1).reshape(-1, 3) - pose["src"]
    r2 = np.sum(q * q, axis=1)
    d = q / np.sqrt(r2)[:, None]
    geom = np.where(P.inside(pose, d), np.abs(d @ pose["nrm"]) / r2, 0.0).reshape(P.nz, P.nx) / pose["omega"]
    E, W, _ = pr.Primary.spectrum(P, 2)
    for k in (0, 1, 2):
        want = float(np.sum(W / E * E ** k)) * geom
        got = planes[(k, 2, "f64")]
        err = float(np.max(np.abs(got - want)) / want.max())
        print(f"no matter, k = {k}: sum_q W_q^(k) = {float(np.sum(W / E * E ** k)):.6g}, largest deviation {err:.2e} of the maximum")
        assert err <= 1e-12 and np.array_equal(got > 0, geom > 0)
    assert abs(float(np.sum(W / E)) - 1.0) <= 1e-12                       # M_0 counts photons: the probabilities sum to 1


def test_moment_one_is_the_plane_of_primary_ref(host):
    ctx, P = host("slab_angles")
    planes = P.moment_planes(2, (2, 3), (2,), moments=(1,))
    assert np.array_equal(planes[(1, 2, "f64")], pr.Primary(ctx).plane(2, (2, 3), 2))


# ---- 2: the sampler's moments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", nr.STAT_LAMBDAS)
def test_sampler_moments_on_constant_planes(lam):
    m0, m1, m2, histories = nr.stat_case(lam)
    planes = [np.full((1,) + nr.STAT_SHAPE, v, dtype=np.float32) for v in (m0, m1, m2)]
    value, count, ambiguous = nr.compound_poisson(*planes, histories, nr.STAT_AREA, seed=20261021)
    assert abs(histories * nr.STAT_AREA * m0 / lam - 1.0) < 1e-12
    nr.sampler_statement(value.astype(np.float32), m0, m1, m2, histories, nr.STAT_AREA, f"restatement lambda {lam:g}")
    print(f"mean count {count.mean():.4f}, ambiguous {int(ambiguous.sum())}")
    assert abs(count.mean() - lam) <= 5.0 * np.sqrt(lam / count.size) + 0.01


def test_sampler_gives_exact_zeros_where_it_must():
    shape = (1, 9, 11)
    m0 = np.full(shape, 1e-4, dtype=np.float32)
    m0[0, ::2, ::3] = 0.0
    m1, m2 = m0 * np.float32(5e4), m0 * np.float32(2.6e9)
    value, count, _ = nr.compound_poisson(m0, m1, m2, 1e6, 0.01, seed=3)
    print(f"zeros {int(np.sum(value == 0))} of {value.size}, counts of zero {int(np.sum(count == 0))}")
    assert np.all(value[m0 == 0] == 0.0) and np.all(value[count == 0] == 0.0) and np.any(value > 0)
    g, _ = nr.gaussian(np.full(shape, -1.0), np.full(shape, -4.0), seed=3)            # a negative variance reads as 0, the value clamps
    assert np.all(g == 0.0)
    again, _, _ = nr.compound_poisson(m0, m1, m2, 1e6, 0.01, seed=3)
    other, _, _ = nr.compound_poisson(m0, m1, m2, 1e6, 0.01, seed=4)
    assert np.array_equal(value, again) and not np.array_equal(value, other)


# ---- the caps the issue leaves to the builder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", nr.SAMPLER_SHAPES, ids=["7x5", "16x16", "17x33"])
def test_inputs_of_the_sampler_comparison_stay_under_the_ambiguity_cap(shape):
    m0, m1, m2 = nr.sampler_inputs(shape)
    lam = nr.SAMPLER_HISTORIES * nr.SAMPLER_AREA * m0.astype(np.float64)
    for want in nr.SAMPLER_LAMBDAS:
        assert np.any(np.abs(lam - want) <= 1e-6 * max(want, 1e-12)), want
    assert np.any(lam == 64.0) and np.any((lam > 63.8) & (lam < 64.0))
    flagged = 0
    for seed in (7, 2 ** 63 + 11):
        value, count, ambiguous = nr.compound_poisson(m0, m1, m2, nr.SAMPLER_HISTORIES, nr.SAMPLER_AREA, seed, first_projection=5)
        flagged = max(flagged, int(ambiguous.sum()))
        assert np.all(value[m0 == 0] == 0.0)
    print(f"{shape}: pixels {m0.size}, ambiguous at most {flagged} (cap {0.001 * m0.size:.2f})")
    assert flagged <= 0.001 * m0.size


@pytest.mark.parametrize("name,p", [("water", 0), ("slab_angles", 1)])
def test_restatement_leaves_out_few_blocks_as_aperture_edge(host, name, p):
    """The mask of "M_2 is what the engine tallies" comes from the restatement alone: held here to the cap of 0.2 of the lit blocks."""
    ctx, P = host(name)
    upper, lower, var, fine = nr.w2_expectations(P, p, 100_000_000, (2, 2))
    ub, lb, vb, lit, edge, used = nr.w2_blocks(upper, lower, var, fine)
    rel = float((upper.sum() - lower.sum()) / upper.sum())
    print(f"{name} p{p}: blocks lit {int(lit.sum())}, left out {int(edge.sum())}, truncation lowers the sum by {rel:.2e}, "
          f"relative sd of the sum {float(np.sqrt(var.sum()) / upper.sum()):.2e}")
    assert lit.sum() > 50 and edge.sum() <= 0.2 * lit.sum()
    assert np.all(lower <= upper) and 0 < rel < 1e-3
