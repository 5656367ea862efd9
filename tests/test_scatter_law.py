"""CPU tests: the float64 restatements of tests/scatter_ref.py against the CPU oracle (which tests/test_oracle_golden.py pins call by
call to the reference build), and the fixture tests/golden/scatter_law.npz against its generator -- before any GPU is involved.
tests/test_scatter_gpu.py then holds the HIP samplers to these restatements."""
import ctypes as C
import importlib.util

import numpy as np
import pytest
from scipy import stats

import golden_util as gu
import oracle_lib as ol
import parity
import scatter_cases as sc
import scatter_ref as sr

P_FALSE_ALARM = 1e-6   # of every chi-square test here; the seeds are fixed, so each test is deterministic


@pytest.fixture(scope="module")
def model(engine, tmp_path_factory):
    ctx = engine.create(sc.build_input(tmp_path_factory.mktemp("scatter_law")), device=-1)
    yield parity.tables_from_context(ctx), sr.tables(ctx)
    ctx.close()


@pytest.fixture(scope="module")
def golden():
    return gu.load("scatter_law.npz")


@pytest.mark.parametrize("material,energy", sc.CASES)
def test_compton_law_agrees_with_the_oracles_histogram(model, golden, material, energy):
    """compton_angular_law (envelope T S integrated in float64) against 2^20 oracle_gcoa samples: one-sample chi-square."""
    _, tab = model
    name = sc.key(material, energy)
    counts = golden[name + "_co_cos"].astype(np.float64)
    p = sr.compton_angular_law(energy, sc.material_index(material), golden[name + "_co_edges"], tab)
    assert abs(p.sum() - 1.0) < 1e-7   # two quadratures of one integral: far below the 1e-3 a bin of 2^14 events resolves
    expected = p * counts.sum()
    assert expected.min() >= 100
    chi2 = float(np.sum((counts - expected) ** 2 / expected))
    assert chi2 < stats.chi2.isf(P_FALSE_ALARM, counts.size - 1), chi2


def test_compton_s_is_the_oracles(model):
    """S(E, theta) of the restatement against oracle_compton_s (float32 arithmetic: a few 1e-7 per shell term)."""
    T, tab = model
    lib = ol.oracle()
    for material, energy in sc.CASES:
        mat = sc.material_index(material)
        cdt = np.array([0.0, 1e-4, 0.01, 0.3, 1.0, 1.7, 2.0])
        got = sr.compton_s(tab, mat, energy, cdt)
        want = np.array([lib.oracle_compton_s(C.byref(T.ct), float(energy), float(c), mat, ol.MATH_LIBM) for c in cdt])
        assert np.max(np.abs(got - want)) < 2e-5 * want.max(), (material, energy)


@pytest.mark.parametrize("material,energy", sc.CASES)
def test_rayleigh_replay_reproduces_the_oracle_call_by_call(model, material, energy):
    """rayleigh_replay fed the RANECU doubles that oracle_graa draws gives its cos(theta) to 1e-12 and consumes as many deviates."""
    T, tab = model
    lib = ol.oracle()
    mat, index = sc.material_index(material), sr.energy_index(tab, energy)
    n, depth = 1500, 48
    table, want, used = np.zeros((n, depth)), np.zeros(n), np.zeros(n, dtype=np.int64)
    s = (C.c_int * 2)()
    lib.oracle_init_prng(3, 150, 1234, s)
    for k in range(n):
        probe = (C.c_int * 2)(s[0], s[1])
        table[k] = [lib.oracle_ranecu_double(probe) for _ in range(depth)]
        c = C.c_double()
        lib.oracle_graa(C.byref(T.ct), C.c_float(energy), C.byref(c), mat, index, s)
        want[k] = c.value
    # deviates each call consumed: replay the stream once more and count the steps between the calls' seeds
    r = sr.rayleigh_replay(tab, mat, energy, index, sr.ArrayDeviates(table))
    assert np.max(np.abs(r["costh"] - want) / np.maximum(np.abs(want), 1e-3)) < 1e-12
    s = (C.c_int * 2)()
    lib.oracle_init_prng(3, 150, 1234, s)
    for k in range(n):
        c = C.c_double()
        before = (C.c_int * 2)(s[0], s[1])
        lib.oracle_graa(C.byref(T.ct), C.c_float(energy), C.byref(c), mat, index, s)
        steps = 0
        while (before[0], before[1]) != (s[0], s[1]):
            lib.oracle_ranecu_double(before)
            steps += 1
            assert steps <= depth
        used[k] = steps
    assert np.array_equal(used, r["drawn"]) and r["trials"].min() >= 1 and r["trials"].max() > 1


@pytest.mark.parametrize("mapping", ["f32", "f64"])
def test_fragile_share_of_the_rayleigh_replay(model, mapping):
    """A decision whose relative margin is below 1e-5 may fall the other way in another arithmetic; such events are left out of the
    per-event comparison on the device, and may be at most 0.5 % of a case.  Computed by the restatement alone."""
    _, tab = model
    ids = np.arange(1 << 16, dtype=np.uint64)
    for material, energy in sc.CASES:
        r = sr.rayleigh_replay(tab, sc.material_index(material), energy, sr.energy_index(tab, energy), sr.MwcDeviates(ids, 11, 0, mapping))
        share = float(np.mean(r["margin"] < 1e-5))
        assert share <= 0.005, (material, energy, share)


def test_rotation_is_the_oracles():
    """rotate / azimuth_about against oracle_rotate (rotate_double of the reference, float32 directions)."""
    lib = ol.oracle()
    rng = np.random.default_rng(5)
    n = 400
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:6] = [[0, 0, 1], [0, 0, -1], [1e-9, 0, 1], [0, 1e-9, -1], [1, 0, 0], [0, -1, 0]]
    d = d.astype(np.float32)
    costh, phi = rng.uniform(-1, 1, n), rng.uniform(0, 2 * np.pi, n)
    want = np.zeros((n, 3))
    for k in range(n):
        v = (C.c_float * 3)(*d[k])
        lib.oracle_rotate(v, costh[k], phi[k], ol.MATH_LIBM)
        want[k] = v[:]
    got = sr.rotate(d, costh, phi)
    assert np.max(np.abs(got - want)) < 2e-7          # the oracle's result is a float32 direction
    back = sr.azimuth_about(d, want)
    assert np.max(np.abs(np.angle(np.exp(1j * (back - phi))))) < 1e-6 / np.sqrt(1 - np.max(costh ** 2))


def test_fixture_is_what_its_generator_writes(model, golden):
    """One case of tests/golden/scatter_law.npz, sampled again by oracle/gen_scatter_golden.py's own functions."""
    T, tab = model
    spec = importlib.util.spec_from_file_location("gen_scatter_golden", ol.ROOT / "oracle" / "gen_scatter_golden.py")
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    k = sc.CASES.index(("blood", 60000.0))
    cos = gen.graa(T, sc.material_index("blood"), 60000.0, sr.energy_index(tab, 60000.0), sc.SAMPLES, gen.stream(2 * k + 1, 1313))
    assert np.array_equal(np.histogram(cos, golden["blood_60000_ra_edges"])[0], golden["blood_60000_ra_cos"])
    assert int(golden["samples"]) == sc.SAMPLES and all(int(golden[sc.key(m, e) + "_co_cos"].sum()) == sc.SAMPLES for m, e in sc.CASES)
