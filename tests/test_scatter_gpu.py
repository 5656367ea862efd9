"""The FAST personality's scattering samplers, event by event (run with -m gpu on an MI355X): csrc/kat_scatter.inc runs the service
bodies of the photon kernels (serve_compton, serve_rayleigh: compton_draw, compton_momentum_trial, rayleigh_trial, rotate_dir) on one
event per thread, in both arithmetics (`fast`, `fast64`), from streams that oracle/fast_rng.py replays.  They are held to the float64
restatements of tests/scatter_ref.py and to the reference's own histograms (tests/golden/scatter_law.npz, oracle/gen_scatter_golden.py);
tests/test_scatter_law.py pins both to the CPU oracle.  The detector images cannot do this: scattered photons are a small, smooth share
of them, and an azimuth leaves no trace in them at all.

Cases: tests/scatter_cases.py.  Not reached: rayleigh_trial's branch xmax < 0.01, which needs a photon below 124 eV -- the tables start
at 5 keV -- and is not forced with a fabricated table.

Every launch is 2^20 events; the per-event replays take the first 2^18 of them (the restatement runs on the host).  A quarter of the
events fly along +z and a quarter along -z: rotate_dir then hands the polar cosine through unchanged (out.w = +-cos), which is how the
tests see it without the rounding of a dot product.

Float32 tolerances are 4 x the largest deviation measured on an MI355X (the hardware's sine, cosine, reciprocal and reciprocal square
root carry no error bound one could cite, and a maximum over 1e4..1e6 events underestimates the worst case), under a cap that does not
depend on the measurement.  Measured figures: the constants below, and DESIGN.md section 1, row of this file.

Wall time of this file on one MI355X: DESIGN.md section 1."""
import numpy as np
import pytest
from scipy import stats

import golden_util as gu
import scatter_cases as sc
import scatter_ref as sr

pytestmark = pytest.mark.gpu

MODES = ("fast", "fast64")
N = sc.SAMPLES
REPLAY = 1 << 18
SEED, KEY, FIRST_ID = 20241, 3, (1 << 33) + 12345      # ids beyond 32 bits: the high counter word of the stream takes part
PH_FLIGHT, PH_NEW = 0, 5
P_FALSE_ALARM = 1e-6                                    # of every chi-square test; seeds are fixed, so each test is deterministic
FRAGILE_MARGIN, FRAGILE_CAP = 1e-5, 0.005

# --- measured on an MI355X (this file prints every figure before it asserts) -------------------------------------------------------
ROTATE_F32_MEASURED = 2.4e-7     # 2.30e-7 / 2.37e-7 / 1.34e-7: largest |component|, |norm - 1|, |dot - cos| deviation of the float32 rotate_dir from float64
RAYLEIGH_OMC_F32_MEASURED = 4.0e-7  # 3.97e-7 (bone_100, 5.5 keV; 1.6e-7 .. 2.7e-7 at 60 and 124.5 keV): largest |omc - restatement| of the float32 Rayleigh sampler
ROTATE_F32_CAP, RAYLEIGH_OMC_F32_CAP = 1e-5, 2e-6
# fast64 hands a float32 direction out: a dot product of two such directions carries three roundings of 2^-24 each and the
# normalisation of the incoming one, < 2e-7; along z the cosine itself is visible and held to 1e-12 (see _cos_within)
F64_DOT_BOUND = 2e-7
F64_AZIMUTH_BOUND = 1e-6


def rotate_bound():
    return min(4.0 * ROTATE_F32_MEASURED, ROTATE_F32_CAP)


@pytest.fixture(scope="module")
def gpu_engine(engine):
    return engine


class Model:
    """One context that holds the three materials, the events' inputs, and every device run / replay the tests share."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.tab = sr.tables(ctx)
        rng = np.random.default_rng(2024)
        d = rng.normal(size=(N, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        k = np.arange(N) % 4
        d[k == 0] = [0.0, 0.0, 1.0]
        d[k == 1] = [0.0, 0.0, -1.0]
        self.d_in = d.astype(np.float32)
        self.axis = np.where(k == 0, 1.0, np.where(k == 1, -1.0, 0.0))   # +-1: along +-z, 0: a general direction
        unit = self.d_in.astype(np.float64)
        self.unit = unit / np.linalg.norm(unit, axis=1, keepdims=True)
        self.ids = FIRST_ID + np.arange(N, dtype=np.uint64)
        self.runs, self.replays = {}, {}

    def run(self, mode, kind, material, energy):
        key = (mode, kind, material, energy)
        if key not in self.runs:
            e, d, calls, phase, state = self.ctx.kat_scatter(mode, kind, self.d_in, energy, self.ids, sc.material_index(material), seed=SEED, stream_key=KEY)
            out = d.astype(np.float64)
            self.runs[key] = dict(e=e, d=out, calls=calls.astype(np.int64), phase=phase.astype(np.int64), state=state.astype(np.uint64),
                                  cos=np.where(self.axis != 0, self.axis * out[:, 2], np.sum(self.unit * out, axis=1)))
        return self.runs[key]

    def replay(self, mode, material, energy):
        """rayleigh_replay of the first REPLAY events with the device's deviates, then the azimuth's draw."""
        key = (mode, material, energy)
        if key not in self.replays:
            dev = sr.MwcDeviates(self.ids[:REPLAY], SEED, KEY, "f32" if mode == "fast" else "f64")
            r = sr.rayleigh_replay(self.tab, sc.material_index(material), energy, sr.energy_index(self.tab, energy), dev)
            dev.u32(np.arange(REPLAY))
            r["state"] = np.stack([dev.x, dev.c], axis=1)
            self.replays[key] = r
        return self.replays[key]


@pytest.fixture(scope="module")
def model(gpu_engine, tmp_path_factory):
    with gpu_engine.create(sc.build_input(tmp_path_factory.mktemp("scatter_gpu")), device=0) as ctx:
        yield Model(ctx)


@pytest.fixture(scope="module")
def golden():
    return gu.load("scatter_law.npz")


def turn_of(mode, u32):
    """The azimuth as a fraction of a turn, from the 32-bit deviate: rng_f's mapping in `fast`, rng_d's in `fast64`."""
    u = np.asarray(u32, dtype=np.uint64)
    if mode == "fast":  # rounded to float32, as rng_f hands it out
        return (((u >> np.uint64(8)).astype(np.float64) + 0.25) * 2.0 ** -24).astype(np.float32).astype(np.float64)
    return (u.astype(np.float64) + 0.5) * 2.0 ** -32


def transverse_error(d_in, d_out, phi):
    """Distance between d_out's component across d_in and where the azimuth phi puts it (a per-component quantity: an error of
    the azimuth weighs sin(theta))."""
    _, e1, e2 = sr._frame(d_in)
    a, b = np.sum(d_out * e1, axis=1), np.sum(d_out * e2, axis=1)
    st = np.hypot(a, b)
    return np.hypot(a - st * np.cos(phi), b - st * np.sin(phi))


def _cos_within(out_w, ref, rel):
    """A float32 that a double within `rel` of `ref` rounds to."""
    lo, hi = (ref - rel * np.abs(ref)).astype(np.float32).astype(np.float64), (ref + rel * np.abs(ref)).astype(np.float32).astype(np.float64)
    return (out_w >= lo) & (out_w <= hi)


def test_rotate_f32_against_float64(model):
    """The float32 rotate_dir (v_sin_f32 / v_cos_f32 of a turn fraction, v_rsq_f32, v_rcp_f32, the polar angle as omc = 1 - cos)
    against the textbook rotation in float64: unit norm, dot(in, out) = 1 - omc, every component.  20 000 random inputs and the
    product of the edges: directions along +-z and 1e-8 .. 1e-5 off it (either side of the 1e-12 that dxy once switched at), lengths
    off by +-1e-3, omc in {0, 1e-7, 1, 2 - 2^-23, 2}, deviates on every quadrant border.
    Measured on an MI355X: see ROTATE_F32_MEASURED; the assertion is at 4 x that, and never above 1e-5 per component (a quarter
    turn, a sign or a wrong branch costs 1e-1 or more)."""
    rng = np.random.default_rng(9)
    n = 20000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    omc = np.concatenate([rng.uniform(0, 2, n // 2), 10.0 ** rng.uniform(-8, 0, n // 2)])
    u = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    small = [0.0, 1e-8, -1e-8, 1e-7, -3e-7, 9e-7, 1.1e-6, -3e-6, 1e-5]
    e_d = [[a, b, w] for a in small for b in small for w in (1.0, -1.0)]
    e_d += [list(v * s) for v in d[:8] for s in (1.0 + 1e-3, 1.0 - 1e-3)] + [[1, 0, 0], [0, -1, 0], [0.6, 0.8, 0]]
    e_omc = [0.0, 1e-7, 1.0, 2.0 - 2.0 ** -23, 2.0]
    e_u = [0, 1, 2 ** 29 - 1, 2 ** 29, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 255, 2 ** 30 + 256, 2 ** 31 - 1, 2 ** 31, 3 * 2 ** 30 - 1, 3 * 2 ** 30,
           2 ** 32 - 2 ** 29, 2 ** 32 - 256, 2 ** 32 - 1]
    g = np.array([[*a, b, c] for a in e_d for b in e_omc for c in e_u])
    d = np.concatenate([d, g[:, :3]]).astype(np.float32)
    omc = np.concatenate([omc, g[:, 3]]).astype(np.float32)
    u = np.concatenate([u, g[:, 4].astype(np.uint64)])
    _, out, _, _, state = model.ctx.kat_scatter("fast", "rotate", d, omc, u)
    assert np.array_equal(state[:, 0].astype(np.uint64), u)          # the injected deviate is the one the generator handed out
    out = out.astype(np.float64)
    o64 = omc.astype(np.float64)
    costh, sinth = 1.0 - o64, np.sqrt(o64 * (2.0 - o64))
    want = sr.rotate(d, costh, 2.0 * np.pi * turn_of("fast", u), sinth)
    unit = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    dev_c = float(np.max(np.abs(out - want)))
    dev_n = float(np.max(np.abs(np.linalg.norm(out, axis=1) - 1.0)))
    dev_d = float(np.max(np.abs(np.sum(unit * out, axis=1) - costh)))
    edge = np.arange(d.shape[0]) >= n
    print(f"\nrotate f32: component {dev_c:.3e} (edges {np.max(np.abs(out - want)[edge]):.3e}), norm {dev_n:.3e}, dot {dev_d:.3e}; "
          f"bound {rotate_bound():.3e}; near-axis inputs {int(np.sum((d[:, 0] ** 2 + d[:, 1] ** 2 < 1e-12) & (d[:, 0] ** 2 + d[:, 1] ** 2 > 0)))}")
    assert np.isfinite(out).all()
    assert dev_n <= rotate_bound() and dev_d <= rotate_bound() and dev_c <= rotate_bound()


@pytest.mark.parametrize("material,energy", sc.CASES)
@pytest.mark.parametrize("mode", MODES)
def test_rayleigh_replay(model, mode, material, energy):
    """Per event: the float64 restatement of GRAa's loop, fed the device's own deviates, gives the trial count (= service calls), the
    final generator state and cos(theta).  Events with a decision closer than 1e-5 (relative) are left out; they may be 0.5 % at
    most (tests/test_scatter_law.py checks that on the CPU; measured shares: 2e-4 .. 1.5e-3).  The deviate of the table look-up is
    (u + 1/2) 2^-32 in both builds (scatter_ref.MwcDeviates.next: wide), that of the acceptance test rng_f's or rng_d's.  cos(theta): to 1e-12 relative under
    fast64 along z, where the float32 direction shows the cosine itself (2e-7 elsewhere: the roundings of a float32 dot product); under
    `fast`, omc to 4 x RAYLEIGH_OMC_F32_MEASURED and never above 2e-6."""
    dev, r = model.run(mode, "rayleigh", material, energy), model.replay(mode, material, energy)
    assert np.all(dev["phase"] == PH_FLIGHT) and np.all(dev["e"] == np.float32(energy)) and dev["calls"].min() >= 1
    keep = r["margin"] >= FRAGILE_MARGIN
    share = 1.0 - float(np.mean(keep))
    s = slice(0, REPLAY)
    same = (dev["calls"][s] == r["trials"]) & np.all(dev["state"][s] == r["state"], axis=1)
    cos, axis = dev["cos"][s], model.axis[s]
    err = np.abs((1.0 - cos) - (1.0 - r["costh"]))
    on_axis = keep & same & (axis != 0)
    print(f"\nrayleigh {mode} {material} {energy}: fragile {share:.2e}, disagreeing among them {int(np.sum(~same & ~keep))}, "
          f"omc error on the axis {err[on_axis].max():.3e}, elsewhere {err[keep & same & (axis == 0)].max():.3e}")
    assert share <= FRAGILE_CAP
    assert np.all(same[keep]), int(np.sum(~same & keep))
    if mode == "fast64":
        assert np.all(_cos_within(cos[on_axis], r["costh"][on_axis], 1e-12))
        assert err[keep & (axis == 0)].max() <= F64_DOT_BOUND
    else:
        assert err[keep].max() <= min(4.0 * RAYLEIGH_OMC_F32_MEASURED, RAYLEIGH_OMC_F32_CAP)


def _chi2_two_sample(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    assert a.sum() == b.sum() and (a + b).min() >= 200
    return float(np.sum((a - b) ** 2 / (a + b))), a.size - 1


@pytest.mark.parametrize("material,energy", sc.CASES)
@pytest.mark.parametrize("mode", MODES)
def test_scatter_laws_against_the_oracle(model, golden, mode, material, energy):
    """2^20 device events against 2^20 of the reference's (oracle_gcoa / oracle_graa, LIBM): two-sample chi-square of cos(theta) for both
    processes and of E'/E for Compton; one-sample chi-square of the Compton cos(theta) against the law envelope T S integrated in
    float64; the mean E'/E in every cos(theta) bin within 5 standard errors (what a shell drawn with the wrong conditional probability
    moves); the share of Compton products below the tables' floor (PH_NEW) within 5 standard errors.  Thresholds:
    chi2.isf(1e-6, bins - 1)."""
    name = sc.key(material, energy)
    ra, co = model.run(mode, "rayleigh", material, energy), model.run(mode, "compton", material, energy)
    report = []

    def check(label, chi2, dof):
        report.append(f"{label} {chi2:.1f}/{dof}")
        return chi2 < stats.chi2.isf(P_FALSE_ALARM, dof)

    ok = [check("rayleigh cos", *_chi2_two_sample(np.histogram(ra["cos"], golden[name + "_ra_edges"])[0], golden[name + "_ra_cos"]))]
    edges = golden[name + "_co_edges"]
    b = np.searchsorted(edges, co["cos"], side="right") - 1
    counts = np.bincount(b, minlength=edges.size - 1)
    ok.append(check("compton cos", *_chi2_two_sample(counts, golden[name + "_co_cos"])))
    tau = co["e"].astype(np.float64) / np.float64(np.float32(energy))
    ok.append(check("compton E'/E", *_chi2_two_sample(np.histogram(tau, golden[name + "_co_tedges"])[0], golden[name + "_co_tau"])))
    expected = sr.compton_angular_law(energy, sc.material_index(material), edges, model.tab) * N
    assert expected.min() >= 100
    ok.append(check("compton cos against the law", float(np.sum((counts - expected) ** 2 / expected)), counts.size - 1))
    # mean E'/E per cos(theta) bin
    n_o = golden[name + "_co_cos"].astype(np.float64)
    mean_o, mean_d = golden[name + "_co_tsum"] / n_o, np.bincount(b, weights=tau, minlength=counts.size) / counts
    var_o = golden[name + "_co_tsq"] / n_o - mean_o ** 2
    var_d = np.bincount(b, weights=tau * tau, minlength=counts.size) / counts - mean_d ** 2
    z = (mean_d - mean_o) / np.sqrt(np.maximum(var_o, 0) / n_o + np.maximum(var_d, 0) / counts + 1e-30)
    # Compton products below the floor end as PH_NEW, everything else flies on
    low = co["e"] < model.tab["e0"]
    n_new, n_low = int(np.sum(co["phase"] == PH_NEW)), int(golden[name + "_co_low"])
    p = (n_new + n_low) / (2.0 * N)
    print(f"\nlaws {mode} {name}: " + ", ".join(report) + f"; max |z| of the bin means {np.abs(z).max():.2f}; below the floor {n_new} vs {n_low}")
    assert np.array_equal(co["phase"] == PH_NEW, low) and np.all((co["phase"] == PH_NEW) | (co["phase"] == PH_FLIGHT))
    assert all(ok), report
    assert np.abs(z).max() <= 5.0
    assert abs(n_new - n_low) <= 5.0 * np.sqrt(2.0 * N * p * (1.0 - p))
    assert n_low == 0 or n_new > 0


def _deviates_consumed(ids, state, limit=1 << 16):
    """How many draws lead from the seeding of each stream to `state` (x, c); -1 where `limit` draws do not."""
    x, c = sr.fast_rng.seed_streams(ids, SEED, KEY)
    n = np.full(ids.size, -1, dtype=np.int64)
    todo = np.arange(ids.size)
    for k in range(1, limit + 1):
        x[todo], c[todo] = sr.fast_rng.mwc_step(x[todo], c[todo])
        hit = (x[todo] == state[todo, 0]) & (c[todo] == state[todo, 1])
        n[todo[hit]] = k
        todo = todo[~hit]
        if todo.size == 0:
            break
    return n


@pytest.mark.parametrize("material,energy", sc.CASES)
@pytest.mark.parametrize("mode", MODES)
def test_azimuth_and_deviate_budget(model, mode, material, energy):
    """The last deviate of an event is its azimuth -- rng_u32 returns the generator's new x, so the final state names it -- and the
    direction must lie at 2 pi turn about the incoming one (across the incoming direction: to the rotate test's bound under `fast`,
    1e-6 under fast64).  This is the quarter-turn check the float32 kernel never had.
    Deviates consumed, from the position of the final state in the replayed stream: Rayleigh, what the restatement consumed plus
    one.  Compton, what the service calls allow: a call that draws tau takes 4 (tau twice, shell, test), one that redraws the shell at
    an accepted angle 2, a momentum trial 1 or 2 more, the azimuth 1 -- so 7 for an event of one call, and 2c + 6 .. 4c + 3 for c > 1
    calls (the first call draws tau, the last completes both momentum tests).
    An event of ONE call drew its tau from its first two deviates: cos(theta) = 1 - (1 - tau) / (tau ek) of the float64 tau, to
    4 ulp of a float32 tau (v_log, v_exp, the product, the quotient of taumin) through d cos / d tau = 1 / (tau^2 ek), plus 4 ulp
    of the float32 quotient 1 - cos <= 2 itself, plus the dot product's 2e-7."""
    s = slice(0, REPLAY)
    ids = model.ids[s]
    tol = rotate_bound() if mode == "fast" else F64_AZIMUTH_BOUND
    ra, r = model.run(mode, "rayleigh", material, energy), model.replay(mode, material, energy)
    keep = r["margin"] >= FRAGILE_MARGIN
    n_ra = _deviates_consumed(ids, ra["state"][s])
    t_ra = transverse_error(model.d_in[s], ra["d"][s], 2.0 * np.pi * turn_of(mode, ra["state"][s, 0]))
    co = model.run(mode, "compton", material, energy)
    n_co, calls = _deviates_consumed(ids, co["state"][s]), co["calls"][s]
    t_co = transverse_error(model.d_in[s], co["d"][s], 2.0 * np.pi * turn_of(mode, co["state"][s, 0]))
    one = calls == 1
    first = sr.fast_rng.streams_u32(ids, SEED, KEY, 2).astype(np.uint64)
    xi0, xi1 = (turn_of("fast", first[:, k]) for k in (0, 1))      # both arithmetics draw tau with rng_f
    tau, branch_margin = sr.compton_first_tau(energy, xi0, xi1)
    ek = np.float64(np.float32(energy)) * sr.INV_MC2
    cos_first = 1.0 - np.minimum((1.0 - tau) / (tau * ek), 2.0)
    sel = one & (branch_margin >= FRAGILE_MARGIN)
    cos_err = np.abs(co["cos"][s] - cos_first)[sel]
    cos_tol = 4.0 * 2.0 ** -24 / (tau[sel] ** 2 * ek) + 4.0 * 2.0 ** -24 * 2.0 + F64_DOT_BOUND
    print(f"\nazimuth {mode} {material} {energy}: rayleigh {t_ra[keep].max():.3e}, compton {t_co.max():.3e} (bound {tol:.3e}); compton calls "
          f"mean {calls.mean():.2f} max {calls.max()}, one call {one.mean():.3f}; first-trial cos error / bound {np.max(cos_err / cos_tol):.3f}")
    assert np.array_equal(n_ra[keep], r["drawn"][keep] + 1)
    assert t_ra[keep].max() <= tol and t_co.max() <= tol
    assert n_co.min() >= 7 and calls.min() >= 1
    assert np.all(n_co[one] == 7)
    assert np.all((n_co[~one] >= 2 * calls[~one] + 6) & (n_co[~one] <= 4 * calls[~one] + 3))
    assert sel.sum() >= 10000 and np.all(cos_err <= cos_tol)      # a fifth to a half of the events take one call


@pytest.mark.parametrize("material,energy", sc.CASES)
@pytest.mark.parametrize("kind", ["rayleigh", "compton"])
def test_fast_and_fast64_take_the_same_decisions(model, kind, material, energy):
    """With the same ids and seed both arithmetics draw the same 32-bit words: the service calls and the final generator state agree
    for all but 0.5 % of the events at most, and where they do, E' agrees to 1e-4 relative and cos(theta) to 1e-5.
    Measured on an MI355X, 2^20 events per case: differing events 0 in 17 of the 18 cases and 9.5e-7 (one event) in Rayleigh /
    bone_100 / 5.5 keV; E' to 6.3e-5 (Compton, 5.5 keV); cos(theta) to 4.2e-7 in both processes.
    The Rayleigh cases are what made the float32 rayleigh_trial take the whole 32-bit word for its table look-up: with rng_f's 24 bits
    there, against the 32 of rng_d, cos(theta) differed by 3.5e-4 (h2o), 1.4e-4 (blood) and 1.3e-5 (bone_100) at 124.5 keV and by up to
    9.4e-6 at 60 keV -- GRAa's distribution is steep at the top of the tables, 2^-24 in the deviate is 1e-4 in omc there."""
    a, b = model.run("fast", kind, material, energy), model.run("fast64", kind, material, energy)
    same = (a["calls"] == b["calls"]) & np.all(a["state"] == b["state"], axis=1)
    e_rel = np.abs(a["e"].astype(np.float64) / b["e"].astype(np.float64) - 1.0)[same]
    c_abs = np.abs(a["cos"] - b["cos"])[same]
    print(f"\nfast vs fast64 {kind} {material} {energy}: differing {1.0 - same.mean():.2e}, E' {e_rel.max():.3e}, cos {c_abs.max():.3e}")
    assert 1.0 - same.mean() <= 0.005
    assert e_rel.max() <= 1e-4 and c_abs.max() <= 1e-5
