"""The two ends of a FAST history, event by event (run with -m gpu on an MI355X): csrc/kat_history.inc runs start_history
(sample_source_energy, sample_source_direction, source_entry with cylinder_span and entry_face_shell or move_to_bbox, classify_real),
score_finished (tally_pixel) and exterior_record + exterior_hop -- the production functions themselves -- on one item per thread, in both
arithmetics (`fast`, `fast64`), under the poses of tests/source_cases.py, from streams that oracle/fast_rng.py replays.  They are held to
the restatements of tests/source_ref.py, which tests/test_source_law.py pins to the CPU oracle.  A whole detector image cannot do this:
a pixel-boundary slip moves counts between neighbouring columns far below its noise, a mis-read alias table tilts the spectrum by a
smooth per cent, the cot clamp moves photons by 1e-6 rad at the beam edge only, and the tangent, parallel and miss branches of the
cylinder test hold almost no ray of a CBCT fan.

Every SOURCE launch is 2^18 ids beyond 2^33; the host replays the first 2^16.  TALLY and HOP launches hold at most 2^16 designed items.

Float32 tolerances are 4 x the largest deviation measured on an MI355X (the hardware's sine, cosine, reciprocal, logarithm and square
root carry no error bound one could cite), under a cap that does not depend on the measurement.  Every figure is printed before it is
asserted; the measured ones are the constants below and DESIGN.md section 1, row of this file."""
import numpy as np
import pytest
from scipy import stats

import source_cases as sc
import source_ref as so

pytestmark = pytest.mark.gpu

MODES = ("fast", "fast64")
P_FALSE_ALARM = 1e-6                 # of every chi-square test; seeds are fixed, so each test is deterministic
FRAGILE_CAP, SHELL_CAP = 0.005, 0.001

# --- measured on an MI355X (this file prints every figure before it asserts) -------------------------------------------------------
# direction: largest |dx|, |dy| deviation in the beam frame and | |d| - 1 | of the device's float32 direction from the restatement
# (v_sin_f32 / v_cos_f32 of phi, v_sqrt_f32, under a pose three float32 multiply-adds per component), over all cases and both modes:
# 2.56e-7 (dx, 45.25 degrees), 2.28e-7 (dy), 2.29e-7 (norm); 2.04e-7 / 1.78e-7 / 1.83e-7 in the unrotated pose.  Cap 1e-5.
DIRECTION_F32_MEASURED, DIRECTION_F32_CAP = 2.6e-7, 1.0e-5
# position [cm]: largest deviation of the entry point from the restatement (from the device's own float32 direction), per route:
#   "plain"  move_to_bbox: 1.55e-5 from the restated point, 4.26e-5 off the ray (float32 sum at |focal spot| = 92 cm, ulp 7.6e-6 cm)
#   "box"    source_entry / exterior_hop against the box alone: 1.19e-5 / 3.3e-6 (v_rcp_f32 slab quotients, v_log_f32 free path)
#   "cyl"    with the elliptic cylinder: 1.72e-3 at the source (300.5 degrees), 1.16e-4 for the tangent rays of the hop -- the float32
#            discriminant qb^2 - qa qc cancels for a grazing ray seen from 92 cm; the point moves ALONG its ray, in the background
# cap: 1 % of the case's smallest voxel pitch (4e-3 cm for "cyl" and "box", 6e-3 cm for "plain"), which is what holds "cyl".
# KNOWN LIMIT, not only a tolerance: on the cylinder route an error of the entry point below 4e-3 cm along the ray -- `target - 1e-4`
# for `target + 1e-4`, say -- passes these tests; the box route ("box": bound 4.8e-5 cm) is what catches it.  DESIGN.md, this file's row.
POSITION_F32_MEASURED_CM = {"plain": 4.3e-5, "box": 1.2e-5, "cyl": 1.72e-3}
POSITION_CAP_PITCH = 0.01


def direction_bound():
    return min(4.0 * DIRECTION_F32_MEASURED, DIRECTION_F32_CAP)


def position_bound(scene, name):
    return min(4.0 * POSITION_F32_MEASURED_CM[sc.CONTEXTS[name][0]], POSITION_CAP_PITCH * float(scene.voxel_size.min()))


class Rig:
    """The contexts of source_cases.CONTEXTS on the device, and every device run / replay the tests share."""

    def __init__(self, engine, root):
        self.ctx, self.scene, self.cold = {}, {}, {}
        for name in sc.CONTEXTS:
            ctx = engine.create(sc.build_input(name, root), device=0)
            self.ctx[name] = ctx
            self.cold[name] = so.cold(ctx)
            self.scene[name] = so.Scene(ctx, self.cold[name] if self.cold[name]["has_exterior"] and (ctx.geti("exterior_mode") & 2) else None)
        self.ids = sc.source_ids()
        self.runs, self.replays, self.tallies, self.hops = {}, {}, {}, {}

    def fan(self, name):
        return self.cold[name]["fan_lo"], self.cold[name]["fan_hi"]

    def source(self, mode, name, p):
        if (mode, name, p) not in self.runs:
            self.runs[mode, name, p] = self.ctx[name].kat_history(mode, "source", p, ids=self.ids, seed=sc.SEED)
        return self.runs[mode, name, p]

    def edge(self, mode, name, p):
        """The histories whose azimuth deviate sits at an end of the aperture (source_cases.EDGE_OFFSETS): where the cot clamp acts."""
        if ("edge", mode, name, p) not in self.runs:
            self.runs["edge", mode, name, p] = self.ctx[name].kat_history(mode, "source", p, ids=sc.edge_ids(p), seed=sc.SEED)
        return self.runs["edge", mode, name, p]

    def replay(self, mode, name, p):
        """The first REPLAY events restated, their entry from the direction this mode's kernel sampled."""
        if (mode, name, p) not in self.replays:
            d = self.source(mode, name, p)["d"][:sc.REPLAY]
            self.replays[mode, name, p] = sc.replay_source(self.scene[name], p, self.ids[:sc.REPLAY], self.fan(name), direction=d)
        return self.replays[mode, name, p]

    def tally(self, mode, name, p):
        if (mode, name, p) not in self.tallies:
            items = sc.tally_items(self.scene[name], p)
            flat = np.concatenate(list(items.values()))
            out = self.ctx[name].kat_history(mode, "tally", p, items=flat)
            res, at = {}, 0
            for block, v in items.items():
                res[block] = (v, {k: a[at:at + v.shape[0]] for k, a in out.items()})
                at += v.shape[0]
            self.tallies[mode, name, p] = res
        return self.tallies[mode, name, p]

    def hop(self, mode, name, p):
        if (mode, name, p) not in self.hops:
            res = {}
            for block, v in sc.hop_items(self.scene[name]).items():
                res[block] = (v, self.ctx[name].kat_history(mode, "hop", p, items=v, ids=sc.hop_ids(v.shape[0]), seed=sc.SEED))
            self.hops[mode, name, p] = res
        return self.hops[mode, name, p]

    def close(self):
        for ctx in self.ctx.values():
            ctx.close()


@pytest.fixture(scope="module")
def rig(engine, tmp_path_factory):
    r = Rig(engine, tmp_path_factory.mktemp("source_gpu"))
    yield r
    r.close()


def _unrotate(scene, p, d):
    """Directions of the pose frame back in the beam frame (rot_fan is orthonormal), float64."""
    d = np.asarray(d, dtype=np.float64)
    if int(scene.det[p]["rotation_flag"]) == 1:
        return d @ scene.src[p]["rot_fan"].astype(np.float64).reshape(3, 3)
    return d


# ======================================================================================================================================
# the contexts and the hook's refusals
# ======================================================================================================================================
def test_exposed_scalars_and_regions(rig):
    """fan_ratio_lo / hi recomputed in float64 from source_data by model_device.cpp's formula equal the exposed float32 values (to one
    float32 ulp: the host's cos / sin may differ from numpy's in the last place); the exposed object box and elliptic cylinder equal the
    restatement of mark_exterior_region from the host voxels; the three kinds of entry are all there."""
    for name, ctx in rig.ctx.items():
        s, c = rig.scene[name], rig.cold[name]
        lo, hi = s.fan_ratio()
        print(f"\n{name}: fan ratio {c['fan_lo']:.9g} {c['fan_hi']:.9g} restated {lo:.9g} {hi:.9g}; exterior mode {ctx.geti('exterior_mode')}, "
              f"cylinder {ctx.geti('exterior_cylinder')}, brick shift {ctx.geti('brick_shift')}, box {c['box_lo']} {c['box_hi']}, ellipse {c['ell_c']} {c['ell_inv']}")
        assert abs(float(c["fan_lo"]) - float(lo)) <= 2.0 ** -23 * abs(float(lo)) and abs(float(c["fan_hi"]) - float(hi)) <= 2.0 ** -23 * abs(float(hi))
        assert c["fan_lo"] < c["fan_hi"] and np.array_equal(c["bbox"], s.bbox)
        assert ctx.geti("brick_shift") == sc.BRICK_SHIFT
        want = so.object_region(ctx, sc.BRICK_SHIFT)
        geometry = sc.CONTEXTS[name][0]
        if geometry == "plain":
            assert want is None and c["has_exterior"] == 0 and ctx.geti("exterior_mode") == 0 and s.region is None
            continue
        assert (ctx.geti("exterior_mode") & 2) and c["has_exterior"] == 1 and ctx.geti("exterior_cylinder") == (1 if geometry == "cyl" else 0)
        assert np.array_equal(c["box_lo"], want["box_lo"]) and np.array_equal(c["box_hi"], want["box_hi"])
        assert c["ext_material"] == want["ext_material"] and c["ext_density"] == want["ext_density"] and c["ext_compact"] >= 0
        if geometry == "cyl":
            assert np.array_equal(c["ell_c"], want["ell_c"]) and np.allclose(c["ell_inv"], want["ell_inv"], rtol=1e-6, atol=0) and c["ell_inv"].min() > 0
        else:
            assert np.all(c["ell_inv"] == 0)


def test_the_hook_refuses_what_it_cannot_index(rig):
    """A projection outside the context, an energy outside the tables, a scatter state outside 0..3, a hop where there is no exterior:
    an error before any launch."""
    ctx, plain = rig.ctx["cyl"], rig.ctx["plain"]
    ok = np.array([[5.0, 5.0, 2.0, 0.0, 1.0, 0.0, 6.0e4, 0.0]], dtype=np.float32)
    ids = np.array([7], dtype=np.uint64)
    for p in (-1, 3):
        with pytest.raises(Exception, match="projection"):
            ctx.kat_history("fast", "source", p, ids=ids)
    for e in (100.0, 4.0e5, np.nan):
        bad = ok.copy()
        bad[0, 6] = e
        with pytest.raises(Exception, match="energy|number"):
            ctx.kat_history("fast", "hop", 1, items=bad, ids=ids)
    for state in (-1.0, 4.0, 1.5):
        bad = ok.copy()
        bad[0, 7] = state
        with pytest.raises(Exception, match="scatter state"):
            ctx.kat_history("fast", "tally", 1, items=bad)
    with pytest.raises(Exception, match="exterior"):
        plain.kat_history("fast", "hop", 1, items=ok, ids=ids)
    for kw in (dict(kind="source"), dict(kind="tally", ids=ids), dict(kind="hop", items=ok), dict(kind="walk", ids=ids), dict(kind="hop", items=ok, ids=np.arange(2, dtype=np.uint64))):
        with pytest.raises(ValueError):                                           # the binding names a missing or mismatched input itself
            ctx.kat_history("fast", kw.pop("kind"), 1, **kw)
    with pytest.raises(Exception, match="FAST"):
        ctx.kat_history("compat", "source", 1, ids=ids)
    assert ctx.kat_history("fast", "tally", 1, items=ok)["phase"][0] == so.PH_NEW       # and the context still works


# ======================================================================================================================================
# SOURCE
# ======================================================================================================================================
@pytest.mark.parametrize("name,p", sc.SOURCE_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_source_energy(rig, mode, name, p):
    """E and h.index are bit-equal to the float32 numpy evaluation of the rule on the replayed deviates (every step is one IEEE float32
    operation, the translation units are built without contraction), h.mfpW is the coarse majorant of that bin, h.scatter 0; over the
    whole launch, the spectrum bins against the probabilities the alias table encodes: chi-square at P_FALSE_ALARM."""
    s, dev, r = rig.scene[name], rig.source(mode, name, p), rig.replay(mode, name, p)
    n = sc.REPLAY
    same_e, same_i = int(np.sum(dev["e"][:n] == r["e"])), int(np.sum(dev["index"][:n] == r["index"]))
    bins = np.minimum(np.searchsorted(s.espc[:s.nbins + 1], dev["e"], side="right") - 1, s.nbins - 1)   # (E = the spectrum's last edge, by rounding)
    counts = np.bincount(bins, minlength=s.nbins).astype(np.float64)
    prob = so.alias_probabilities(s.cutoff, s.alias, s.nbins)
    # bins that expect fewer than 20 events are pooled into one (the spectrum's two ends)
    expected_all = prob * dev["e"].size
    big = expected_all >= 20.0
    expected = np.append(expected_all[big], expected_all[~big].sum())
    observed = np.append(counts[big], counts[~big].sum())
    chi2 = float(np.sum((observed - expected) ** 2 / expected))
    dof = expected.size - 1
    limit = float(stats.chi2.isf(P_FALSE_ALARM, dof))
    print(f"\nenergy {mode} {name} {p}: bit-equal E {same_e}/{n}, index {same_i}/{n}; bins chi2 {chi2:.1f}/{dof} (limit {limit:.1f}), "
          f"pooled bins {int(np.sum(~big))} expecting {expected[-1]:.1f} events, events in bins of probability 0: {int(counts[prob == 0].sum())}")
    assert same_e == n and same_i == n
    assert np.array_equal(dev["mfpw"][:n], s.wood_coarse[r["index"] >> 6]) and np.all(dev["scatter"] == 0)
    assert bins.min() >= 0 and counts[prob == 0].sum() == 0
    assert expected.min() >= 20.0 and dof >= 50 and chi2 < limit


@pytest.mark.parametrize("name,p", sc.SOURCE_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_source_direction(rig, mode, name, p):
    """The direction, undone to the beam frame in float64.  dz = cos_theta_low + xi D_cos_theta in float32: bit-equal in every pose
    (the poses of this suite turn the fan about z only: the third row of rot_fan is exactly 0, 0, 1, and 0 tx + 0 ty + 1 dz is dz).  dx, dy and |d| - 1 against the restatement: 4 x
    DIRECTION_F32_MEASURED, never above 1e-5.  The aperture, for EVERY event of the launch: unrotated, dx >= dy fan_ratio_lo and
    dx <= dy fan_ratio_hi as float32 comparisons; under a pose to 1e-6 after un-rotating; |dz / (dy + 1e-7)| <= max_height_at_y1cm
    (to the 2^-22 of the kernel's reciprocal and product; 1e-6 under a pose).  A launch holds no history near enough to an end of the
    aperture for the clamp to act: the histories of source_cases.EDGE_OFFSETS do, and are held the same way.  Events with an aperture ratio within 1e-5 of its bound are
    fragile (at most 0.5 %); trial counts and generator states are held by the entry tests below, which replay every deviate."""
    s, dev, r = rig.scene[name], rig.source(mode, name, p), rig.replay(mode, name, p)
    n = sc.REPLAY
    rotated = int(s.det[p]["rotation_flag"]) == 1
    beam = _unrotate(s, p, dev["d"])
    norm = np.abs(np.linalg.norm(dev["d"].astype(np.float64), axis=1) - 1.0)
    keep = r["dir"]["margin"] >= sc.FRAGILE_MARGIN
    share = 1.0 - float(keep.mean())
    dz_equal = int(np.sum(dev["d"][:n, 2][keep] == r["dir"]["dz32"][keep]))
    err = np.abs(beam[:n] - r["dir"]["beam"])[keep]
    lo, hi = rig.fan(name)
    mh = float(s.src[p]["max_height_at_y1cm"])
    ratio = np.abs(beam[:, 2] / (beam[:, 1] + 1.0e-7))
    if rotated:
        slack_lo = float(np.max(beam[:, 1] * float(lo) - beam[:, 0]))
        slack_hi = float(np.max(beam[:, 0] - beam[:, 1] * float(hi)))
    else:
        dx, dy = dev["d"][:, 0], dev["d"][:, 1]
        slack_lo, slack_hi = float(np.sum(~(dx >= dy * lo))), float(np.sum(~(dx <= dy * hi)))      # counts of float32 violations
    print(f"\ndirection {mode} {name} {p}: fragile {share:.2e}; dz bit-equal {dz_equal}/{int(keep.sum())}; beam-frame deviation dx {err[:, 0].max():.3e} "
          f"dy {err[:, 1].max():.3e} dz {err[:, 2].max():.3e}, | |d| - 1 | {norm.max():.3e} (bound {direction_bound():.3e}); aperture slack lo {slack_lo:.3e} "
          f"hi {slack_hi:.3e}, height ratio / bound - 1 {ratio.max() / mh - 1.0:.3e}; clamped {int(r['dir']['clamped'].sum())}, trials max {r['dir']['trials'].max()}")
    # the ends of the aperture: histories chosen for an azimuth deviate at an end of rng_f's range, where the clamp acts
    edge = rig.edge(mode, name, p)
    er = sc.replay_source(s, p, sc.edge_ids(p), (lo, hi))["dir"]
    eb = _unrotate(s, p, edge["d"])
    e_err = float(np.max(np.abs(eb - er["beam"])[er["margin"] >= sc.FRAGILE_MARGIN]))
    if rotated:
        e_lo, e_hi = float(np.max(eb[:, 1] * float(lo) - eb[:, 0])), float(np.max(eb[:, 0] - eb[:, 1] * float(hi)))
    else:
        e_lo, e_hi = float(np.sum(~(edge["d"][:, 0] >= edge["d"][:, 1] * lo))), float(np.sum(~(edge["d"][:, 0] <= edge["d"][:, 1] * hi)))
    on_bound = int(np.sum((edge["d"][:, 0] == edge["d"][:, 1] * lo) | (edge["d"][:, 0] == edge["d"][:, 1] * hi))) if not rotated else -1
    print(f"direction {mode} {name} {p}, {edge['d'].shape[0]} histories at the aperture's ends: restatement clamps {int(er['clamped'].sum())}, deviation {e_err:.3e}, "
          f"aperture slack lo {e_lo:.3e} hi {e_hi:.3e}, exactly on a bound {on_bound}")
    assert er["clamped"].sum() >= 8 and e_err <= direction_bound()
    assert (e_lo <= 1e-6 and e_hi <= 1e-6) if rotated else (e_lo == 0 and e_hi == 0 and on_bound >= 8)
    assert share <= FRAGILE_CAP
    assert not rotated or np.array_equal(s.src[p]["rot_fan"][6:], np.array([0, 0, 1], dtype=np.float32))    # (unrotated: rot_fan is not used)
    assert dz_equal == int(keep.sum())
    assert err.max() <= direction_bound() and norm.max() <= direction_bound()
    assert np.all(beam[:, 1] > 0)
    if rotated:
        assert slack_lo <= 1e-6 and slack_hi <= 1e-6 and ratio.max() <= mh * (1.0 + 1e-6)
    else:
        assert slack_lo == 0 and slack_hi == 0 and ratio.max() <= mh * (1.0 + 2.0 ** -22)


def _entry_fragile(s, r):
    if s.region is None:
        return (r["dir"]["margin"] < sc.FRAGILE_MARGIN) | (r["entry"]["margin"] < sc.BBOX_MARGIN_CM)
    return (r["dir"]["margin"] < sc.FRAGILE_MARGIN) | (r["entry"]["margin"] < sc.FRAGILE_MARGIN)


@pytest.mark.parametrize("name,p", [c for c in sc.SOURCE_CASES if sc.CONTEXTS[c[0]][0] == "plain"])
@pytest.mark.parametrize("mode", MODES)
def test_source_entry_without_exterior(rig, mode, name, p):
    """move_to_bbox: position and `miss` (phase ESCAPED, back at the focal spot to the position bound: like the reference the kernel
    steps forward and back in float32; else FLIGHT) against the restatement from the device's own direction; the position lies on the ray and, unless missed, inside the box; the generator state is the replay's
    (energy 2 deviates, 2 per trial, none for the entry)."""
    s, dev, r = rig.scene[name], rig.source(mode, name, p), rig.replay(mode, name, p)
    n = sc.REPLAY
    keep = ~_entry_fragile(s, r)
    miss = dev["phase"][:n] == so.PH_ESCAPED
    pos = dev["pos"][:n].astype(np.float64)
    err = np.abs(pos - r["entry"]["pos"]).max(axis=1)
    rel = pos - r["focal"]
    along = np.sum(rel * r["d32"], axis=1)
    off_ray = np.linalg.norm(rel - along[:, None] * r["d32"], axis=1)
    state_same = np.all(dev["state"][:n] == r["state"], axis=1)
    focal32 = s.src[p]["position"]
    print(f"\nentry {mode} {name} {p}: fragile {1 - keep.mean():.2e}, missed {miss.mean():.3f}; position deviation {err[keep].max():.3e} cm, off the ray "
          f"{off_ray.max():.3e} cm (bound {position_bound(s, name):.3e}); states differing {int(np.sum(~state_same & keep))}")
    assert 1.0 - keep.mean() <= FRAGILE_CAP
    assert np.all((dev["phase"] == so.PH_ESCAPED) | (dev["phase"] == so.PH_FLIGHT))
    assert np.array_equal(miss[keep], r["entry"]["miss"][keep]) and np.all(state_same[keep])
    assert np.max(np.abs(dev["pos"][dev["phase"] == so.PH_ESCAPED].astype(np.float64) - focal32.astype(np.float64))) <= position_bound(s, name)
    assert err[keep].max() <= position_bound(s, name) and off_ray.max() <= position_bound(s, name)
    inside = np.all((pos >= 0) & (pos <= s.bbox), axis=1)
    assert np.all(inside[~miss]) and np.all(along[~miss] > 0)


@pytest.mark.parametrize("name,p", [c for c in sc.SOURCE_CASES if sc.CONTEXTS[c[0]][0] != "plain"])
@pytest.mark.parametrize("mode", MODES)
def test_source_entry_with_exterior(rig, mode, name, p):
    """source_entry and classify_real: the phase (ESCAPED / FLIGHT / COMPTON / RAYLEIGH / ABSORBED), h.mc of an interaction and the final
    generator state equal the replay outside fragile events (at most 0.5 %) and outside the events the replay sends into
    entry_face_shell (reach <= 6e-5 |1 / cos|; counted, at most 0.1 %; test_fast_reproduces_the_entry_face_shell keeps that branch).
    FLIGHT photons stand at focal spot + (o_in + 1e-4) d, interacting ones at focal spot + s d (position bound), missed and
    through-going ones at the focal spot, bit for bit."""
    s, dev, r = rig.scene[name], rig.source(mode, name, p), rig.replay(mode, name, p)
    n = sc.REPLAY
    en = r["entry"]
    shell = en["shell"]
    keep = ~_entry_fragile(s, r) & ~shell
    ph = dev["phase"][:n]
    pos = dev["pos"][:n].astype(np.float64)
    err = np.abs(pos - en["pos"]).max(axis=1)
    state_same = np.all(dev["state"][:n] == r["state"], axis=1)
    focal32 = s.src[p]["position"]
    moved = keep & (ph != so.PH_ESCAPED)
    kinds = {k: int(np.sum(ph[keep] == v)) for k, v in (("escaped", so.PH_ESCAPED), ("flight", so.PH_FLIGHT), ("compton", so.PH_COMPTON),
                                                       ("rayleigh", so.PH_RAYLEIGH), ("absorbed", so.PH_ABSORBED))}
    print(f"\nentry {mode} {name} {p}: fragile {np.mean(_entry_fragile(s, r)):.2e}, shell candidates {shell.mean():.2e} ({int(shell.sum())}); {kinds}; phases differing "
          f"{int(np.sum((ph != en['phase']) & keep))}, states differing {int(np.sum(~state_same & keep))}; position deviation {err[moved].max():.3e} cm "
          f"(bound {position_bound(s, name):.3e}); differing among the left-out {int(np.sum((ph != en['phase']) & ~keep))}")
    assert np.mean(_entry_fragile(s, r)) <= FRAGILE_CAP and shell.mean() <= SHELL_CAP
    assert np.array_equal(ph[keep], en["phase"][keep]) and np.all(state_same[keep])
    real = keep & en["real"]
    assert real.sum() > 10 and np.all(dev["mc"][:n][real] == rig.cold[name]["ext_compact"])
    assert kinds["escaped"] > 1000 and kinds["flight"] > 1000
    assert np.all(dev["pos"][:n][keep & (ph == so.PH_ESCAPED)] == focal32)
    assert np.all(dev["pos"][dev["phase"] == so.PH_ESCAPED] == focal32)                   # the whole launch
    assert err[moved].max() <= position_bound(s, name)


@pytest.mark.parametrize("name,p", sc.SOURCE_CASES)
def test_source_is_one_text_in_both_arithmetics(rig, name, p):
    """The source functions carry no MC_FAST_F64 branch: `fast` and `fast64` hand out the same bits, word for word, over the launch."""
    a, b = rig.source("fast", name, p), rig.source("fast64", name, p)
    diff = {k: int(np.sum(a[k].view(np.uint32) != b[k].view(np.uint32))) if a[k].dtype == np.float32 else int(np.sum(a[k] != b[k])) for k in a}
    print(f"\nfast vs fast64 {name} {p}: differing words {diff}")
    assert not any(diff.values())


# ======================================================================================================================================
# TALLY
# ======================================================================================================================================
def _restated(s, p, v):
    return so.tally(s, p, v[:, :3], v[:, 3:6], v[:, 6], v[:, 7].astype(np.int64))


@pytest.mark.parametrize("name,p", sc.TALLY_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_tally_pixels(rig, mode, name, p):
    """Every pixel centre in each of the four scatter states: the exact word state * total_pixels + px + pz * nx, no event left out.
    Pixel edges at k +- 1e-3 .. 1e-6 pixel in xd and in zd: the exact word outside the block's margin (4 x source_cases.XD_F32_MEASURED, at most 1e-3
    pixel), inside it one of the two neighbouring pixels.  Borders and corners just inside and outside: a word, or -1.  Random events.
    The phase after the call is NEW."""
    s = rig.scene[name]
    run = rig.tally(mode, name, p)
    nx, total = int(s.det[p]["num_pixels"][0]), int(s.det[p]["total_num_pixels"])
    worst, f32_dev = {"aimed": 0.0, "reach": 0.0}, {"aimed": 0.0, "reach": 0.0}
    for block in ("centres", "edges_x", "edges_z", "borders", "random", "values", "reach"):
        v, out = run[block]
        r = _restated(s, p, v)
        x32, z32 = so.tally_f32(s, p, v[:, :3], v[:, 3:6])
        near = r["reaches"] & (np.abs(r["xd"]) < 200) & (np.abs(r["zd"]) < 200)
        kind, margin = ("reach" if block == "reach" else "aimed"), sc.tally_pixel_margin(block)
        f32_dev[kind] = max(f32_dev[kind], float(np.max(np.abs(x32 - r["xd"])[near], initial=0.0)), float(np.max(np.abs(z32 - r["zd"])[near], initial=0.0)))
        firm = (r["margin_pixel"] >= margin) & (r["margin_reach"] >= sc.FRAGILE_MARGIN * 0.025)
        differ = out["word"] != r["word"]
        worst[kind] = max(worst[kind], float(np.max(r["margin_pixel"][differ & (r["margin_reach"] >= sc.FRAGILE_MARGIN * 0.025)], initial=0.0)))
        # inside the margin: the word of a neighbour across the near boundary in x or in z (or none, across a border)
        state = v[:, 7].astype(np.int64)
        allowed = np.zeros(v.shape[0], dtype=bool)
        side_x, side_z = np.where(np.rint(r["xd"]) <= r["xd"], -1, 1), np.where(np.rint(r["zd"]) <= r["zd"], -1, 1)   # towards the near boundary
        for use_x in (False, True):
            for use_z in (False, True):
                px, pz = r["px"] + np.where(use_x, side_x, 0), r["pz"] + np.where(use_z, side_z, 0)
                ok_x = (not use_x) | (np.abs(r["xd"] - np.rint(r["xd"])) < margin)
                ok_z = (not use_z) | (np.abs(r["zd"] - np.rint(r["zd"])) < margin)
                inside = r["reaches"] & (px >= 0) & (px < nx) & (pz >= 0) & (pz < int(s.det[p]["num_pixels"][1]))
                allowed |= ok_x & ok_z & (out["word"] == np.where(inside, state * total + px + pz * nx, -1))
        print(f"\ntally {mode} {name} {p} {block}: {v.shape[0]} events, inside the margin {1 - firm.mean():.3f}, words differing {int(differ.sum())} "
              f"(outside the margin {int(np.sum(differ & firm))}), on the detector {np.mean(r['word'] >= 0):.3f}")
        assert np.all(out["phase"] == so.PH_NEW)
        assert np.array_equal(out["word"][firm], r["word"][firm])
        assert np.all(allowed[r["margin_reach"] >= sc.FRAGILE_MARGIN * 0.025])
        if block == "centres":
            assert firm.all() and np.array_equal(np.sort(out["word"]), np.arange(4 * total))
            assert np.array_equal(out["word"], state * total + r["px"] + r["pz"] * nx)
        if block in ("edges_x", "edges_z"):
            assert 0.45 < firm.mean() < 0.9                                 # the 1e-3 and 1e-4 offsets are firm, the 1e-5 and 1e-6 ones are not
            nominal = np.repeat(np.tile(np.array(sc.EDGE_DELTAS), 2), 3)        # the offset each event was aimed with (source_cases.tally_items)
            assert np.all(firm[np.tile(nominal, v.shape[0] // nominal.size) >= 1e-4])
        if block == "borders":
            assert firm.all() and 0.2 < np.mean(out["word"] < 0) < 0.8
    for kind, block in (("aimed", "centres"), ("reach", "reach")):
        print(f"\ntally {mode} {name} {p} {kind}: float32 cost of xd / zd on the host {f32_dev[kind]:.3e} pixel; largest margin of an event the device put in "
              f"another pixel {worst[kind]:.3e} pixel; margin {sc.tally_pixel_margin(block):.3e}")
        assert f32_dev[kind] <= sc.xd_measured(block) and worst[kind] < sc.tally_pixel_margin(block)


@pytest.mark.parametrize("name,p", sc.TALLY_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_tally_reach_and_value(rig, mode, name, p):
    """Reach: cosang on both sides of 0.025 (rotated poses) or v on both sides of 1e-4 (the unrotated one), and directions away from the
    detector: -1 below the threshold -- also where the harmless divisor of the straight-line code puts the point on the detector --
    and above it the word of the projected point.  Value: rint(float32(E) * float32(100)), ties to even, on exact ties and at the
    spectrum's two ends."""
    s = rig.scene[name]
    run = rig.tally(mode, name, p)
    v, out = run["reach"]
    r = _restated(s, p, v)
    firm = (r["margin_reach"] >= sc.FRAGILE_MARGIN * 0.025) & (r["margin_pixel"] >= sc.tally_pixel_margin("reach"))
    below = ~r["reaches"]
    x32, z32 = so.tally_f32(s, p, v[:, :3], v[:, 3:6])            # what the divisor 1 projects to
    nx, nz = (int(k) for k in s.det[p]["num_pixels"])
    decoy = below & (x32 >= 0) & (x32 < nx) & (z32 >= 0) & (z32 < nz)
    print(f"\nreach {mode} {name} {p}: {v.shape[0]} events, below the threshold {below.mean():.3f}, of them projected onto the detector by the divisor 1: "
          f"{int(decoy.sum())}; within 1e-5 of the threshold {int(np.sum(~firm))}; words differing {int(np.sum((out['word'] != r['word']) & firm))}")
    assert below.sum() > 1000 and (~below).sum() > 1000 and decoy.sum() >= 10
    assert np.all(out["word"][below & firm] == -1) and np.array_equal(out["word"][firm], r["word"][firm])
    for block in run:
        v, out = run[block]
        want = np.rint(v[:, 6] * np.float32(100.0)).astype(np.int64)
        assert np.array_equal(out["value"], want), block
    v, out = run["values"]
    ties = np.isin(v[:, 6], np.array(sc.TIES, dtype=np.float32))
    e100 = v[ties, 6].astype(np.float64) * 100.0
    print(f"values {mode} {name} {p}: ties {v[ties, 6].tolist()} -> {out['value'][ties].tolist()}; largest spectrum energy {float(s.espc[s.nbins])} -> "
          f"{int(out['value'][len(sc.TIES)])}")
    assert ties.sum() == len(sc.TIES) and np.all(e100 - np.floor(e100) == 0.5)
    assert np.array_equal(out["value"][ties], 2 * np.round(e100 / 2).astype(np.int64)) and np.all(out["value"][ties] % 2 == 0)
    assert np.any(out["value"][ties] == np.floor(e100)) and np.any(out["value"][ties] == np.floor(e100) + 1)
    assert v[len(sc.TIES), 6] == s.espc[s.nbins]


# ======================================================================================================================================
# HOP
# ======================================================================================================================================
@pytest.mark.parametrize("name,p", sc.HOP_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_exterior_hop(rig, mode, name, p):
    """exterior_record + exterior_hop + classify_real on designed rays -- through box and cylinder, through the box's corner regions past
    the cylinder, tangent within 1e-4 either side, along the cylinder's axis inside and outside it, missing the box through each face,
    from inside the cylinder's span but outside the box -- and on 2^16 random ones: phase, h.mc of an interaction, generator state and
    position against the restatement outside fragile events (at most 0.5 %).  An escaping photon keeps its position bit for bit.  Over the
    random rays the number interacting in the background against the sum of 1 - exp(-mu L): 5 standard deviations."""
    s = rig.scene[name]
    run = rig.hop(mode, name, p)
    for block, (v, out) in run.items():
        r = sc.replay_hop(s, p, v)
        keep = r["margin"] >= sc.FRAGILE_MARGIN
        pos = out["pos"].astype(np.float64)
        err = np.abs(pos - r["pos"]).max(axis=1)
        state_same = np.all(out["state"] == r["state"], axis=1)
        esc = out["phase"] == so.PH_ESCAPED
        kinds = {k: int(np.sum(out["phase"] == q)) for k, q in (("escaped", so.PH_ESCAPED), ("flight", so.PH_FLIGHT), ("compton", so.PH_COMPTON),
                                                                 ("rayleigh", so.PH_RAYLEIGH), ("absorbed", so.PH_ABSORBED))}
        print(f"\nhop {mode} {name} {p} {block}: {v.shape[0]} rays, fragile {1 - keep.mean():.2e}, {kinds}; phases differing {int(np.sum((out['phase'] != r['phase']) & keep))}, "
              f"states differing {int(np.sum(~state_same & keep))}; position deviation {err[keep].max():.3e} cm (bound {position_bound(s, name):.3e})")
        assert 1.0 - keep.mean() <= FRAGILE_CAP
        assert np.array_equal(out["phase"][keep], r["phase"][keep]) and np.all(state_same[keep])
        assert np.array_equal(out["index"], r["index"]) and np.all(out["e"] == v[:, 6]) and np.all(out["d"] == v[:, 3:6])
        assert np.all(out["pos"][esc] == v[esc, :3])
        assert err[keep].max() <= position_bound(s, name)
        real = keep & r["real"]
        assert np.all(out["mc"][real] == rig.cold[name]["ext_compact"])
        if block == "random":
            prob = 1.0 - np.exp(-r["mu"] * np.maximum(r["target"], 0.0))
            got = int(np.sum(np.isin(out["phase"], (so.PH_COMPTON, so.PH_RAYLEIGH, so.PH_ABSORBED))))
            sigma = float(np.sqrt(np.sum(prob * (1.0 - prob))))
            print(f"hop {mode} {name} {p}: interacting in the background {got}, expected {prob.sum():.1f} +- {sigma:.1f}")
            assert real.sum() >= 100 and abs(got - prob.sum()) <= 5.0 * sigma


@pytest.mark.parametrize("name,p", sc.HOP_CASES)
def test_exterior_hop_is_one_text_in_both_arithmetics(rig, name, p):
    """exterior_hop, cylinder_span and classify_real carry no MC_FAST_F64 branch: both arithmetics hand out the same bits."""
    a, b = rig.hop("fast", name, p), rig.hop("fast64", name, p)
    for block in a:
        for k in a[block][1]:
            x, y = a[block][1][k], b[block][1][k]
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), (block, k)
