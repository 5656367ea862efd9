"""The middle of a FAST history, the Woodcock flight step, event by event (run with -m gpu on an MI355X): csrc/kat_flight.inc runs
flight_locate, flight_steps (flight_locate + flight_resolve), real_record and classify_real -- the production functions themselves -- on
one item per thread, in both arithmetics (`fast`, `fast64`) and in all five kernel variants (u8, u8 with second-level codes, u8 with
tile records, u16, raw float2), from streams that oracle/fast_rng.py replays.  They are held to the restatement of tests/flight_ref.py,
which tests/test_flight_law.py pins to the CPU oracle.  Whole images cannot do this: a decode slip in a rare tile record reaches a few
voxels, a bracket that misses its cross section in one bin decides a sliver of deviates wrongly, and an index slip at a voxel face moves
counts between neighbouring voxels far below the noise.

Everything behind the position of a step is float32 with contraction off and is compared BIT FOR BIT, with no exclusion: voxel, `out`,
exterior, phase, material, the cached cross section, the generator state, the kind.  Only the position goes through the hardware's
logarithm: it is compared with the float64 restatement from the device's own previous position, under 4 x the largest deviation of the
float32 numpy run of the same formula over the same events, capped at 1 % of the smallest voxel pitch.

Measured on an MI355X (this file prints every figure before it asserts; DESIGN.md section 1, row of this file), over all cases and
both modes: the device's largest deviation of a position from the float64 restatement 4.85e-6 cm (thorax64, positions up to 51 cm), the
float32 numpy yardstick over the same events 4.08e-6 cm, the largest ratio of the two in one case 1.30 (graded_raw: 3.71e-6 against
2.86e-6 cm); bounds 9.9e-6 ... 1.6e-5 cm, far below the cap of 1 % of a voxel pitch (4e-3 cm and more)."""
import contextlib
import os

import numpy as np
import pytest

import cases
import flight_cases as fc
import flight_ref as fr
import source_ref as so

pytestmark = pytest.mark.gpu

MODES = ("fast", "fast64")
POSITION_CAP_PITCH = 0.01            # of tests/test_source_gpu.py
POSITION_FIGURES_CM = (4.85e-6, 4.08e-6, 1.30)   # device, yardstick, largest ratio: as measured (documentation; the bound is computed per run)
MIN_EVENTS = 1000
TRACE_STEPS = 16
# (name, case, second level, MCGPU_MAX_BRICKS, brackets) of every context; `designed` is tests/flight_cases.py's geometry
LOOKUP_CONFIGS = [(f"designed-{s}-{b}", "designed", s, b, True) for s in fc.SECOND_LEVEL for b in fc.MAX_BRICKS] + \
                 [(f"thorax64-{s}", "thorax64", s, None, True) for s in fc.SECOND_LEVEL] + \
                 [("graded_u16", "graded_u16", "off", None, True), ("graded_raw", "graded_raw", "off", None, True)]
TRACE_CONFIGS = [("designed-records-None", "designed", "records", None, True), ("designed-off-nobrackets", "designed", "off", None, False),
                 ("designed-codes-40", "designed", "codes", "40", True),
                 ("thorax64-records", "thorax64", "records", None, True), ("tissue22", "tissue22", "off", None, True),
                 ("tissue22-nobrackets", "tissue22", "off", None, False), ("cirs76", "cirs76", "off", None, True),
                 ("slab_angles", "slab_angles", "off", None, True), ("graded_u16", "graded_u16", "off", None, True),
                 ("graded_raw", "graded_raw", "off", None, True),
                 # exterior bricks in the grid, but the hop switched off in flight (MCGPU_EXTERIOR_MODE bit 0): a virtual step there stays FLIGHT
                 ("designed-records-sourcehop", "designed", "records", None, True)]
EXTRA_ENV = {"designed-records-sourcehop": {"MCGPU_EXTERIOR_MODE": "2"}}
CONFIG = {c[0]: c for c in LOOKUP_CONFIGS + TRACE_CONFIGS}


@contextlib.contextmanager
def knobs(second, max_bricks, brackets, extra=None):
    env = dict(fc.SECOND_LEVEL[second][0])
    env["MCGPU_EXTERIOR_MODE"] = None
    env.update(extra or {})
    env["MCGPU_MAX_BRICKS"] = max_bricks
    env["MCGPU_NO_BRACKETS"] = None if brackets else "1"
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Rig:
    """Contexts by configuration (built on first use, the knobs set only while the device model is built), their tables, and every
    device run / replay the tests share."""

    def __init__(self, engine, root):
        self.engine, self.root = engine, root
        self.inputs, self.ctxs, self.tabs, self.traces, self.replays, self.item_sets = {}, {}, {}, {}, {}, {}

    def ctx(self, name):
        if name not in self.ctxs:
            _, case, second, max_bricks, brackets = CONFIG[name]
            if case not in self.inputs:
                self.inputs[case] = fc.build_designed(self.root) if case == "designed" else cases.build_case(case, self.root / case)
            with knobs(second, max_bricks, brackets, EXTRA_ENV.get(name)):
                self.ctxs[name] = self.engine.create(self.inputs[case], device=0)
            self.tabs[name] = fr.Tables(self.ctxs[name], True)
        return self.ctxs[name]

    def tables(self, name) -> fr.Tables:
        self.ctx(name)
        return self.tabs[name]

    def items(self, name):
        """The start states of a configuration (flight_cases.flight_items) with the states the source leaves in flight, in one array."""
        if name not in self.item_sets:
            ctx, t = self.ctx(name), self.tables(name)
            src = ctx.kat_history("fast", "source", 0, ids=fc.FIRST_ID + (1 << 24) + np.arange(1 << 14, dtype=np.uint64), seed=fc.SEED)
            fl = src["phase"] == fr.PH_FLIGHT
            states = np.concatenate([src["pos"][fl], src["d"][fl], src["e"][fl][:, None]], axis=1)
            sets = fc.flight_items(t, source_states=states if fl.any() else None)
            items = np.concatenate(list(sets.values()))
            band, band_ids = fc.band_items(t)
            sizes = {k: v.shape[0] for k, v in sets.items()}
            sizes["band"] = band.shape[0]
            self.item_sets[name] = (np.concatenate([items, band]), sizes, np.concatenate([fc.flight_ids(items.shape[0]), band_ids]))
        return self.item_sets[name]

    def trace(self, mode, name, steps=TRACE_STEPS, items_of=None):
        """`items_of`: run the items and ids of that configuration (the same geometry under other knobs) instead of this one's."""
        key = (mode, name, steps, items_of)
        if key not in self.traces:
            items, _, ids = self.items(items_of or name)
            self.traces[key] = self.ctx(name).kat_flight(mode, "flight", 0, items, ids=ids, max_steps=steps, seed=fc.SEED)
        return self.traces[key]

    def replay(self, mode, name):
        """The restated trace from this mode's own positions.  Both arithmetics draw with rng_f (mapping "f32")."""
        if (mode, name) not in self.replays:
            items, _, ids = self.items(name)
            out = self.trace(mode, name)
            dev = fr.sr.MwcDeviates(ids, fc.SEED, 0, "f32")
            r = fr.replay(self.tables(name), items, dev, out["pos"], out["phase"], TRACE_STEPS)
            r["end_state"] = np.stack([dev.x, dev.c], axis=1)
            self.replays[mode, name] = r
        return self.replays[mode, name]

    def close(self):
        for ctx in self.ctxs.values():
            ctx.close()


@pytest.fixture(scope="module")
def rig(engine, tmp_path_factory):
    r = Rig(engine, tmp_path_factory.mktemp("flight_gpu"))
    yield r
    r.close()


# ======================================================================================================================================
# the tables the hook and the restatement read
# ======================================================================================================================================
def test_exposed_tables_are_the_host_builders(rig):
    """The downloads of what the kernel reads against the same tables built from the reference-layout host tables: mfp_tot rows (material-
    major, table_row), the compact numbering, the coarse Woodcock table by coarse_woodcock's rule; the designed geometry has its three
    bricks a side at the brick size the engine picks, an exterior, and every decode path in the records the DEVICE holds."""
    for name in ("designed-records-None", "thorax64-records", "tissue22", "graded_u16", "graded_raw"):
        t, ctx = rig.tables(name), rig.ctx(name)
        assert np.array_equal(t.compact_of, fr.host_compact_of(ctx)), name
        assert np.array_equal(t.tot.view(np.uint32), t.host_tot(t.compact_of).view(np.uint32)), name
        assert np.array_equal(t.wood.view(np.uint32), fr.coarse_woodcock(t.mfp_woodcock, t.e0, t.ide, t.nv).view(np.uint32)), name
        assert t.sig_shift >= 6 and t.sig_mid.shape == ((t.nv + (1 << t.sig_shift) - 1) >> t.sig_shift, t.nmat) and t.sig_w.shape[0] == t.sig_mid.shape[0]
    assert rig.tables("designed-off-nobrackets").sig_shift == -1
    t = rig.tables("designed-records-None")
    assert tuple(t.n) == fc.SHAPE and t.brick_shift == 2 and np.all(t.brick_n >= 3) and t.has_exterior & 1
    assert [rig.tables(f"designed-off-{b}").brick_shift for b in fc.MAX_BRICKS] == [2, 3, 4]
    rec = t.tile_records
    sub = (t.n + 3) >> 2
    rn = (sub + 1) >> 1
    tz, ty, tx = np.meshgrid(np.arange(sub[2]), np.arange(sub[1]), np.arange(sub[0]), indexing="ij")
    ri = ((((tx >> 1) + (ty >> 1) * rn[0] + (tz >> 1) * rn[0] * rn[1])) << 3) | ((tz & 1) << 2) | ((ty & 1) << 1) | (tx & 1)
    mixed = t.brick_code[tz, ty, tx] == fr.BRICK_MIXED                                  # bricks of 4^3 voxels: one tile each
    paths = fr.tile_paths(rec[ri[mixed]])
    counts = np.bincount(paths, minlength=4)
    print("designed: tiles of mixed bricks by decode path {two entries, r.y narrow, r.y wide, kTileAskVolume}:", counts,
          " exterior bricks:", int(np.sum(t.brick_code == fr.BRICK_EXTERIOR)))
    assert np.all(counts >= fc.MIN_TILES_PER_PATH)
    high = rec[ri[mixed]][:, 3] != 0
    assert np.all(np.bincount(paths[high], minlength=3)[:3] >= fc.MIN_TILES_PER_PATH)
    # the restated decoder on the device's records gives the voxel's palette entry (or asks the volume) for every voxel of those tiles
    pal = t.palette
    for z, y, x in zip(*np.nonzero(mixed)):
        r = rec[ri[z, y, x]]
        for b in range(64):
            ix, iy, iz = 4 * x + (b & 3), 4 * y + ((b >> 2) & 3), 4 * z + (b >> 4)
            if ix < t.n[0] and iy < t.n[1] and iz < t.n[2]:
                e = fr.decode_tile(r, b)
                if e >= 0:
                    assert pal[e, 0].view(np.uint32) == t.vox_density[iz, iy, ix].view(np.uint32) and int(pal[e, 1].view(np.int32)) == t.vox_mc[iz, iy, ix]


# ======================================================================================================================================
# lookup
# ======================================================================================================================================
def _outside_region(t, region, bx, by, bz):
    """Brick (bx, by, bz) lies wholly outside the object region (box AND elliptic cylinder), by source_ref.object_region's rule."""
    edge = 1 << t.brick_shift
    lo = np.stack([bx, by, bz], axis=1) * edge * t.voxel_size
    hi = np.minimum((np.stack([bx, by, bz], axis=1) + 1) * edge, t.n) * t.voxel_size
    off_box = np.any((hi <= region["box_lo"] + 1e-6) | (lo >= region["box_hi"] - 1e-6), axis=1)
    if region["ell_inv"][0] > 0:
        px = np.clip(region["ell_c"][0], lo[:, 0], hi[:, 0]) - region["ell_c"][0]
        py = np.clip(region["ell_c"][1], lo[:, 1], hi[:, 1]) - region["ell_c"][1]
        return off_box | (px * px * region["ell_inv"][0] + py * py * region["ell_inv"][1] > 1.001)
    return off_box


@pytest.mark.parametrize("mode", MODES)
def test_lookup_of_every_voxel_in_every_variant(rig, mode):
    """The centre of every voxel of the designed geometry (three second levels x three brick sizes), of thorax64 (three second levels)
    and of the u16 and raw volumes through LOOKUP: (density bits, compact material) equal the host voxels', with no tolerance and no
    exclusion; `exterior` is the brick's code being kBrickExterior, and the object region restated from the host voxels puts exactly
    those bricks outside; all five variants and three brick sizes were reached."""
    variants, shifts = set(), set()
    for name, case, second, max_bricks, _ in LOOKUP_CONFIGS:
        t, ctx = rig.tables(name), rig.ctx(name)
        pts, idx = fc.voxel_centres(t)
        got = ctx.kat_flight(mode, "lookup", 0, pts)
        ridx, out, _ = fr.locate(t, pts)
        assert np.array_equal(ridx, idx) and not out.any(), name
        dens, mc = fr.voxel(t, idx)
        bad = (got["density"].view(np.uint32) != dens.view(np.uint32)) | (got["mc"] != mc)
        assert not bad.any(), (name, int(bad.sum()), idx[bad][:5].tolist())
        assert not got["out"].any() and np.array_equal(got["exterior"], fr.exterior(t, idx)), name
        want = {"graded_u16": fr.VOL_U16, "graded_raw": fr.VOL_RAW}.get(case, fc.SECOND_LEVEL[second][1])
        assert np.all(got["variant"] == want) and ctx.geti("volume_kind") == (want if want < fr.VOL_U8_SUB else fr.VOL_U8), name
        assert ctx.geti("tile_records") == (1 if want == fr.VOL_U8_REC else 0) and (max_bricks is None or ctx.geti("brick_count") <= int(max_bricks))
        variants.add(want)
        if case == "designed":
            shifts.add(t.brick_shift)
        if t.volume_kind == fr.VOL_U8:
            bz, by, bx = np.meshgrid(*(np.arange(n) for n in t.brick_n[::-1]), indexing="ij")
            ext = (t.brick_code == fr.BRICK_EXTERIOR).reshape(-1)
            assert int(ext.sum()) == ctx.geti("bricks_exterior"), name
            if case == "designed":                                # (object_region wants a unique background: the designed geometry has one)
                region = so.object_region(ctx, t.brick_shift)
                if region is None:
                    assert not ext.any(), name
                else:
                    assert np.array_equal(_outside_region(t, region, bx.reshape(-1), by.reshape(-1), bz.reshape(-1)), ext), name
            if max_bricks is None:
                assert ext.any(), name
    assert variants == {fr.VOL_U8, fr.VOL_U16, fr.VOL_RAW, fr.VOL_U8_SUB, fr.VOL_U8_REC} and shifts == {2, 3, 4}


FACE_CONFIGS = ("designed-off-None", "designed-codes-40", "designed-records-None", "designed-records-6", "thorax64-records", "slab_angles", "graded_u16", "graded_raw")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FACE_CONFIGS)
def test_lookup_at_faces_clamps_and_outside(rig, mode, name):
    """For every axis, 0, kEps, every voxel face, bbox_hi and bbox at -2..+2 ulps, points outside and the eight corners: `out` and the
    looked-up voxel equal the restatement bit for bit -- the voxel of the CLAMPED position, which the restatement asserts to lie inside
    the grid whatever the point."""
    t, ctx = rig.tables(name), rig.ctx(name)
    pts = fc.face_points(t)
    got = ctx.kat_flight(mode, "lookup", 0, pts)
    idx, out, c = fr.locate(t, pts)
    assert np.all(idx >= 0) and np.all(idx < t.n) and np.all(c >= fr.K_EPS) and np.all(c <= t.bbox_hi)
    dens, mc = fr.voxel(t, idx)
    assert np.array_equal(got["out"], out), (name, pts[got["out"] != out][:5].tolist())
    bad = (got["density"].view(np.uint32) != dens.view(np.uint32)) | (got["mc"] != mc)
    assert not bad.any(), (name, int(bad.sum()), pts[bad][:5].tolist())
    assert np.array_equal(got["exterior"], fr.exterior(t, idx)), name
    assert out.any() and (~out).any() and np.unique(idx[:, 0]).size == t.n[0] and np.unique(idx[:, 1]).size == t.n[1] and np.unique(idx[:, 2]).size == t.n[2]


# ======================================================================================================================================
# properties of the tables, over every entry, in the kernel's float32
# ======================================================================================================================================
PROPERTY_CONFIGS = ("designed-records-None", "thorax64-records", "tissue22", "cirs76", "slab_angles", "graded_u16", "graded_raw")


def _all_bins(t):
    bins = np.arange(0, t.nv - 1)
    lo, hi = t.bin_energy_range(bins)
    return np.concatenate([bins, bins]), np.concatenate([lo, hi])


@pytest.mark.parametrize("name", PROPERTY_CONFIGS)
def test_brackets_contain_the_exact_cross_section(rig, name):
    """For every coarse bin, every compact material and every table bin of it, at the smallest and the largest float32 energy whose
    energy_index is that bin: fmaf(-mid, w, mid) <= fmaf(E, b, a) <= fmaf(mid, w, mid).  It follows (fma is monotonic) and is asserted at
    each material's largest density: p_lo <= p0 <= p_hi in float32, so the deviates next to p_lo and p_hi are decided as the exact test
    decides them."""
    t = rig.tables(name)
    bins, e = _all_bins(t)
    cb = bins >> t.sig_shift
    worst = []
    for mc in range(t.nmat):
        lo, hi = fr.bracket_bounds(t, cb, np.full(bins.size, mc))
        aux = fr.fma32(e, t.tot[mc, bins, 1], t.tot[mc, bins, 0])
        bad = ~((lo <= aux) & (aux <= hi))
        assert not bad.any(), (name, "material", int(t.material_of[mc]), "bins", bins[bad][:5].tolist(), "coarse", cb[bad][:5].tolist(),
                               lo[bad][:3], aux[bad][:3], hi[bad][:3])
        worst.append(float(np.min(np.minimum(aux - lo, hi - aux) / aux)))
        dmax = t.density_max[t.material_of[mc]]
        if dmax > 0:
            md = t.wood[bins >> fr.WOOD_SHIFT] * dmax
            p0, p_lo, p_hi = fr.fma32(-md, aux, np.float32(1)), fr.fma32(-md, hi, np.float32(1)), fr.fma32(-md, lo, np.float32(1))
            assert np.all(p_lo <= p0) and np.all(p0 <= p_hi), (name, mc)
            # the deviates next to the thresholds, through the restated step: settled decisions are the exact ones
            for xi, settled in ((np.nextafter(p_lo, np.float32(-1)), fr.BR_LO), (p_hi, fr.BR_HI)):
                n = bins.size
                ph, _, _, br, _, _, _ = fr.resolve(t, e, bins, t.wood[bins >> fr.WOOD_SHIFT], np.full(n, dmax, dtype=np.float32), np.full(n, mc), np.full(n, -1),
                                                   np.zeros(n, dtype=np.float32), xi, np.zeros(n, dtype=bool), np.zeros(n, dtype=bool))
                assert np.all(br == settled) and np.array_equal(ph == fr.PH_FLIGHT, xi < p0), (name, mc, settled)
    print(f"{name}: brackets of 2^{t.sig_shift} bins, {t.nmat} materials: smallest relative slack of a bound {min(worst):.3e}")


@pytest.mark.parametrize("name", PROPERTY_CONFIGS)
def test_coarse_majorant_keeps_the_probability_non_negative(rig, name):
    """For those energies and every material in the volume at its largest density: fmaf(-(wood[i >> kWoodShift] * dens), sigma, 1) >= 0 in
    float32, sigma = fmaf(E, b, a) -- the majorant is one in the arithmetic the kernel uses."""
    t = rig.tables(name)
    bins, e = _all_bins(t)
    present = np.unique(t.vox_material)
    smallest = []
    for m in present:
        mc = int(t.compact_of[m])
        dens = np.float32(max(float(t.density_max[m]), float(t.vox_density[t.vox_material == m].max())))
        sigma = fr.fma32(e, t.tot[mc, bins, 1], t.tot[mc, bins, 0])
        md = t.wood[bins >> fr.WOOD_SHIFT] * dens
        p = fr.fma32(-md, sigma, np.float32(1))
        bad = ~(p >= 0)
        assert not bad.any(), (name, "material", int(m), "density", float(dens), "bins", bins[bad][:8].tolist(), p[bad][:4])
        smallest.append(float(p.min()))
    print(f"{name}: smallest p0 over {present.size} materials x {t.nv - 1} bins x 2 energies: {min(smallest):.3e}")


# ======================================================================================================================================
# single steps and traces
# ======================================================================================================================================
def _position_figures(t, out, r):
    taken = r["taken"]
    dev = np.abs(out["pos"].astype(np.float64) - r["pos64"])[taken]
    ref = np.abs(r["pos32"].astype(np.float64) - r["pos64"])[taken]
    return float(dev.max()), float(ref.max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [c[0] for c in TRACE_CONFIGS])
def test_traces_step_by_step(rig, mode, name):
    """FLIGHT with max_steps 16 from the states the source leaves in flight, uniform points, energies at the coarse bins' edges, points at
    faces moving outward, points in exterior bricks moving both ways, and histories whose stream sends their first step to the exact
    table (flight_cases.band_items).  Every step is restated from the device's own previous position:
    the position within the bound above; h.mc, bits(h.aux), the phase, the generator state bit-equal for every event and step; after
    REAL the kind; steps taken, h.index and h.mfpW; rows of steps not taken are zero; HOP only where the geometry hops in flight."""
    t, out, r = rig.tables(name), rig.trace(mode, name), rig.replay(mode, name)
    items, sizes, _ = rig.items(name)
    taken = r["taken"]
    dev, ref = _position_figures(t, out, r)
    bound = min(4.0 * ref, POSITION_CAP_PITCH * float(t.voxel_size.min()))
    print(f"{name} {mode}: position: device {dev:.3e} cm, float32 numpy {ref:.3e} cm, ratio {dev / ref:.2f}; bound {bound:.3e} cm; item sets {sizes}")
    assert dev <= bound
    assert np.all(out["variant"] == {"graded_u16": fr.VOL_U16, "graded_raw": fr.VOL_RAW}.get(CONFIG[name][1], fc.SECOND_LEVEL[CONFIG[name][2]][1]))
    assert np.array_equal(out["steps"], r["steps"]) and np.array_equal(out["index"], r["index"])
    assert np.array_equal(out["mfpw"].view(np.uint32), r["mfpw"].view(np.uint32))
    for key in ("phase", "mc", "aux_bits"):
        bad = (out[key] != r[key]) & taken
        assert not bad.any(), (name, mode, key, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(out["state"][taken], r["state"][taken])                       # two deviates per step, no more, no fewer
    assert np.array_equal(out["final"], r["final"]) and np.array_equal(out["end_state"], r["end_state"])
    assert np.array_equal(out["mc_old"], r["mc_old"]) and np.sum(r["mc_old"] >= 0) >= MIN_EVENTS        # the cache is filled by the exact fetch, and only by it
    for key in ("phase", "mc", "aux_bits"):                                             # the steps after the last one stay zero
        assert not out[key][~taken].any()
    assert not out["pos"][~taken].any() and not out["state"][~taken].any()
    if not (t.has_exterior & 1):
        assert not np.any(out["phase"] == fr.PH_HOP)
    if name == "designed-records-sourcehop":                                            # ... although steps do end in exterior bricks
        assert t.has_exterior == 2 and "exterior" in sizes
        land = fr.exterior(t, fr.locate(t, out["pos"][taken])[0])
        assert np.sum(land & (out["phase"][taken] == fr.PH_FLIGHT)) >= MIN_EVENTS
    # the events behind the sums
    br, ph = r["branch"][taken], r["phase"][taken]
    counts = dict(p_lo=int(np.sum(br == fr.BR_LO)), p_hi=int(np.sum(br == fr.BR_HI)), exact=int(np.sum(br == fr.BR_EXACT)), cache=int(np.sum(br == fr.BR_CACHE)),
                  compton=int(np.sum(r["final"] == fr.PH_COMPTON)), rayleigh=int(np.sum(r["final"] == fr.PH_RAYLEIGH)),
                  absorbed=int(np.sum(r["final"] == fr.PH_ABSORBED)), hop=int(np.sum(ph == fr.PH_HOP)), escaped=int(np.sum(ph == fr.PH_ESCAPED)),
                  steps=int(taken.sum()))
    print(f"{name} {mode}: events {counts}")
    need = ["exact", "cache", "compton", "rayleigh", "absorbed", "escaped"] + (["p_lo", "p_hi"] if t.sig_shift >= 0 else []) + (["hop"] if t.has_exterior & 1 else [])
    assert all(counts[k] >= MIN_EVENTS for k in need), (name, {k: counts[k] for k in need})


@pytest.mark.parametrize("name", ["designed-records-None", "plain-slab", "thorax64-records"])
def test_source_states_carry_the_coarse_majorant(rig, name):
    """The states the traces start from are the ones start_history leaves in flight: their majorant is the coarse bin's,
    wood[index >> kWoodShift], bit for bit -- what the hook's own setup (and the restatement) assumes of every history that flies."""
    name = "slab_angles" if name == "plain-slab" else name
    ctx, t = rig.ctx(name), rig.tables(name)
    src = ctx.kat_history("fast", "source", 0, ids=fc.FIRST_ID + (1 << 24) + np.arange(1 << 14, dtype=np.uint64), seed=fc.SEED)
    assert np.array_equal(src["index"], t.energy_index(src["e"])) and np.unique(src["index"] >> fr.WOOD_SHIFT).size > 100
    assert np.array_equal(src["mfpw"].view(np.uint32), t.wood[src["index"] >> fr.WOOD_SHIFT].view(np.uint32))
    assert np.sum(src["phase"] == fr.PH_FLIGHT) >= MIN_EVENTS


@pytest.mark.parametrize("name", ["designed-records-None", "tissue22", "graded_raw"])
def test_fast_and_fast64_traces_are_bit_equal(rig, name):
    """The flight step has no double-precision part: the two arithmetics return the same words."""
    a, b = rig.trace("fast", name), rig.trace("fast64", name)
    for key in a:
        assert np.array_equal(a[key].view(np.uint32) if a[key].dtype == np.float32 else a[key], b[key].view(np.uint32) if b[key].dtype == np.float32 else b[key]), (name, key)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["designed-records-None", "tissue22"])
def test_single_steps_are_the_first_rows(rig, mode, name):
    """max_steps 1: the one row is the first row of the 16-step trace, the history is left where that step left it (a real interaction
    draws its kind at once), and one step was taken."""
    one, many = rig.trace(mode, name, 1), rig.trace(mode, name)
    for key in ("pos", "phase", "mc", "aux_bits", "state"):
        assert np.array_equal(one[key][:, 0].view(np.uint32) if one[key].dtype == np.float32 else one[key][:, 0],
                              many[key][:, 0].view(np.uint32) if many[key].dtype == np.float32 else many[key][:, 0]), key
    assert np.all(one["steps"] == 1)
    real = one["phase"][:, 0] == fr.PH_REAL
    assert np.array_equal(one["final"][~real], one["phase"][~real, 0]) and np.all(np.isin(one["final"][real], (fr.PH_COMPTON, fr.PH_RAYLEIGH, fr.PH_ABSORBED)))
    first_real = many["steps"] == 1
    assert np.array_equal(one["final"][first_real], many["final"][first_real]) and np.array_equal(one["end_state"][first_real], many["end_state"][first_real])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("on,off", [("designed-records-None", "designed-off-nobrackets"), ("tissue22", "tissue22-nobrackets")])
def test_brackets_on_and_off_decide_alike(rig, mode, on, off):
    """With and without the brackets the traces are bit-equal -- positions, phases, materials, generator states, kinds -- except
    bits(h.aux) on the steps the brackets settled, where it keeps the cached value; the restatement says which steps those are."""
    a, b, r = rig.trace(mode, on), rig.trace(mode, off, items_of=on), rig.replay(mode, on)
    for key in ("pos", "phase", "mc", "state", "final", "steps", "end_state", "index", "mfpw"):
        assert np.array_equal(a[key].view(np.uint32) if a[key].dtype == np.float32 else a[key], b[key].view(np.uint32) if b[key].dtype == np.float32 else b[key]), key
    settled = (r["branch"] == fr.BR_LO) | (r["branch"] == fr.BR_HI)
    assert settled.sum() >= MIN_EVENTS and np.array_equal(a["aux_bits"][~settled], b["aux_bits"][~settled])
    differ = a["aux_bits"] != b["aux_bits"]
    print(f"{on} {mode}: {int(settled.sum())} steps settled by the brackets, the cached value differs from the exact one on {int(differ.sum())}")
    assert differ.sum() >= MIN_EVENTS


# ======================================================================================================================================
# refusals
# ======================================================================================================================================
def test_refusals(rig, engine):
    """The entry point refuses its arguments before any HIP call: -1 for a count, a step count, a projection, a mode or a kind out of
    range; -2 for an input that is not a number, an energy outside the tables, a direction of length zero.  The context still works."""
    ctx = rig.ctx("designed-records-None")
    ok = np.array([[5.0, 4.0, 2.0, 0.0, 1.0, 0.0, 6.0e4]], dtype=np.float32)
    ids = np.array([7], dtype=np.uint64)

    def refused(code, match, *a, **kw):
        with pytest.raises(engine.EngineError, match=match) as err:
            ctx.kat_flight(*a, **kw)
        assert err.value.code == code

    for e in (100.0, 4.0e5):
        bad = ok.copy()
        bad[0, 6] = e
        refused(-2, "energy", "fast", "flight", 0, bad, ids=ids, max_steps=4)
    for col in range(7):
        for v in (np.nan, np.inf):
            bad = ok.copy()
            bad[0, col] = v
            refused(-2, "number", "fast", "flight", 0, bad, ids=ids, max_steps=4)
    bad = ok.copy()
    bad[0, 0] = np.nan
    refused(-2, "number", "fast", "lookup", 0, bad[:, :3])
    bad = ok.copy()
    bad[0, 3:6] = 0.0
    refused(-2, "direction", "fast64", "flight", 0, bad, ids=ids, max_steps=4)
    for steps in (0, -1, 33):
        refused(-1, "step count", "fast", "flight", 0, ok, ids=ids, max_steps=steps)
    for p in (-1, 1):
        refused(-1, "projection", "fast", "flight", p, ok, ids=ids, max_steps=4)
    refused(-1, "FAST", "compat", "flight", 0, ok, ids=ids, max_steps=4)
    n = (1 << 20) + 1
    refused(-1, "bad argument", "fast", "lookup", 0, np.broadcast_to(ok[:, :3], (n, 3)))
    n = (1 << 18) + 1
    refused(-1, "step count", "fast", "flight", 0, np.broadcast_to(ok, (n, 7)), ids=np.arange(n, dtype=np.uint64), max_steps=16)
    with pytest.raises(ValueError):
        ctx.kat_flight("fast", "walk", 0, ok, ids=ids)
    with pytest.raises(ValueError):
        ctx.kat_flight("fast", "flight", 0, ok)
    out = ctx.kat_flight("fast", "flight", 0, ok, ids=ids, max_steps=4, seed=fc.SEED)
    assert 1 <= out["steps"][0] <= 4 and out["variant"][0] == fr.VOL_U8_REC
