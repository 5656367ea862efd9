"""CPU tests: the restatements of tests/source_ref.py against the CPU oracle (oracle_source, oracle_tally_image; tests/test_oracle_golden.py
pins the oracle to the reference build), the alias tables against the spectrum they encode, and the share of fragile events of every case
of tests/test_source_gpu.py -- before any GPU is involved.  tests/test_source_gpu.py then holds the HIP code to these restatements."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import parity
import source_cases as sc
import source_ref as so

FRAGILE_CAP, SHELL_CAP = 0.005, 0.001


@pytest.fixture(scope="module")
def scenes(engine, tmp_path_factory):
    out, ctxs = {}, []
    root = tmp_path_factory.mktemp("source_law")
    for name in sc.CONTEXTS:
        ctx = engine.create(sc.build_input(name, root), device=-1)
        ctxs.append(ctx)
        out[name] = (so.Scene(ctx, so.object_region(ctx, sc.BRICK_SHIFT)), parity.tables_from_context(ctx))
    yield out
    for ctx in ctxs:
        ctx.close()


def test_the_cases_cover_the_poses_and_the_three_entries(scenes):
    """One unrotated pose and two rotated ones (300.5 degrees: beyond 180); a displaced (half-fan) detector; one region with the elliptic
    cylinder, one with the box alone, one geometry without exterior; small enough to enumerate."""
    for name, (s, _) in scenes.items():
        assert [int(f) for f in s.det["rotation_flag"]] == ([1, 1, 1] if sc.CONTEXTS[name][1] else [0])
        assert float(s.det[0]["lateral_displacement"]) != 0.0
        assert tuple(int(v) for v in s.det[0]["num_pixels"]) == (64, 48)
    assert {scenes[c][0].det[p]["rotation_flag"] for c, p in sc.SOURCE_CASES} == {0, 1} == {scenes[c][0].det[p]["rotation_flag"] for c, p in sc.TALLY_CASES}
    assert sc.ANGLES[1] > 180.0 and ("cyl", 1) in sc.SOURCE_CASES and ("cyl", 1) in sc.TALLY_CASES
    cyl, box, plain = (scenes[k][0].region for k in ("cyl", "box", "plain"))
    assert scenes["cyl0"][0].region is not None and scenes["plain0"][0].region is None
    assert cyl is not None and cyl["ell_inv"][0] > 0 and cyl["ell_inv"][1] > 0
    assert box is not None and box["ell_inv"][0] == 0 and box["ell_inv"][1] == 0
    assert plain is None
    for r in (cyl, box):
        assert np.all(r["box_lo"] > 0) and np.all(r["box_hi"] < r["bbox"])          # exterior on every side
        assert r["ext_material"] == sc.cases.materials.material_number("air") - 1


def _ranecu_table(seed2, depth):
    lib = ol.oracle()
    probe = (C.c_int * 2)(seed2[0], seed2[1])
    return [float(lib.oracle_ranecu(probe)) for _ in range(depth)]


def _steps_between(before, after, limit):
    lib = ol.oracle()
    probe = (C.c_int * 2)(before[0], before[1])
    for k in range(limit + 1):
        if (probe[0], probe[1]) == (after[0], after[1]):
            return k
        lib.oracle_ranecu(probe)
    raise AssertionError("the oracle consumed more deviates than the table holds")


@pytest.mark.parametrize("name,p", [("plain0", 0), ("plain", 1), ("plain", 2)])
def test_source_is_the_oracles(scenes, name, p):
    """On RANECU deviates the restated energy, beam-frame direction (through the pose's rotation), trial count and bounding-box entry
    equal oracle_source (LIBM) to 1e-6 relative, and consume as many deviates.  The energy is bit-equal: it is the same float32 rule.
    The entry point is a float32 sum focal spot + step x direction in the oracle: its rounding is relative to those operands (the focal
    spot lies 92 cm from the volume), so the position's error is taken relative to the focal spot's distance."""
    s, T = scenes[name]
    lib = ol.oracle()
    n, depth = 4000, 64
    table = np.zeros((n, depth))
    want_e, want_d, want_p, want_flag, used = np.zeros(n, dtype=np.float32), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=int), np.zeros(n, dtype=int)
    seed = (C.c_int * 2)()
    lib.oracle_init_prng(5, 150, 4321, seed)
    for k in range(n):
        before = (seed[0], seed[1])
        table[k] = _ranecu_table(before, depth)
        pos, d, e, flag = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(), C.c_int()
        lib.oracle_source(C.byref(T.ct), p, seed, pos, d, C.byref(e), C.byref(flag), ol.MATH_LIBM)
        want_e[k], want_d[k], want_p[k], want_flag[k] = e.value, d[:], pos[:], flag.value
        used[k] = _steps_between(before, (seed[0], seed[1]), depth)
    dev = so.sr.ArrayDeviates(table)
    idx = np.arange(n)
    e, _, _, _ = so.source_energy(s, dev, idx)
    d = so.source_direction(s, p, dev, idx, fan=None)
    focal = np.broadcast_to(s.src[p]["position"].astype(np.float64), (n, 3))
    pos, miss, margin = so.move_to_bbox(focal, want_d, s.bbox)
    firm = (d["margin"] >= 1e-5) & (margin >= sc.BBOX_MARGIN_CM)
    assert firm.mean() > 0.99
    assert np.array_equal(e, want_e)
    assert np.array_equal(dev.drawn[firm], used[firm]) and np.array_equal(2 + 2 * d["trials"][firm], used[firm]) and d["trials"].max() > 1
    assert np.max(np.abs(d["d"] - want_d)[firm]) <= 1e-6
    assert np.array_equal(miss[firm], want_flag[firm] == -111) and 0.05 < miss.mean() < 0.95
    assert np.max(np.abs(pos - want_p)[firm]) / np.linalg.norm(focal[0]) <= 1e-6


@pytest.mark.parametrize("name,p", sc.TALLY_CASES)
def test_tally_is_the_oracles(scenes, name, p):
    """The restated word equals oracle_tally_image on every designed TALLY input whose detector coordinates are firmer than the device test's margin and
    whose reach test is firmer than 1e-5; no pixel centre is fragile.  The weight keeps the known deviation of FAST from COMPAT, asserted as
    what it is (below)."""
    s, T = scenes[name]
    for block, items in sc.tally_items(s, p).items():
        r = so.tally(s, p, items[:, :3], items[:, 3:6], items[:, 6], items[:, 7].astype(np.int64))
        word, weight = T.tally_events(p, items[:, :3], items[:, 3:6], items[:, 6], items[:, 7].astype(np.int32))
        firm = (r["margin_pixel"] >= sc.tally_pixel_margin(block)) & (r["margin_reach"] >= 1e-5 * 0.025)
        if block == "centres":
            assert firm.all() and np.all(r["word"] >= 0)
            assert np.array_equal(np.sort(r["word"]), np.arange(4 * int(s.det[p]["total_num_pixels"])))
        assert np.array_equal(r["word"][firm], word[firm]), (block, int(np.sum(r["word"][firm] != word[firm])))
        # the weight: COMPAT truncates the float32 sum E * 100 + 0.5, FAST rounds the float32 product E * 100 to nearest even.  They
        # differ on exact ties (the designed ones, and products that round to k + 1/2 between 2^22 and 2^23), and from 2^23 on (E >= 83.9 keV), where the sum's own rounding (ties to even) adds 1 to every odd product
        e100 = items[:, 6] * np.float32(100.0)
        assert e100.dtype == np.float32
        compat = (e100 + np.float32(0.5)).astype(np.int64)
        assert np.array_equal(weight.astype(np.int64), compat), block
        designed = np.isin(items[:, 6], np.array(sc.TIES, dtype=np.float32))
        tie = e100 - np.floor(e100) == np.float32(0.5)
        assert np.all(tie[designed])
        same = ~tie & (e100 < np.float32(2.0 ** 23))
        assert np.array_equal(r["value"][same], compat[same]), block
        big = e100 >= np.float32(2.0 ** 23)
        assert np.array_equal(r["value"][big], e100[big].astype(np.int64)) and np.array_equal(compat[big], r["value"][big] + (r["value"][big] & 1))
        if block == "values":
            assert designed.sum() == len(sc.TIES) and same.sum() > 100 and big.sum() > 100
        if tie.any():
            t100 = e100[tie].astype(np.float64)
            assert np.array_equal(compat[tie], np.floor(t100).astype(np.int64) + 1)                          # COMPAT: half up
            assert np.array_equal(r["value"][tie], 2 * np.round(t100 / 2).astype(np.int64))                  # FAST: half to even
        if block == "values":
            assert np.any(r["value"][tie] != compat[tie]) and np.any(r["value"][tie] == compat[tie])


def test_tally_value_at_0p125():
    """E = 0.125: E * 100 = 12.5 exactly; FAST scores 12, COMPAT 13."""
    assert np.float32(0.125) * np.float32(100.0) == np.float32(12.5)
    assert int(np.rint(np.float32(0.125) * np.float32(100.0))) == 12 and int(np.float32(12.5) + np.float32(0.5)) == 13


def test_alias_tables_encode_the_spectrum(scenes):
    """The bin probabilities rebuilt from espc_cutoff / espc_alias equal the spectrum file's normalised weights to 1e-6."""
    s, _ = scenes["plain"]
    rows = []
    for line in open(sc.cases.spectrum_file()):
        t = line.split("#")[0].split()
        if len(t) >= 2:
            rows.append((float(t[0]), float(t[1])))
            if float(t[1]) < 0:
                break
    w = np.array([r[1] for r in rows[:-1]])
    assert w.size == s.nbins and np.allclose([r[0] for r in rows], s.espc[:s.nbins + 1], rtol=1e-7)
    p = so.alias_probabilities(s.cutoff, s.alias, s.nbins)
    assert abs(p.sum() - 1.0) <= 1e-6
    assert np.max(np.abs(p - w / w.sum())) <= 1e-6
    assert np.all((s.alias[:s.nbins] >= 0) & (s.alias[:s.nbins] < s.nbins)) and np.all((s.cutoff[:s.nbins] >= 0) & (s.cutoff[:s.nbins] <= 1.0 + 1e-6))


def test_fan_ratio_restated(scenes):
    """cot at the two ends of the aperture, drawn in by 2e-6 of the range: lo < hi, and the aperture's own ends lie outside."""
    s, _ = scenes["plain"]
    lo, hi = s.fan_ratio()
    phi0, phi1 = float(s.src[0]["phi_low"]), float(s.src[0]["phi_low"]) + float(s.src[0]["D_phi"])
    assert 1.0 / np.tan(phi1) < lo < hi < 1.0 / np.tan(phi0)


@pytest.mark.parametrize("name,p", sc.SOURCE_CASES)
def test_fragile_share_of_the_source_cases(scenes, name, p):
    """For every SOURCE case of the device test: the share of replayed events whose rejection loop, entry or classification is closer to
    flipping than the margin stays under the cap of 0.5 %, and the share sent into the entry-face shell under 0.1 %.  From MwcDeviates
    alone: a cap never hides a failure of the device."""
    s, _ = scenes[name]
    r = sc.replay_source(s, p, sc.source_ids()[:sc.REPLAY], s.fan_ratio())
    assert float(np.mean(r["dir"]["margin"] < sc.FRAGILE_MARGIN)) <= FRAGILE_CAP
    if s.region is None:
        assert float(np.mean(r["entry"]["margin"] < sc.BBOX_MARGIN_CM)) <= FRAGILE_CAP
        assert 0.05 < r["entry"]["miss"].mean() < 0.95
    else:
        fragile = (r["dir"]["margin"] < sc.FRAGILE_MARGIN) | (r["entry"]["margin"] < sc.FRAGILE_MARGIN)
        assert float(np.mean(fragile)) <= FRAGILE_CAP, float(np.mean(fragile))
        assert float(np.mean(r["entry"]["shell"])) <= SHELL_CAP
        ph = r["entry"]["phase"]
        assert np.sum(ph == so.PH_FLIGHT) > 1000 and np.sum(ph == so.PH_ESCAPED) > 1000 and r["entry"]["real"].sum() > 10


@pytest.mark.parametrize("name,p", [("plain0", 0), ("plain", 1), ("plain", 2)])
def test_edge_ids_sit_at_the_ends_of_the_aperture(scenes, name, p):
    """The histories of source_cases.EDGE_OFFSETS draw an azimuth deviate at an end of rng_f's range; the restatement clamps the
    direction of those whose first trial is accepted: at both ends, several each."""
    s, _ = scenes[name]
    ids = sc.edge_ids(p)
    k = so.sr.fast_rng.streams_u32(ids, sc.SEED, p, 4)[:, 3] >> np.uint32(8)
    n_low = len(sc.EDGE_OFFSETS[p][0])
    assert np.all(k[:n_low] <= 3) and np.all(k[n_low:] >= (1 << 24) - 4)
    lo, hi = s.fan_ratio()
    free = sc.replay_source(s, p, ids, None)["dir"]
    r = sc.replay_source(s, p, ids, (lo, hi))["dir"]
    ratio = free["beam"][:, 0] / free["beam"][:, 1]
    assert np.sum(r["clamped"] & (ratio > float(hi))) >= 4 and np.sum(r["clamped"] & (ratio < float(lo))) >= 4
    assert np.all(r["beam"][:, 0] <= r["beam"][:, 1] * float(hi)) and np.all(r["beam"][:, 0] >= r["beam"][:, 1] * float(lo))


@pytest.mark.parametrize("name,p", sc.HOP_CASES)
def test_fragile_share_of_the_hop_cases(scenes, name, p):
    """The designed HOP rays and the random ones: fragile under 0.5 %, and every design reaches the branch it is written for."""
    s, _ = scenes[name]
    cyl = s.region["ell_inv"][0] > 0
    for block, items in sc.hop_items(s).items():
        r = sc.replay_hop(s, p, items)
        share = float(np.mean(r["margin"] < sc.FRAGILE_MARGIN))
        assert share <= FRAGILE_CAP, (block, share)
        flight, escaped = np.mean(r["phase"] == so.PH_FLIGHT), np.mean(r["phase"] == so.PH_ESCAPED)
        if block == "through":
            assert flight > 0.95
        if block == "corner" and cyl:
            assert escaped > 0.9                      # through the box, past the cylinder
        if block == "corner" and not cyl:
            assert flight > 0.9                       # the same rays enter the box
        if block == "tangent" and cyl:
            assert 0.4 < flight < 0.6         # the rays on the inner side enter, the ones on the outer side pass
        if block == "along" and cyl:
            assert 0.4 < flight < 0.6
        if block == "faces":
            assert escaped > 0.5 and flight > 0.05
        if block == "random":
            assert r["real"].sum() >= 100


@pytest.mark.parametrize("name,p", sc.TALLY_CASES)
def test_fragile_share_of_the_tally_cases(scenes, name, p):
    """Pixel centres are never fragile; of the random TALLY events fewer than 0.5 % lie within the margin of a pixel boundary.  (The edge
    blocks are fragile by design: they are held to "one of the two neighbours".)"""
    s, _ = scenes[name]
    items = sc.tally_items(s, p)
    for block in ("centres", "random", "values", "borders"):
        v = items[block]
        r = so.tally(s, p, v[:, :3], v[:, 3:6], v[:, 6], v[:, 7].astype(np.int64))
        share = float(np.mean(r["margin_pixel"] < sc.tally_pixel_margin(block)))
        assert share <= (0.0 if block == "centres" else FRAGILE_CAP), (block, share)
