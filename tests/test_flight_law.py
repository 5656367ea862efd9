"""CPU tests: the restatement of the Woodcock flight step (tests/flight_ref.py) against the CPU oracle (oracle_flight_many: track_batch's
Woodcock loop and interaction draw from given states; tests/test_oracle_golden.py pins the oracle to the reference build), its table row
and record layout against the reference-layout host tables, its float32 fused multiply-add against exact rational arithmetic, and the
designed geometry's tile classes -- before any GPU is involved.  tests/test_flight_gpu.py then holds the HIP code to the restatement.

The oracle and the FAST kernels draw the same law from different deviates: the oracle takes the reference's majorant a + E b of the
table bin and decides real-or-virtual AND the kind on one deviate r (cumulative thresholds p0, p0 + md s_Co, p0 + md (s_Co + s_Ra)); the
kernels take the coarse bin's majorant and draw the kind from a second deviate xi against s_Co / s_tot.  Both are fed here: flight_ref.walk
gets the oracle's majorant and its deviates, flight_ref.classify gets xi = (r - p0) / (1 - p0), the deviate that makes the two tests the
same inequality."""
import ctypes as C

import numpy as np
import pytest

import cases
import flight_cases as fc
import flight_ref as fr
import oracle_lib as ol
import parity

FRAGILE_CAP = 0.005              # of tests/test_source_gpu.py
FACE_MARGIN_CM = 1e-5            # a float64 position nearer than this to a voxel face (or the kEps shell) may index another voxel in float32
DEVIATE_MARGIN = 1e-6            # a deviate nearer than this to a threshold may decide the other way in float32
LAW_CASES = ("designed", "thorax64", "slab_angles", "tissue22", "graded_u16")
N_EVENTS, MAX_STEPS = 6000, 8


@pytest.fixture(scope="module")
def contexts(engine, tmp_path_factory):
    root = tmp_path_factory.mktemp("flight_law")
    out, ctxs = {}, []
    for name in LAW_CASES:
        ctx = engine.create(fc.build_designed(root) if name == "designed" else cases.build_case(name, root / name), device=-1)
        ctxs.append(ctx)
        out[name] = (fr.Tables(ctx, False), parity.tables_from_context(ctx), ctx)
    yield out
    for ctx in ctxs:
        ctx.close()


def test_fma32_is_one_rounding():
    """The float64 emulation of fmaf against exact rational arithmetic: random operands, and operands built so that a * b + c lies on
    and next to the midpoint of two float32 (where rounding the float64 sum a second time goes wrong)."""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.uniform(-2, 2, 4000).astype(np.float32)
    b = rng.uniform(-2, 2, 4000).astype(np.float32)
    c = (rng.uniform(-2, 2, 4000) * 10.0 ** rng.integers(-6, 2, 4000)).astype(np.float32)
    # ties: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is exactly the midpoint of two float32 (spacing 2^-23 there); a c far below the float64
    # ulp puts the true sum just off it, where the float64 sum still is the midpoint and rounds to even
    ta = np.full(6, 1 + 2.0 ** -12, dtype=np.float32)
    tb = np.full(6, 1 + 2.0 ** -12, dtype=np.float32)
    tc = np.array([0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -80, -2.0 ** -80, 2.0 ** -149], dtype=np.float32)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = fr.fma32(a, b, c)
    for i in range(a.size):
        want = fr._round_fraction_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i].view(np.uint32) == want.view(np.uint32), (i, a[i], b[i], c[i])
    # the double rounding is real: without the exact path at least one designed tie rounds the other way
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert np.any(naive[-6:] != got[-6:])


def test_table_row_and_record_layout(contexts):
    """flight_ref's rows are the kernel's: mfp_tot[compact material, bin] = {a_tot, b_tot} of mfp_a / mfp_b at [bin, material], the record of
    classify_real its six numbers, the compact numbering the used materials in order, the coarse majorant coarse_woodcock's rule."""
    for name, (t, _, ctx) in contexts.items():
        used = np.nonzero(t.compact_of >= 0)[0]
        assert np.array_equal(t.compact_of[used], np.arange(used.size)) and np.array_equal(t.material_of, used) and t.nmat == used.size
        assert set(np.unique(t.vox_material)) <= set(used) and np.all(t.vox_mc >= 0)
        rng = np.random.default_rng(2)
        idx, mc = rng.integers(0, t.nv - 1, 500), rng.integers(0, t.nmat, 500)
        a_tot, a_co, a_ra, b_tot, b_co, b_ra = t.record(idx, mc)
        A, B = ctx.host_table("mfp_a", "<f4").reshape(-1, 3), ctx.host_table("mfp_b", "<f4").reshape(-1, 3)
        row = idx * fr.MAXMAT + used[mc]                          # the reference's row: bin-major, material number - 1
        assert np.array_equal(np.stack([a_tot, a_co, a_ra], 1), A[row]) and np.array_equal(np.stack([b_tot, b_co, b_ra], 1), B[row])
        assert np.array_equal(t.tot[mc, idx, 0], A[row, 0]) and np.array_equal(t.tot[mc, idx, 1], B[row, 0])
        assert np.array_equal(t.wood.view(np.uint32), fr.coarse_woodcock(t.mfp_woodcock, t.e0, t.ide, t.nv).view(np.uint32)), name
        for k in range(3):                                        # make_args' upper clamp indexes the last voxel, one ulp more does not (or leaves the shell)
            assert int(np.float32(t.bbox_hi[k] * t.inv_vs[k])) == t.n[k] - 1 and t.bbox_hi[k] <= np.float32(t.bbox[k] - fr.K_EPS)


def test_designed_geometry_has_every_tile_class(contexts, engine):
    """37 x 22 x 13 voxels in the engine's frame, seven (material, density) pairs, tiles of 1, 2, 3, 4 and 5 or more entries with and
    without a majority, minority voxels in both mask words: at least MIN_TILES_PER_PATH tiles per decode path of flight_locate, by the
    host's encoder (the device test repeats the count on the records the device holds), and the restated decoder reads every voxel back."""
    t = contexts["designed"][0]
    assert tuple(t.n) == fc.SHAPE and all(n % 4 != 0 and n >= 12 for n in fc.SHAPE)
    pairs = np.unique(np.stack([t.vox_material, t.vox_density.view(np.int32)], -1).reshape(-1, 2), axis=0, return_inverse=True)
    assert pairs[0].shape[0] == len(fc.PAIRS) >= 6
    code = pairs[1].reshape(t.n[2], t.n[1], t.n[0])
    sub = (t.n + 3) >> 2
    tiles = np.full((sub[2], sub[1], sub[0], 4, 4, 4), -1, dtype=np.int16)
    for z in range(t.n[2]):
        for y in range(t.n[1]):
            tiles[z >> 2, y >> 2, np.arange(t.n[0]) >> 2, z & 3, y & 3, np.arange(t.n[0]) & 3] = code[z, y]
    tiles = tiles.reshape(-1, 64)
    rec = engine.kat_tile_records(tiles)
    entries = np.array([np.unique(v[v >= 0]).size for v in tiles])
    paths = fr.tile_paths(rec)[entries > 1]
    print("tiles by entries 1..6:", np.bincount(entries, minlength=7)[1:], " by decode path {two, narrow, wide, ask}:", np.bincount(paths, minlength=4))
    assert np.all(np.bincount(paths, minlength=4) >= fc.MIN_TILES_PER_PATH)
    assert all(np.sum(entries == k) >= 5 for k in (1, 2, 3, 4)) and np.sum(entries >= 5) >= 5
    high = (rec[:, 3] != 0) & (entries > 1)
    assert np.all(np.bincount(fr.tile_paths(rec)[high], minlength=3)[:3] >= fc.MIN_TILES_PER_PATH)      # minority voxels in the high mask word
    for v, r in zip(tiles, rec):
        for b in np.nonzero(v >= 0)[0]:
            assert fr.decode_tile(r, int(b)) in (-1, int(v[b]))


def _ranecu_pairs(seeds):
    """The next two RANECU floats of each stream (the seeds are not advanced)."""
    lib = ol.oracle()
    out = np.zeros((seeds.shape[0], 2))
    for k in range(seeds.shape[0]):
        probe = (C.c_int * 2)(int(seeds[k, 0]), int(seeds[k, 1]))
        out[k, 0] = float(lib.oracle_ranecu(probe))
        out[k, 1] = float(lib.oracle_ranecu(probe))
    return out


@pytest.mark.parametrize("name", LAW_CASES)
def test_flight_is_the_oracles(contexts, name):
    """From uniform points, isotropic directions and energies across the spectrum, up to MAX_STEPS Woodcock steps one at a time, each from
    the oracle's own float32 position and with the oracle's deviates: the restated voxel, escape and real-or-virtual decision equal the
    oracle's for every step whose float64 position is further than 1e-5 cm from a voxel face and whose deviate is further than 1e-6 from
    p0; the restated kind (classify_real fed the deviate that makes its test the oracle's) equals the oracle's outside a deviate margin
    of 1e-6.  Both excluded shares are printed and lie below 0.5 %."""
    t, T, _ = contexts[name]
    lib = ol.oracle()
    rng = np.random.default_rng(2026)
    n = N_EVENTS
    e = rng.uniform(1.2e4, 1.2e5, n)
    b = np.floor((e - float(t.e0)) * float(t.ide))
    e = (float(t.e0) + (b + rng.uniform(0.05, 0.95, n)) / float(t.ide)).astype(np.float32)        # off the table bins' borders
    state = np.concatenate([rng.uniform(0.01, 0.99, (n, 3)) * t.bbox.astype(np.float64), fc.isotropic(rng, n), e[:, None]], axis=1).astype(np.float32)
    seeds = np.zeros((n, 2), dtype=np.int32)
    for k in range(n):                                                    # one leap-frogged stream per event
        s = (C.c_int * 2)()
        lib.oracle_init_prng(k, 150, 4321, s)
        seeds[k] = s[0], s[1]
    index = t.energy_index(e)
    wt = np.asarray(t.mfp_woodcock, dtype=np.float32).reshape(-1, 2)
    mfpw = wt[index, 0] + e * wt[index, 1]                                # the oracle's majorant, in its float32
    assert mfpw.dtype == np.float32
    active = np.arange(n)
    events = face_out = dev_out = kind_events = kind_out = 0
    kinds = np.zeros(5, dtype=np.int64)
    for _ in range(MAX_STEPS):
        if active.size == 0:
            break
        table = _ranecu_pairs(seeds[active])
        pos, vox, kind, steps, seeds[active] = T.flight_events(state[active], seeds[active], 1)
        assert np.all(steps == 1)
        w = fr.walk(t, state[active, :3], state[active, 3:6], e[active], mfpw[active], fr.sr.ArrayDeviates(table), 1)
        firm = (w["face"] >= FACE_MARGIN_CM) & (w["margin"] >= DEVIATE_MARGIN)
        events += active.size
        face_out += int(np.sum(w["face"] < FACE_MARGIN_CM))
        dev_out += int(np.sum((w["face"] >= FACE_MARGIN_CM) & (w["margin"] < DEVIATE_MARGIN)))
        want_status = np.where(kind == 3, fr.PH_ESCAPED, np.where(kind == 0, fr.PH_FLIGHT, fr.PH_REAL))
        assert np.array_equal(w["status"][firm], want_status[firm]), name
        inside = firm & (want_status != fr.PH_ESCAPED)
        flat = w["voxel"][:, 0] + w["voxel"][:, 1] * t.n[0] + w["voxel"][:, 2] * t.n[0] * t.n[1]
        assert np.array_equal(flat[inside], vox[inside]) and np.all(vox[firm & (want_status == fr.PH_ESCAPED)] == -1)
        assert np.max(np.abs(w["pos"] - pos)[firm]) <= 1e-5                # the oracle's float32 step against the float64 one
        real = np.nonzero(firm & (want_status == fr.PH_REAL))[0]
        if real.size:
            xi = (w["xi"][real] - w["p0"][real]) / (1.0 - w["p0"][real])
            got, margin = fr.classify(t, e[active][real], index[active][real], w["mc"][real], xi.astype(np.float32))
            firm_kind = margin * (1.0 - w["p0"][real]) >= DEVIATE_MARGIN   # the margin in units of the oracle's deviate
            kind_events += real.size
            kind_out += int(np.sum(~firm_kind))
            assert np.array_equal(got[firm_kind], kind[real][firm_kind]), name
            kinds += np.bincount(kind[real], minlength=5)
        go = want_status == fr.PH_FLIGHT
        state[active[go], :3] = pos[go]
        active = active[go]
    share_face, share_dev, share_kind = face_out / events, dev_out / events, kind_out / max(kind_events, 1)
    print(f"{name}: {events} steps, {kind_events} interactions {dict(compton=int(kinds[1]), rayleigh=int(kinds[2]), absorbed=int(kinds[4]))}; "
          f"excluded: {share_face:.5f} within {FACE_MARGIN_CM} cm of a face, {share_dev:.5f} + {share_kind:.5f} (kind) within {DEVIATE_MARGIN} of a threshold")
    assert events > n + n // 2 and kind_events > n // 4 and np.all(kinds[[1, 2, 4]] >= 50)
    assert share_face < FRAGILE_CAP and share_dev + share_kind < FRAGILE_CAP
