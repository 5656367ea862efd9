"""The cases of the flight-step tests (tests/test_flight_law.py on the CPU, tests/test_flight_gpu.py on the device): a designed u8
geometry whose 4^3 tiles take every decode path of flight_locate, the existing cases of tests/cases.py, the knobs that select the five
kernel variants, three brick sizes and the brackets, and the start states of the LOOKUP and FLIGHT kinds of mcgpu_kat_flight.

  designed   37 x 22 x 13 voxels of 4 mm (no axis a multiple of 4 voxels or of a brick edge; at least three 4^3 bricks a side), seven
             (material, density) pairs.  A margin of one brick of air in x and y becomes exterior bricks; inside it the tiles rotate
             through six classes: one entry (a homogeneous brick that is not background), two entries, three with a majority (`r.y`
             narrow), four with a majority (`r.y` wide), three without a majority and five or more (both kTileAskVolume).  Minority voxels
             are drawn over all 64 positions, so they sit in both mask words; the last z layer of tiles is one voxel thick (padding:
             its records are built from 16 voxels and take whatever class those leave)."""
from __future__ import annotations

import numpy as np

import cases
import flight_ref as fr

SEED = 20261
FIRST_ID = (1 << 34) + 97531    # ids beyond 32 bits: the high counter word of the stream takes part
SHAPE, PITCH_MM = (37, 22, 13), 4.0
MIN_TILES_PER_PATH = 20
# (material, density): air is the background (and the exterior); the rest fills the tiles
PAIRS = [("air", 0.0013), ("h2o", 1.0), ("adipose", 0.95), ("bone_050", 1.4), ("bone_100", 1.92), ("h2o", 0.3), ("soft_tissue", 1.06)]
EXISTING = ("thorax64", "tissue22", "cirs76", "slab_angles", "graded_u16", "graded_raw")
# knob settings -> the kernel variant they select on a u8 volume
SECOND_LEVEL = {"off": ({"MCGPU_SUB_BRICKS": "0", "MCGPU_TILE_RECORDS": "0"}, fr.VOL_U8),
                "codes": ({"MCGPU_SUB_BRICKS": "1", "MCGPU_TILE_RECORDS": "0"}, fr.VOL_U8_SUB),
                "records": ({"MCGPU_SUB_BRICKS": "0", "MCGPU_TILE_RECORDS": "1"}, fr.VOL_U8_REC)}
MAX_BRICKS = (None, "40", "6")   # designed: bricks of 4^3 (10 x 6 x 4), 8^3 (5 x 3 x 2) and 16^3 (3 x 2 x 1) voxels


def designed_geometry():
    rng = np.random.default_rng(37)
    # the voxel file holds the geometry's arrays turned by rot90(k=3) in the x/y plane (geometry.py: mcgpu_arrays): the tiles are laid out
    # in the ENGINE's frame (SHAPE) and turned back at the end
    g = cases.geometry.MCBoxGeometry(shape=(SHAPE[1], SHAPE[0], SHAPE[2]), image_spacing=(PITCH_MM,) * 3, material="air")
    number = [cases.materials.material_number(m) for m, _ in PAIRS]
    dens = [d for _, d in PAIRS]
    entry = np.zeros(SHAPE, dtype=np.int64)                      # index into PAIRS per voxel, [x, y, z]
    count = 0
    for tz in range(4):                                          # z 0..12: tz = 3 is one voxel thick
        for ty in range(1, 5):                                   # y 4..19: ty = 0 and ty = 5 (y 20, 21) stay air
            for tx in range(1, 9):                               # x 4..35: tx = 0 and tx = 9 (x 36) stay air
                k = (1, 2, 3, 4, 1, 2, 3, 5)[count % 8] if tz < 3 else (0, 1, 2, 3, 5)[count % 5]
                count += 1
                v = np.zeros(64, dtype=np.int64)
                others = rng.permutation(np.arange(1, len(PAIRS)))
                if k == 0:                                       # one entry, not the background: a homogeneous coded brick
                    v[:] = others[0]
                elif k == 1:                                     # two entries, any split
                    v[:] = others[0]
                    v[rng.random(64) < rng.uniform(0.1, 0.9)] = others[1]
                    v[int(rng.integers(0, 16))] = others[1]
                elif k == 2:                                     # three with a majority: at most 30 minority voxels, one selector bit each
                    v[:] = others[0]
                    m = rng.choice(64, size=int(rng.integers(4, 31)), replace=False)
                    v[m] = rng.choice(others[1:3], size=m.size)
                    v[m[0]], v[m[1]] = others[1], others[2]
                elif k == 3:                                     # four with a majority: at most 15 minority voxels, two selector bits each
                    v[:] = others[0]
                    m = rng.choice(64, size=int(rng.integers(6, 16)), replace=False)
                    v[m] = rng.choice(others[1:4], size=m.size)
                    v[m[0]], v[m[1]], v[m[2]] = others[1], others[2], others[3]
                elif k == 4:                                     # three without a majority the record can hold (more than 30 others)
                    v[:] = np.resize(others[:3], 64)[rng.permutation(64)]
                else:                                            # five and more
                    v[:] = rng.choice(others[:int(rng.integers(5, 7))], size=64)
                    v[rng.permutation(64)[:5]] = others[:5]
                blk = v.reshape(4, 4, 4).transpose(2, 1, 0)      # [iz, iy, ix] -> [x, y, z]
                sx, sy, sz = slice(4 * tx, 4 * tx + 4), slice(4 * ty, 4 * ty + 4), slice(4 * tz, min(4 * tz + 4, SHAPE[2]))
                entry[sx, sy, sz] = blk[:, :, :sz.stop - sz.start]
    g.materials[:] = np.rot90(np.array(number)[entry], k=1, axes=(0, 1))
    g.densities[:] = np.rot90(np.array(dens, dtype=np.float32)[entry], k=1, axes=(0, 1))
    assert np.array_equal(g.mcgpu_arrays()[0], np.array(number)[entry])
    return g


def build_designed(out_dir):
    sim = cases.simulation.MCSimulation(designed_geometry(), cases.material_files(), cases.spectrum_file(), n_projections=1, n_histories=1000,
                                        **cases.SMALL_DET)
    return sim.prepare_simulation(out_dir / "designed")


def voxel_centres(t: fr.Tables):
    """The centre of every voxel, float32[n, 3], x fastest -- and its index."""
    iz, iy, ix = np.meshgrid(np.arange(t.n[2]), np.arange(t.n[1]), np.arange(t.n[0]), indexing="ij")
    idx = np.stack([ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)], axis=1)
    return ((idx + 0.5) * t.voxel_size).astype(np.float32), idx


def ulps_around(v, k=2):
    """The float32 values from -k to +k ulps around each entry."""
    out = [np.asarray(v, dtype=np.float32)]
    lo = hi = out[0]
    for _ in range(k):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.unique(np.concatenate(out))


def face_points(t: fr.Tables):
    """For every axis: 0, kEps, every voxel face, bbox_hi and bbox at -2..+2 ulps (the other two coordinates at three interior values
    off every face), points outside the volume on each side, and the eight corners at -2..+2 ulps on every axis together."""
    rng = np.random.default_rng(5)
    pts = []
    inner = [np.array([0.37, 0.5, 0.81]) * float(t.bbox[a]) + 0.0123 for a in range(3)]
    for a in range(3):
        faces = (np.arange(t.n[a] + 1) * t.voxel_size[a]).astype(np.float32)
        faces = np.concatenate([faces, (np.arange(t.n[a] + 1).astype(np.float32) / t.inv_vs[a]).astype(np.float32)])
        special = np.array([0.0, fr.K_EPS, t.bbox_hi[a], t.bbox[a], t.bbox[a] - fr.K_EPS], dtype=np.float32)
        vals = ulps_around(np.concatenate([faces, special]))
        vals = np.concatenate([vals, np.array([-1.0, -1e-3, -1e-7, float(t.bbox[a]) + 1e-3, float(t.bbox[a]) + 5.0, 1e6, -1e6], dtype=np.float32)])
        for j in range(3):
            p = np.zeros((vals.size, 3), dtype=np.float32)
            for b in range(3):
                p[:, b] = vals if b == a else np.float32(inner[b][(j + b) % 3])
            pts.append(p)
    lo = ulps_around(np.array([0.0, fr.K_EPS], dtype=np.float32))
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                ends = [ulps_around(np.array([t.bbox_hi[a], t.bbox[a]], dtype=np.float32)) if c else lo for a, c in enumerate((cx, cy, cz))]
                m = min(e.size for e in ends)
                pts.append(np.stack([e[:m] for e in ends], axis=1))
                pts.append(np.stack([rng.permutation(e)[:m] for e in ends], axis=1))
    return np.concatenate(pts).astype(np.float32)


def isotropic(rng, n):
    w = rng.uniform(-1, 1, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - w * w)
    return np.stack([s * np.cos(phi), s * np.sin(phi), w], axis=1)


def edge_energies(t: fr.Tables, lo_ev, hi_ev):
    """Energies within 2 ulps of every multiple of 2^kWoodShift and 2^sig_shift table bins inside [lo_ev, hi_ev]."""
    shifts = {fr.WOOD_SHIFT} | ({t.sig_shift} if t.sig_shift >= 0 else set())
    bins = np.unique(np.concatenate([np.arange(0, t.nv - 1, 1 << s) for s in shifts]))
    e = (float(t.e0) + bins / float(t.ide)).astype(np.float32)
    e = ulps_around(e[(e > lo_ev) & (e < hi_ev)])
    return e


def flight_items(t: fr.Tables, n_random=44000, espc=(1.5e4, 1.2e5), source_states=None):
    """name -> float32[n, 7] {x, y, z, u, v, w, E}: uniform points with isotropic directions and energies over the spectrum, the coarse
    bins' edges, points at faces moving outward, points in exterior bricks moving both ways, and (given) the states a source left in
    flight.  Together at most 2^16 items."""
    rng = np.random.default_rng(11)
    bbox = t.bbox.astype(np.float64)
    out = {}

    def pack(pos, d, e):
        pos, d = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
        e = np.broadcast_to(np.asarray(e, dtype=np.float64), (pos.shape[0],))
        return np.concatenate([pos, d / np.linalg.norm(d, axis=1, keepdims=True), e[:, None]], axis=1).astype(np.float32)

    out["uniform"] = pack(rng.uniform(0.001, 0.999, (n_random, 3)) * bbox, isotropic(rng, n_random), rng.uniform(*espc, n_random))
    e = edge_energies(t, *espc)
    e = e[rng.permutation(e.size)[:min(e.size, 1 << 12)]]
    out["bin_edges"] = pack(rng.uniform(0.05, 0.95, (e.size, 3)) * bbox, isotropic(rng, e.size), e)
    m = 1 << 11                                                   # at a face, moving outward through it (and a little sideways)
    axis, side = rng.integers(0, 3, m), rng.integers(0, 2, m)
    pos = rng.uniform(0.02, 0.98, (m, 3)) * bbox
    depth = rng.choice([2e-5, 1e-4, 1e-3, 1e-2, 0.1], m)
    pos[np.arange(m), axis] = np.where(side == 1, bbox[axis] - depth, depth)
    d = 0.3 * rng.normal(size=(m, 3))
    d[np.arange(m), axis] = np.where(side == 1, 1.0, -1.0)
    out["outward"] = pack(pos, d, rng.uniform(*espc, m))
    if t.device and t.volume_kind == fr.VOL_U8 and (t.brick_code == fr.BRICK_EXTERIOR).any():
        bz, by, bx = np.nonzero(t.brick_code == fr.BRICK_EXTERIOR)
        m = 1 << 12
        pick = rng.integers(0, bx.size, m)
        edge = float(1 << t.brick_shift)
        lo = np.stack([bx[pick], by[pick], bz[pick]], axis=1) * edge * t.voxel_size
        pos = np.minimum(lo + rng.uniform(0.05, 0.95, (m, 3)) * edge * t.voxel_size, bbox * 0.9999)
        centre = 0.5 * bbox
        inward = centre - pos + rng.normal(size=(m, 3))
        d = np.where((np.arange(m) % 2 == 0)[:, None], inward, -inward)
        out["exterior"] = pack(pos, d, rng.uniform(*espc, m))
    if source_states is not None:
        out["source"] = np.asarray(source_states, dtype=np.float32)[:1 << 12, :7]
    assert sum(v.shape[0] for v in out.values()) <= (1 << 16) - BAND_ITEMS
    return out


def flight_ids(n):
    return FIRST_ID + np.arange(n, dtype=np.uint64)


BAND_ITEMS, BAND_POOL = 1 << 12, 1 << 21


def band_items(t: fr.Tables):
    """Histories chosen by their stream: (items float32[n, 7], ids).  The band [p_lo, p_hi) in which the brackets leave a step to the
    exact table holds a few deviates in a thousand, and only an exact fetch fills the cache a same-material hit needs: 2^16 histories
    of 16 steps meet both too rarely to count on.  So these start at the centre of a voxel of the denser half, with a direction of
    length 1e-4 (the hook takes any direction that is not zero: the history stays in its voxel for all its steps), under the ids, out of
    a pool of 2^21, whose SECOND deviate -- the first step's test -- falls into the band of that voxel's material at the item's energy.
    The first step then asks the exact table; the steps after it, while virtual, are cache hits.  Without brackets every first step
    asks the table: the first BAND_ITEMS of the pool."""
    rng = np.random.default_rng(23)
    n = BAND_POOL if t.sig_shift >= 0 else BAND_ITEMS
    flat = np.nonzero(t.vox_density.reshape(-1) >= np.median(t.vox_density))[0]
    pick = flat[rng.integers(0, flat.size, n)]
    idx = np.stack([pick % t.n[0], (pick // t.n[0]) % t.n[1], pick // (t.n[0] * t.n[1])], axis=1)
    e = rng.uniform(1.5e4, 1.2e5, n).astype(np.float32)
    ids = FIRST_ID + (1 << 28) + np.arange(n, dtype=np.uint64)
    keep = np.arange(n)
    if t.sig_shift >= 0:
        dev = fr.sr.MwcDeviates(ids, SEED, 0, "f32")
        dev.next(keep)                                            # the step's own deviate
        xi = dev.next(keep).astype(np.float32)
        dens, mc = fr.voxel(t, idx)
        index = t.energy_index(e)
        md = t.wood[index >> fr.WOOD_SHIFT] * dens
        lo, hi = fr.bracket_bounds(t, index >> t.sig_shift, mc)
        p_lo, p_hi = fr.fma32(-md, hi, np.float32(1)), fr.fma32(-md, lo, np.float32(1))
        keep = np.nonzero((xi >= p_lo) & (xi < p_hi))[0][:BAND_ITEMS]
    d = isotropic(rng, keep.size) * 1.0e-4
    items = np.concatenate([(idx[keep] + 0.5) * t.voxel_size, d, e[keep, None].astype(np.float64)], axis=1).astype(np.float32)
    return items, ids[keep]
