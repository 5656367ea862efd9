"""The cases of the source / entry / tally tests (tests/test_source_law.py on the CPU, tests/test_source_gpu.py on the device): three
small geometries under three poses, and the designed inputs of the TALLY and HOP kinds of mcgpu_kat_history.

  cyl    an elliptic water body with a bone insert in air: homogeneous exterior, object region = box AND elliptic cylinder
  box    a rectangular water block with a bone insert in air: homogeneous exterior, no cylinder (it would trim nothing off the box)
  plain  a uniform water block: no exterior, the source's photons enter through move_to_bbox

Poses (tests/cases.py, slab_angles): 270, 300.5 (beyond 180) and 45.25 degrees, all with rotation_flag 1; the contexts "cyl0" and "plain0"
hold the same geometries under the single default projection, the only one the engine (like the reference) gives rotation_flag 0.
The detector is the reference's half-fan one (displaced by -159.856 mm) at 64 x 48 pixels, so that a test can enumerate every pixel."""
from __future__ import annotations

import numpy as np

import cases
import source_ref as so

ANGLES = [270.0, 300.5, 45.25]
DET = dict(n_detector_pixels=(64, 48), detector_size=(717.024, 297.984))
CONTEXTS = {"cyl": ("cyl", True), "cyl0": ("cyl", False), "box": ("box", True), "plain": ("plain", True), "plain0": ("plain", False)}
# (context, projection) of the SOURCE and TALLY kinds; HOP runs on "cyl" and "box" under projection 1
SOURCE_CASES = [("cyl0", 0), ("cyl", 1), ("cyl", 2), ("box", 1), ("plain0", 0), ("plain", 1), ("plain", 2)]
TALLY_CASES = [("plain0", 0), ("cyl", 1), ("cyl", 2)]
HOP_CASES = [("cyl", 1), ("box", 1)]
BRICK_SHIFT = 2                 # bricks of 4^3 voxels: what the engine chooses for volumes this small (asserted on the device)
SEED = 20251
FIRST_ID = (1 << 33) + 54321    # ids beyond 32 bits: the high counter word of the stream takes part
LAUNCH, REPLAY = 1 << 18, 1 << 16
FRAGILE_MARGIN = 1e-5           # relative margin of a decision below which another arithmetic may take it differently
BBOX_MARGIN_CM = 1e-4           # move_to_bbox: distance of the entry point from a face on the axes it did not enter through
# detector coordinates xd / zd [pixels]: largest deviation of their float32 evaluation from float64 over the designed TALLY events of
# every case (source_ref.tally_f32) -- 1.48e-5 for the blocks of rays aimed at the detector, 6.9e-5 for the grazing rays of the "reach"
# block that still come within 200 pixels of it.  The margin of a block is 4 x its figure, at most 1e-3 pixel: 6e-5 for the aimed
# blocks, so that the edge offsets of 1e-3 AND 1e-4 pixel are held to the exact word.  On the MI355X no event outside its margin took
# another pixel (largest margin of one that did: 8.4e-6; tests/test_source_gpu.py prints both figures).
XD_F32_MEASURED = {"aimed": 1.5e-5, "reach": 7.0e-5}
XD_F32_CAP = 1.0e-3


def xd_measured(block: str) -> float:
    return XD_F32_MEASURED["reach" if block == "reach" else "aimed"]


def tally_pixel_margin(block: str) -> float:
    return min(4.0 * xd_measured(block), XD_F32_CAP)


def _body(kind):
    """72 x 56 x 16 voxels of 4 mm: large enough against the 4^3-voxel bricks that the elliptic cylinder trims 5 % of the box's bricks (the
    engine keeps it only then), thin enough to stay at 6e4 voxels."""
    g = cases.geometry.MCBoxGeometry(shape=(72, 56, 16), image_spacing=(4.0, 4.0, 4.0), material="air")
    x, y = np.meshgrid(np.arange(72) + 0.5, np.arange(56) + 0.5, indexing="ij")
    if kind == "cyl":
        inside = ((x - 36.0) / 29.5) ** 2 + ((y - 28.0) / 21.5) ** 2 <= 1.0
    else:
        inside = (np.abs(x - 36.0) < 28.0) & (np.abs(y - 28.0) < 20.0)
    g.materials[:, :, 4:12][inside] = cases.materials.material_number("h2o")
    g.densities[:, :, 4:12][inside] = 1.0
    g.materials[30:38, 24:32, 6:10] = cases.materials.material_number("bone_050")
    g.densities[30:38, 24:32, 6:10] = 1.4
    return g


def build_input(name: str, out_dir):
    geometry, posed = CONTEXTS[name]
    kw = dict(projection_angles=ANGLES, n_histories=1000, **DET) if posed else dict(n_projections=1, n_histories=1000, **DET)
    if geometry == "plain":
        g = cases.geometry.MCBoxGeometry(shape=(32, 28, 20), image_spacing=(6.0, 6.0, 6.0), material="h2o")
    else:
        g = _body(geometry)
    return cases.simulation.MCSimulation(g, cases.material_files(), cases.spectrum_file(), **kw).prepare_simulation(out_dir / name)


def source_ids():
    return FIRST_ID + np.arange(LAUNCH, dtype=np.uint64)


# Histories whose first azimuth deviate (the fourth of the stream) is one of the four smallest or four largest values rng_f hands out:
# phi rounds to an END of the aperture [phi_low, phi_low + D_phi], where cot(phi) lies outside [fan_ratio_lo, fan_ratio_hi] and the
# FAST kernels' clamp acts.  One history in 2e6 is such a one, a launch of 2^18 holds none: these offsets (from FIRST_ID + LAUNCH, per
# projection = stream key) were found by search_edge_ids(), and tests/test_source_law.py checks what they claim.
EDGE_OFFSETS = {
    0: ([9517676, 16796675, 17000336, 17781940, 17937279, 19359720, 21545540, 25973532, 27081052, 32635712],
        [4544644, 6350225, 8989559, 10171343, 16078553, 19773612, 26560442]),
    1: ([165814, 274651, 1066052, 5311457, 9883956, 12426048, 13991919, 21248443, 24119341, 28921905, 29874932],
        [1767845, 6651742, 12744867, 15188392, 15747696, 17644122, 28777309, 30439826, 30788097]),
    2: ([9550040, 13794398, 14886657, 17594219, 19826407, 24758168, 28810901],
        [2629035, 10545175, 14118942, 14242107, 15097923, 16417826, 17352315, 25325971, 26335510]),
}


def edge_ids(p: int):
    low, high = EDGE_OFFSETS[p]
    return FIRST_ID + LAUNCH + np.array(low + high, dtype=np.uint64)


def search_edge_ids(p: int, span: int = 1 << 25, chunk: int = 1 << 21):
    """(offsets with the deviate at the low end, at the high end) among `span` ids behind the launch's: 8 s per projection."""
    low, high = [], []
    for c in range(0, span, chunk):
        k = so.sr.fast_rng.streams_u32(FIRST_ID + LAUNCH + c + np.arange(chunk, dtype=np.uint64), SEED, p, 4)[:, 3] >> np.uint32(8)
        low += (c + np.nonzero(k <= 3)[0]).tolist()
        high += (c + np.nonzero(k >= (1 << 24) - 4)[0]).tolist()
    return low, high


def replay_source(sc: so.Scene, p: int, ids, fan, mapping="f32", direction=None):
    """The restated start_history of the first ids: energy, direction, then the entry (with the scene's region: source_entry, else
    move_to_bbox).  The source functions carry no double-precision branch: both arithmetics draw with rng_f (mapping "f32").
    `direction`: the float32 directions the device sampled, to restate the entry from what the kernel held (the device test: the
    direction has its own test); None: the restated ones, rounded to float32."""
    dev = so.sr.MwcDeviates(ids, SEED, p, mapping)
    idx = np.arange(len(ids))
    e, b, index, ip = so.source_energy(sc, dev, idx)
    d = so.source_direction(sc, p, dev, idx, fan)
    focal = np.broadcast_to(sc.src[p]["position"].astype(np.float64), (len(ids), 3))
    d32 = (d["d"] if direction is None else np.asarray(direction)).astype(np.float32).astype(np.float64)
    out = dict(e=e, bin=b, index=index, dir=d, focal=focal, d32=d32)
    if sc.region is not None:
        mfpw = sc.wood_coarse[index >> 6]
        out["entry"] = so.exterior_entry(sc, focal, d32, e.astype(np.float64), index, dev, idx, True, mfpw)
        out["mfpw"] = mfpw
    else:
        pos, miss, margin = so.move_to_bbox(focal, d32, sc.bbox)
        out["entry"] = dict(pos=pos, miss=miss, margin=margin)
    out["state"] = np.stack([dev.x, dev.c], axis=1)
    out["drawn"] = dev.drawn.copy()
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# TALLY: designed events.  Every block aims rays from points inside the volume at chosen detector coordinates (pixels from the lower
# corner), in float64; the kernel and the restatement then both see the float32 roundings of position and direction.
# ----------------------------------------------------------------------------------------------------------------------------------
TIES = (0.125, 0.375, 2.625, 1000.125, 20000.625, 60000.875)     # E * 100 is exactly k + 1/2 in float32: k even, odd, ...
EDGE_DELTAS = (1e-3, 1e-4, 1e-5, 1e-6)


def _starts(sc, n, rng):
    return (0.1 + 0.8 * rng.random((n, 3))) * sc.bbox


def _aimed(sc, p, xd, zd, rng, state=None, energy=None):
    xd, zd = np.broadcast_arrays(np.asarray(xd, dtype=np.float64), np.asarray(zd, dtype=np.float64))
    xd, zd = xd.reshape(-1), zd.reshape(-1)
    start = _starts(sc, xd.size, rng)
    d = so.detector_point(sc, p, xd, zd) - start
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = rng.uniform(float(sc.espc[0]), float(sc.espc[sc.nbins]), xd.size) if energy is None else np.broadcast_to(energy, (xd.size,))
    s = rng.integers(0, 4, xd.size) if state is None else np.broadcast_to(state, (xd.size,))
    return np.concatenate([start, d, e[:, None], s[:, None].astype(np.float64)], axis=1).astype(np.float32)


def tally_items(sc: so.Scene, p: int) -> dict:
    """name -> float32[n, 8] {x, y, z, u, v, w, E, scatter state}; together fewer than 2^16 items."""
    rng = np.random.default_rng(100 + p)
    nx, nz = (int(v) for v in sc.det[p]["num_pixels"])
    px, pz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    out = {}
    out["centres"] = np.concatenate([_aimed(sc, p, px + 0.5, pz + 0.5, rng, state=s) for s in range(4)])
    sign = np.array([-1.0, 1.0])
    off = (sign[:, None] * np.array(EDGE_DELTAS)[None, :]).reshape(-1)
    ex = (np.arange(nx + 1)[:, None] + off[None, :]).reshape(-1)
    ez = (np.arange(nz + 1)[:, None] + off[None, :]).reshape(-1)
    rows, cols = np.array([0.5, nz / 2 + 0.37, nz - 0.5]), np.array([0.5, nx / 2 + 0.37, nx - 0.5])
    out["edges_x"] = _aimed(sc, p, ex[:, None], rows[None, :], rng)
    out["edges_z"] = _aimed(sc, p, cols[None, :], ez[:, None], rng)
    near = np.array([-0.3, -1e-2, 1e-2, 0.3])
    bx = np.concatenate([near, nx + near])
    bz = np.concatenate([near, nz + near])
    out["borders"] = np.concatenate([_aimed(sc, p, bx[:, None], np.linspace(0.37, nz - 0.63, 7)[None, :], rng),
                                     _aimed(sc, p, np.linspace(0.37, nx - 0.63, 7)[None, :], bz[:, None], rng),
                                     _aimed(sc, p, bx[:, None], bz[None, :], rng)])                       # the four corners, all sides
    # reach: directions at chosen angles to the beam axis (rotated poses: cosang against 0.025) or with chosen v (against 1e-4)
    n = 4096
    axis = sc.src[p]["direction"].astype(np.float64) if int(sc.det[p]["rotation_flag"]) == 1 else np.array([0.0, 1.0, 0.0])
    thr = 0.025 if int(sc.det[p]["rotation_flag"]) == 1 else 1.0e-4
    c = np.concatenate([thr * (1.0 + np.array([s * 10.0 ** -k for k in range(1, 7) for s in (-1, 1)]).repeat(64)), rng.uniform(-1.0, thr, n // 2),
                        rng.uniform(thr, 0.2, n // 4)])
    t = rng.normal(size=(c.size, 3))
    t -= (t @ axis)[:, None] * axis
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    d = c[:, None] * axis + np.sqrt(1.0 - c * c)[:, None] * t
    start = _starts(sc, c.size, rng)
    out["reach"] = np.concatenate([start, d, rng.uniform(2e4, 9e4, (c.size, 1)), rng.integers(0, 4, (c.size, 1)).astype(np.float64)], axis=1).astype(np.float32)
    e = np.concatenate([np.array(TIES), [float(sc.espc[sc.nbins]), float(sc.espc[0])], rng.uniform(float(sc.espc[0]), float(sc.espc[sc.nbins]), 1000)])
    out["values"] = _aimed(sc, p, rng.uniform(0, nx, e.size), rng.uniform(0, nz, e.size), rng, energy=e)
    out["random"] = _aimed(sc, p, rng.uniform(-3, nx + 3, 1 << 13), rng.uniform(-3, nz + 3, 1 << 13), rng)
    assert sum(v.shape[0] for v in out.values()) <= 1 << 16
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# HOP: designed rays in the exterior of a region (box AND, where there is one, elliptic cylinder)
# ----------------------------------------------------------------------------------------------------------------------------------
def hop_items(sc: so.Scene) -> dict:
    """name -> float32[n, 8] {x, y, z, u, v, w, E, 0}.  The designs are written for the cylinder; the same rays run on the region
    without one.  Starts lie inside the volume and outside the region's box or cylinder."""
    R = sc.region
    rng = np.random.default_rng(7)
    lo, hi, bbox = R["box_lo"], R["box_hi"], sc.bbox
    cx, cy = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1])
    ia, ib = R["ell_inv"] if R["ell_inv"][0] > 0 else (1.0 / (0.5 * (hi[0] - lo[0])) ** 2, 1.0 / (0.5 * (hi[1] - lo[1])) ** 2)
    a, b = 1.0 / np.sqrt(ia), 1.0 / np.sqrt(ib)
    zmid = 0.5 * (lo[2] + hi[2])

    def pack(start, d, n=None):
        start, d = np.asarray(start, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        e = rng.uniform(1.5e4, 1.1e5, start.shape[0])
        return np.concatenate([start, d, e[:, None], np.zeros((start.shape[0], 1))], axis=1).astype(np.float32)

    out = {}
    n = 512
    # through box and cylinder: from the volume's -y margin towards points well inside the ellipse
    s = np.stack([rng.uniform(0.05, 0.95, n) * bbox[0], np.full(n, 0.3 * lo[1]), rng.uniform(lo[2] + 0.5, hi[2] - 0.5, n)], axis=1)
    r, th = 0.6 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    t = np.stack([cx + a * r * np.cos(th), cy + b * r * np.sin(th), rng.uniform(lo[2] + 0.5, hi[2] - 0.5, n)], axis=1)
    out["through"] = pack(s, t - s)
    # through the box's corner regions, past the cylinder: aimed at points between the ellipse and the box's corner
    q = rng.integers(0, 4, n)
    sx, sy = np.where(q & 1, 1.0, -1.0), np.where(q & 2, 1.0, -1.0)
    corner = np.stack([cx + sx * 0.5 * (hi[0] - lo[0]) * rng.uniform(0.93, 0.99, n), cy + sy * 0.5 * (hi[1] - lo[1]) * rng.uniform(0.93, 0.99, n),
                       rng.uniform(lo[2] + 0.5, hi[2] - 0.5, n)], axis=1)
    dirs = np.stack([-sy * rng.uniform(0.8, 1.2, n) * a, sx * rng.uniform(0.8, 1.2, n) * b, rng.uniform(-0.2, 0.2, n)], axis=1)   # along the corner's diagonal cut
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    out["corner"] = pack(corner - dirs * rng.uniform(2.0, 4.0, n)[:, None], dirs)
    # tangent to the ellipse within 1e-4 (of its scale) either side: rays in a plane z = const
    th = rng.integers(0, 4, n) * 0.5 * np.pi + rng.uniform(0.55, 1.02, n)     # around the diagonals: where the cylinder, not the box, bounds the region
    eps = np.tile(np.array([-1e-4, 1e-4, -1e-3, 1e-3, -1e-2, 1e-2, -3e-5, 3e-5]), n // 8)
    touch = np.stack([cx + (1 + eps) * a * np.cos(th), cy + (1 + eps) * b * np.sin(th), np.full(n, zmid)], axis=1)
    tang = np.stack([-a * np.sin(th), b * np.cos(th), np.zeros(n)], axis=1)
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    back = rng.uniform(0.3, 0.9, n) * np.minimum(a, b)
    out["tangent"] = pack(touch - tang * back[:, None], tang)
    # parallel to the cylinder's axis, inside and outside it, from below and above the box
    r = np.where(np.arange(n) % 2 == 0, rng.uniform(0.0, 0.95, n), rng.uniform(1.05, 1.3, n))
    th = rng.uniform(0, 2 * np.pi, n)
    up = np.arange(n) % 4 < 2
    s = np.stack([np.clip(cx + a * r * np.cos(th), 0.01 * bbox[0], 0.99 * bbox[0]), np.clip(cy + b * r * np.sin(th), 0.01 * bbox[1], 0.99 * bbox[1]),
                  np.where(up, 0.5 * lo[2], hi[2] + 0.5 * (bbox[2] - hi[2]))], axis=1)
    out["along"] = pack(s, np.stack([np.zeros(n), np.zeros(n), np.where(up, 1.0, -1.0)], axis=1))
    # rays that miss the box and leave through each of the six faces
    s = np.stack([rng.uniform(0.02, 0.98, n) * bbox[0], np.full(n, 0.5 * lo[1]), rng.uniform(0.02, 0.98, n) * bbox[2]], axis=1)
    face = np.arange(n) % 6
    d = rng.normal(size=(n, 3)) * 0.15
    d[np.arange(n), face // 2] = np.where(face % 2 == 0, -1.0, 1.0)
    d[face == 3] = np.array([0.0, 1.0, 0.0]) + rng.normal(size=(int(np.sum(face == 3)), 3)) * 0.02      # +y: towards the box (most hit it)
    out["faces"] = pack(s, d)
    # starts inside the cylinder's span (|z| beyond the box, x / y inside the ellipse) but outside the box
    r, th = 0.8 * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
    s = np.stack([cx + a * r * np.cos(th), cy + b * r * np.sin(th), np.where(np.arange(n) % 2 == 0, 0.6 * lo[2], hi[2] + 0.4 * (bbox[2] - hi[2]))], axis=1)
    d = rng.normal(size=(n, 3))
    out["span"] = pack(s, d)
    # random rays from the exterior below the box in y
    m = 1 << 16
    s = np.stack([rng.uniform(0.01, 0.99, m) * bbox[0], rng.uniform(0.05, 0.9, m) * lo[1], rng.uniform(0.01, 0.99, m) * bbox[2]], axis=1)
    d = rng.normal(size=(m, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.5
    out["random"] = pack(s, d)
    return out


def hop_ids(n):
    return FIRST_ID + (1 << 20) + np.arange(n, dtype=np.uint64)


def replay_hop(sc: so.Scene, p: int, items, mapping="f32"):
    items = np.asarray(items, dtype=np.float32)
    dev = so.sr.MwcDeviates(hop_ids(items.shape[0]), SEED, p, mapping)
    e = items[:, 6]
    index = np.floor((e - sc.e0) * sc.ide).astype(np.int64)
    r = so.exterior_entry(sc, items[:, :3].astype(np.float64), items[:, 3:6].astype(np.float64), e.astype(np.float64), index, dev,
                          np.arange(items.shape[0]), False)
    r["state"] = np.stack([dev.x, dev.c], axis=1)
    r["index"] = index
    return r
