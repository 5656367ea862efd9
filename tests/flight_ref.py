"""TEST INFRASTRUCTURE: a plain restatement of the middle of a FAST history, the Woodcock flight step (4d-cbct-mc_amd/csrc/track_pool.inc:
flight_locate, flight_resolve, flight_steps, classify_real) with the host tables it reads (model_device.cpp: coarse_woodcock,
sigma_brackets; the brick grid; the 16-byte tile records) -- numpy only.  Deviates come from a provider (scatter_ref.MwcDeviates for the
device's streams, scatter_ref.ArrayDeviates for RANECU values).

Everything AFTER the position of a step is IEEE float32 with contraction off, and is restated bit for bit: the clamp to [kEps, bbox_hi],
(int)(c * inv_vs), `out`, md = mfpW * dens, the cached cross section aux = fmaf(E, b, a), p_thr, the bracket path with its mc_old / aux
cache rule, classify_real's three fmaf, xi * s_tot and s_co + s_ra.  fmaf is emulated in float64 (the product of two float32 is exact
there); where the float64 sum lies within one of its ulps of a float32 rounding tie it is recomputed in exact rational arithmetic, so no
event is set aside as fragile.  Only the step length goes through the hardware logarithm: pos + (-ln2 mfpW log2(xi)) d is restated in
float64 (step_position) and in float32 numpy (step_position_f32: the yardstick of the position tolerance).

  Tables            what the step reads, from a context: with a device the downloads ("mfp_tot", "sigma_bracket_mid", ...), without one
                    the same tables built from the reference-layout host tables (mfp_a / mfp_b, density_max)
  locate            flight_locate's clamp, index and `out`; voxel() the (density, compact material) the step must see there
  resolve           flight_resolve: one virtual-or-real test, with the branch it took
  classify          classify_real
  replay            a trace of flight steps from the device's own previous positions
  walk              whole flights in float64 from given deviates and a given majorant (tests/test_flight_law.py: against the oracle)
  coarse_woodcock, tile_paths, decode_tile, bracket_bounds   the host builders' rules and the record layout

tests/test_flight_law.py pins this to the CPU oracle before any GPU is involved; tests/test_flight_gpu.py holds the HIP code to it."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import scatter_ref as sr  # noqa: F401  (MwcDeviates / ArrayDeviates: the providers)

F = np.float32
K_EPS = F(0.000015)
LN2 = 0.69314718055994531
WOOD_SHIFT = 6
MAXMAT = 25
PH_FLIGHT, PH_COMPTON, PH_RAYLEIGH, PH_ESCAPED, PH_ABSORBED, PH_REAL, PH_HOP = 0, 1, 2, 3, 4, 7, 8
VOL_U8, VOL_U16, VOL_RAW, VOL_U8_SUB, VOL_U8_REC = 0, 1, 2, 3, 4
BRICK_EXTERIOR, BRICK_MIXED = 14, 15
TILE_ASK_VOLUME = 0xC0000000
# the branch of flight_resolve a step took
BR_CACHE, BR_LO, BR_HI, BR_EXACT = 0, 1, 2, 3     # same material as the cached cross section / settled by p_lo / by p_hi / exact table


# ----------------------------------------------------------------------------------------------------------------------------------
# float32 fused multiply-add, correctly rounded
# ----------------------------------------------------------------------------------------------------------------------------------
def _round_fraction_f32(x: Fraction) -> np.float32:
    r = F(float(x))                                     # Fraction -> float64 is correctly rounded; then the three float32 around it
    cands = {float(r), float(np.nextafter(r, F(np.inf))), float(np.nextafter(r, F(-np.inf)))}
    best = sorted(cands, key=lambda c: (abs(Fraction(c) - x), int(F(c).view(np.uint32)) & 1))   # nearest; a tie: the even mantissa
    return F(best[0])


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, one rounding.  a * b is exact in float64; the sum is rounded twice (to float64, to float32), which
    differs from one rounding only where the float64 sum sits on -- or within one of its ulps of -- the midpoint of two float32: those
    entries are recomputed exactly."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F), np.asarray(c, dtype=F))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    r = s.astype(F)
    d = s - r.astype(np.float64)
    toward = np.where(d >= 0, F(np.inf), F(-np.inf)).astype(F)
    half = 0.5 * np.abs(np.nextafter(r, toward).astype(np.float64) - r.astype(np.float64))
    risky = np.abs(np.abs(d) - half) <= np.spacing(np.abs(s))
    if np.any(risky):
        r = r.copy()
        for i in zip(*np.nonzero(risky)):
            r[i] = _round_fraction_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def half_to_f32(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(F)


# ----------------------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------------------
def host_compact_of(ctx):
    """model_device.cpp's compact numbering from the host tables: the materials the model holds (air always, and whatever a voxel uses:
    density_max > 0), numbered in order."""
    dm = ctx.host_table("density_max", "<f4")
    used = dm[:MAXMAT] > 0
    used[0] = True
    out = np.full(MAXMAT, -1, dtype=np.int64)
    out[used] = np.arange(int(used.sum()))
    return out


def coarse_woodcock(mfp_woodcock, e0, ide, num_values):
    """model_device.cpp's coarse_woodcock: per coarse bin of 2^WOOD_SHIFT table bins the smallest value x_i + E y_i takes at the ends of its
    table bins, in float64, lowered by one part in 1e6, rounded to float32."""
    w = np.asarray(mfp_woodcock, dtype=F).reshape(-1, 2).astype(np.float64)[:num_values]
    e0, de = float(e0), 1.0 / float(ide)
    i = np.arange(num_values)
    lo = np.minimum(w[:, 0] + (e0 + i * de) * w[:, 1], w[:, 0] + (e0 + (i + 1) * de) * w[:, 1])
    nc = (num_values + (1 << WOOD_SHIFT) - 1) >> WOOD_SHIFT
    pad = np.full(nc << WOOD_SHIFT, np.inf)
    pad[:num_values] = lo
    return (pad.reshape(nc, -1).min(axis=1) * (1.0 - 1.0e-6)).astype(F)


class Tables:
    """What a flight step reads of one context."""

    def __init__(self, ctx, device: bool):
        self.n = np.array([ctx.geti(f"num_voxels_{a}") for a in "xyz"], dtype=np.int64)
        self.inv_vs = ctx.host_table("inv_voxel_size", "<f4").astype(F)[:3]
        self.voxel_size = ctx.host_table("voxel_size", "<f4").astype(np.float64)[:3]
        self.bbox = ctx.host_table("size_bbox", "<f4").astype(F)[:3]
        self.e0, self.ide = F(ctx.getf("e0")), F(ctx.getf("ide"))
        self.nv = ctx.geti("num_energy_values")
        self.bbox_hi = np.array([self._bbox_hi(k) for k in range(3)], dtype=F)
        md = ctx.host_table("voxel_mat_dens", "<f4").reshape(self.n[2], self.n[1], self.n[0], 2)
        self.vox_material = md[..., 0].astype(np.int64) - 1                      # material number - 1, [z, y, x]
        self.vox_density = md[..., 1].astype(F)
        self.mfp_a = ctx.host_table("mfp_a", "<f4").reshape(-1, MAXMAT, 3)       # [bin, material, {total, Compton, Rayleigh}]: a + E b
        self.mfp_b = ctx.host_table("mfp_b", "<f4").reshape(-1, MAXMAT, 3)
        self.density_max = ctx.host_table("density_max", "<f4")[:MAXMAT].astype(F)
        self.wood = ctx.host_table("woodcock_coarse", "<f4").astype(F)
        self.mfp_woodcock = ctx.host_table("mfp_woodcock", "<f4")
        self.device = device
        host_compact = host_compact_of(ctx)
        if device:
            self.compact_of = ctx.host_table("compact_of", "<i4").astype(np.int64)
            self.nmat = int(self.compact_of.max()) + 1
            self.tot = ctx.host_table("mfp_tot", "<f4").reshape(self.nmat, self.nv, 2).astype(F)
            self.sig_shift = ctx.geti("sigma_bracket_shift")
            self.sig_mid = ctx.host_table("sigma_bracket_mid", "<u2").reshape(-1, self.nmat) if self.sig_shift >= 0 else None
            self.sig_w = ctx.host_table("sigma_bracket_w", "<f4").astype(F) if self.sig_shift >= 0 else None
            self.volume_kind = ctx.geti("volume_kind")
            self.brick_shift = ctx.geti("brick_shift")
            self.has_exterior = ctx.geti("exterior_mode") if (self.volume_kind == VOL_U8 and ctx.geti("bricks_exterior") > 0) else 0
            if self.volume_kind == VOL_U8:
                packed = ctx.host_table("brick_codes", "u1")
                self.brick_n = (self.n + (1 << self.brick_shift) - 1) >> self.brick_shift
                codes = np.stack([packed & 0xF, packed >> 4], axis=1).reshape(-1)[:int(np.prod(self.brick_n))]
                self.brick_code = codes.reshape(self.brick_n[2], self.brick_n[1], self.brick_n[0]).astype(np.int64)
                self.brick_palette = ctx.host_table("brick_palette", "<i4").astype(np.int64)
                self.palette = ctx.host_table("palette", "<f4").reshape(-1, 2)
                self.tile_records = ctx.host_table("tile_record_words", "<u4").reshape(-1, 4) if ctx.geti("tile_records") else None
        else:
            self.compact_of, self.sig_shift, self.has_exterior = host_compact, -1, 0
            self.nmat = int(host_compact.max()) + 1
            self.tot = self.host_tot(host_compact)
        self.material_of = np.full(self.nmat, -1, dtype=np.int64)
        self.material_of[self.compact_of[self.compact_of >= 0]] = np.nonzero(self.compact_of >= 0)[0]
        self.vox_mc = self.compact_of[self.vox_material]

    def _bbox_hi(self, k):
        """make_args: bbox - EPS_SOURCE in float32, lowered by nextafter until (int)(hi * inv_vs) indexes the last voxel."""
        hi = F(self.bbox[k] - K_EPS)
        while int(F(hi * self.inv_vs[k])) > int(self.n[k]) - 1:
            hi = np.nextafter(hi, F(0))
        return hi

    def host_tot(self, compact_of):
        """mfp_tot from the reference-layout tables: float2 {a_tot, b_tot} at row compact material * num_values + bin (table_row)."""
        used = np.nonzero(compact_of >= 0)[0]
        tot = np.zeros((used.size, self.nv, 2), dtype=F)
        tot[compact_of[used], :, 0] = self.mfp_a[:self.nv, used, 0].T
        tot[compact_of[used], :, 1] = self.mfp_b[:self.nv, used, 0].T
        return tot

    def record(self, index, mc):
        """The 32-byte record of (bin, compact material) as classify_real reads it: (a_tot, a_co, a_ra, b_tot, b_co, b_ra), float32."""
        m = self.material_of[np.asarray(mc)]
        a, b = self.mfp_a[index, m], self.mfp_b[index, m]
        return a[..., 0], a[..., 1], a[..., 2], b[..., 0], b[..., 1], b[..., 2]

    def energy_index(self, energy):
        """__float2int_rd((E - e0) * ide) in float32."""
        return np.floor((np.asarray(energy, dtype=F) - self.e0) * self.ide).astype(np.int64)

    def bin_energy_range(self, bins):
        """The smallest and the largest float32 energy whose energy_index is the bin, found by nextafter from the bin's edges."""
        bins = np.asarray(bins, dtype=np.int64)
        lo = (self.e0.astype(np.float64) + bins / float(self.ide)).astype(F)
        hi = (self.e0.astype(np.float64) + (bins + 1) / float(self.ide)).astype(F)
        for _ in range(64):                                   # the edge's own rounding is a few ulps at most
            lo = np.where(self.energy_index(lo) < bins, np.nextafter(lo, F(np.inf)), lo)
            hi = np.where(self.energy_index(hi) > bins, np.nextafter(hi, F(-np.inf)), hi)
        for _ in range(64):
            dn, up = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
            lo = np.where(self.energy_index(dn) == bins, dn, lo)
            hi = np.where(self.energy_index(up) == bins, up, hi)
        assert np.array_equal(self.energy_index(lo), bins) and np.array_equal(self.energy_index(hi), bins)
        assert np.all(self.energy_index(np.nextafter(lo, F(-np.inf))) == bins - 1) and np.all(self.energy_index(np.nextafter(hi, F(np.inf))) == bins + 1)
        return lo, hi


# ----------------------------------------------------------------------------------------------------------------------------------
# the step
# ----------------------------------------------------------------------------------------------------------------------------------
def locate(t: Tables, pos):
    """flight_locate after the position: clamp to [kEps, bbox_hi] (fmed3), `out`, the voxel index (int)(c * inv_vs) in float32."""
    p = np.asarray(pos, dtype=F).reshape(-1, 3)
    c = np.minimum(np.maximum(p, K_EPS), t.bbox_hi[None, :])
    out = np.any(c != p, axis=1)
    prod = c * t.inv_vs[None, :]
    assert prod.dtype == F
    idx = prod.astype(np.int64)                                # truncation; the product is positive
    return idx, out, c


def voxel(t: Tables, idx):
    """(density float32, compact material) of voxel idx[:, {x, y, z}]: what the step must look up there, whatever the storage kind."""
    return t.vox_density[idx[:, 2], idx[:, 1], idx[:, 0]], t.vox_mc[idx[:, 2], idx[:, 1], idx[:, 0]]


def exterior(t: Tables, idx):
    """The step's `exterior`: the brick of the voxel carries the code kBrickExterior (u8 volumes)."""
    if not t.device or t.volume_kind != VOL_U8:
        return np.zeros(idx.shape[0], dtype=bool)
    b = idx >> t.brick_shift
    return t.brick_code[b[:, 2], b[:, 1], b[:, 0]] == BRICK_EXTERIOR


def resolve(t: Tables, energy, index, mfpw, dens, mc, mc_old, aux, xi, out, ext):
    """flight_resolve, bit for bit, for arrays of events.  energy, mfpw, dens, aux, xi: float32; mc_old: the cached material (-1: none).
    Returns phase, aux', mc_old', branch (BR_*), and the float32 thresholds p (the exact p0 where it was formed, else nan), p_lo, p_hi."""
    energy, mfpw, dens, aux, xi = (np.asarray(v, dtype=F) for v in (energy, mfpw, dens, aux, xi))
    index, mc, mc_old = np.asarray(index, dtype=np.int64), np.asarray(mc, dtype=np.int64), np.asarray(mc_old, dtype=np.int64).copy()
    n = xi.size
    md = mfpw * dens
    assert md.dtype == F
    aux = aux.copy()
    branch = np.full(n, BR_CACHE, dtype=np.int64)
    p_thr = fma32(-md, aux, F(1))
    p_lo, p_hi = np.full(n, np.nan, dtype=F), np.full(n, np.nan, dtype=F)
    other = mc != mc_old
    need = other.copy()
    if t.sig_shift >= 0 and other.any():
        o = np.nonzero(other)[0]
        cb = index[o] >> t.sig_shift
        mid, w = half_to_f32(t.sig_mid[cb, mc[o]]), t.sig_w[cb]
        p_lo[o] = fma32(-md[o], fma32(mid, w, mid), F(1))
        p_hi[o] = fma32(-md[o], fma32(-mid, w, mid), F(1))
        below = xi[o] < p_lo[o]
        p_thr[o] = np.where(below, F(2), F(-1))
        need[o] = ~below & (xi[o] < p_hi[o])
        branch[o] = np.where(below, BR_LO, BR_HI)
    if need.any():
        e = np.nonzero(need)[0]
        aux[e] = fma32(energy[e], t.tot[mc[e], index[e], 1], t.tot[mc[e], index[e], 0])
        mc_old[e] = mc[e]
        p_thr[e] = fma32(-md[e], aux[e], F(1))
        branch[e] = BR_EXACT
    virtual = xi < p_thr
    hop = np.asarray(ext, dtype=bool) & bool(t.has_exterior & 1)
    phase = np.where(virtual, np.where(hop, PH_HOP, PH_FLIGHT), PH_REAL)
    phase = np.where(np.asarray(out, dtype=bool), PH_ESCAPED, phase)
    p_exact = np.where((branch == BR_CACHE) | (branch == BR_EXACT), p_thr, F(np.nan)).astype(F)
    return phase, aux, mc_old, branch, p_exact, p_lo, p_hi


def classify(t: Tables, energy, index, mc, xi):
    """classify_real, bit for bit: the kind (PH_COMPTON / PH_RAYLEIGH / PH_ABSORBED) and the deviate margin of that decision (its
    distance from the nearer threshold, as a fraction of s_tot)."""
    energy, xi = np.asarray(energy, dtype=F), np.asarray(xi, dtype=F)
    a_tot, a_co, a_ra, b_tot, b_co, b_ra = t.record(np.asarray(index, dtype=np.int64), np.asarray(mc, dtype=np.int64))
    s_tot, s_co, s_ra = fma32(energy, b_tot, a_tot), fma32(energy, b_co, a_co), fma32(energy, b_ra, a_ra)
    x = xi * s_tot
    both = s_co + s_ra
    assert x.dtype == F and both.dtype == F
    kind = np.where(x < s_co, PH_COMPTON, np.where(x < both, PH_RAYLEIGH, PH_ABSORBED))
    margin = np.minimum(np.abs(x.astype(np.float64) - s_co), np.abs(x.astype(np.float64) - both)) / s_tot.astype(np.float64)
    return kind, margin


def step_position(pos, d, mfpw, xi):
    """The position after a step in float64: pos + (-ln2 mfpW log2(xi)) d, from float32 inputs."""
    step = -LN2 * np.asarray(mfpw, dtype=np.float64) * np.log2(np.asarray(xi, dtype=np.float64))
    return np.asarray(pos, dtype=np.float64) + step[:, None] * np.asarray(d, dtype=np.float64)


def step_position_f32(pos, d, mfpw, xi):
    """The same formula operation by operation in float32 numpy (its log2 is correctly rounded to an ulp; one fmaf per axis): what float32
    costs the position, the yardstick of the device's tolerance."""
    mfpw, xi = np.asarray(mfpw, dtype=F), np.asarray(xi, dtype=F)
    negl2 = F(-LN2) * mfpw
    step = negl2 * np.log2(xi)
    assert step.dtype == F
    p, d = np.asarray(pos, dtype=F), np.asarray(d, dtype=F)
    return np.stack([fma32(step, d[:, k], p[:, k]) for k in range(3)], axis=1)


def replay(t: Tables, items, dev, trace_pos, trace_phase, max_steps):
    """A trace of flight steps restated from the DEVICE's own positions: step k of item i takes the device's position after that step
    (trace_pos[i, k], float32) and restates everything behind it; the position itself is predicted from the device's previous one.
    items: float32[n, >= 7] {x, y, z, u, v, w, E}; dev: the deviates' provider; trace_phase: the device's phases (which steps exist).
    Returns a dict of [n, max_steps] arrays -- phase, mc, aux_bits, branch, taken, pos64 (float64 restatement), pos32 (float32 numpy),
    draws -- and [n] arrays final (phase after classify_real), steps, index, mfpw, mc_old, kind_margin, and the provider advanced as the kernel's."""
    items = np.asarray(items, dtype=F)
    n = items.shape[0]
    energy, d = items[:, 6], items[:, 3:6]
    index = t.energy_index(energy)
    mfpw = t.wood[index >> WOOD_SHIFT]
    mc_old, aux = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=F)
    res = dict(phase=np.zeros((n, max_steps), dtype=np.int64), mc=np.zeros((n, max_steps), dtype=np.int64),
               aux_bits=np.zeros((n, max_steps), dtype=np.uint32), branch=np.full((n, max_steps), -1, dtype=np.int64),
               taken=np.zeros((n, max_steps), dtype=bool), pos64=np.zeros((n, max_steps, 3)), pos32=np.zeros((n, max_steps, 3), dtype=F),
               state=np.zeros((n, max_steps, 2), dtype=np.uint32))
    phase = np.full(n, PH_FLIGHT, dtype=np.int64)
    steps = np.zeros(n, dtype=np.int64)
    prev = items[:, :3].copy()
    for k in range(max_steps):
        a = np.nonzero(phase == PH_FLIGHT)[0]
        if a.size == 0:
            break
        xi_step, xi_test = dev.next(a).astype(F), dev.next(a).astype(F)
        res["pos64"][a, k] = step_position(prev[a], d[a], mfpw[a], xi_step)
        res["pos32"][a, k] = step_position_f32(prev[a], d[a], mfpw[a], xi_step)
        here = np.asarray(trace_pos, dtype=F)[a, k]
        idx, out, _ = locate(t, here)
        dens, mc = voxel(t, idx)
        ph, aux[a], mc_old[a], br, _, _, _ = resolve(t, energy[a], index[a], mfpw[a], dens, mc, mc_old[a], aux[a], xi_test, out, exterior(t, idx))
        phase[a] = ph
        steps[a] += 1
        res["phase"][a, k], res["mc"][a, k], res["aux_bits"][a, k], res["branch"][a, k], res["taken"][a, k] = ph, mc, aux[a].view(np.uint32), br, True
        if hasattr(dev, "x"):
            res["state"][a, k, 0], res["state"][a, k, 1] = dev.x[a], dev.c[a]
        prev[a] = here
    final, margin = phase.copy(), np.full(n, np.inf)
    r = np.nonzero(phase == PH_REAL)[0]
    if r.size:
        last = steps[r] - 1
        final[r], margin[r] = classify(t, energy[r], index[r], res["mc"][r, last], dev.next(r).astype(F))
    res.update(final=final, steps=steps, index=index, mfpw=mfpw, kind_margin=margin, mc_old=mc_old)
    return res


def walk(t: Tables, pos, d, energy, mfpw, dev, max_steps):
    """Whole flights in float64 positions from given deviates and a given majorant (the oracle's is the fine table's a + E b): per step
    one deviate for the length, one for the test against the EXACT p0 (float64; no brackets, no cache: the decision they restate).
    Returns status (PH_REAL, PH_ESCAPED, or PH_FLIGHT after max_steps), pos (float64), voxel index [n, 3], mc, p0 and the test's deviate
    of the last step, face = the smallest distance [cm] of any step's position from a voxel face or from the kEps shell, and
    margin = the smallest |xi - p0| over the steps."""
    pos, d = np.asarray(pos, dtype=np.float64).copy(), np.asarray(d, dtype=np.float64)
    energy = np.asarray(energy, dtype=F)
    n = pos.shape[0]
    index = t.energy_index(energy)
    mfpw = np.asarray(mfpw, dtype=np.float64)
    status = np.full(n, PH_FLIGHT, dtype=np.int64)
    face, margin = np.full(n, np.inf), np.full(n, np.inf)
    vox, mc_out = np.zeros((n, 3), dtype=np.int64), np.full(n, -1, dtype=np.int64)
    p0_out, xi_out = np.zeros(n), np.zeros(n)
    vs, bbox = t.voxel_size, t.bbox.astype(np.float64)
    for _ in range(max_steps):
        a = np.nonzero(status == PH_FLIGHT)[0]
        if a.size == 0:
            break
        pos[a] += (-mfpw[a] * np.log(dev.next(a)))[:, None] * d[a]
        p = pos[a]
        out = np.any((p < float(K_EPS)) | (p > bbox - float(K_EPS)), axis=1)
        shell = np.minimum(np.abs(p - float(K_EPS)), np.abs(p - (bbox - float(K_EPS)))).min(axis=1)
        q = p * t.inv_vs.astype(np.float64)
        cell = np.abs(q - np.rint(q)) * vs
        face[a] = np.minimum(face[a], np.minimum(shell, np.where(out, np.inf, cell.min(axis=1))))
        idx = np.clip(np.floor(q).astype(np.int64), 0, t.n - 1)
        dens, mc = voxel(t, idx)
        s_tot = t.tot[mc, index[a], 0].astype(np.float64) + energy[a].astype(np.float64) * t.tot[mc, index[a], 1]
        p0 = 1.0 - mfpw[a] * dens * s_tot
        inside = a[~out]
        xi = np.zeros(a.size)
        xi[~out] = dev.next(inside)                                  # the oracle draws the test's deviate only inside the volume
        margin[inside] = np.minimum(margin[inside], np.abs(xi - p0)[~out])
        status[a] = np.where(out, PH_ESCAPED, np.where(xi < p0, PH_FLIGHT, PH_REAL))
        vox[a], mc_out[a], p0_out[a], xi_out[a] = idx, mc, p0, xi
    return dict(status=status, pos=pos, voxel=vox, mc=mc_out, p0=p0_out, xi=xi_out, face=face, margin=margin, index=index)


# ----------------------------------------------------------------------------------------------------------------------------------
# host builders
# ----------------------------------------------------------------------------------------------------------------------------------
def tile_paths(records):
    """The decode path of flight_locate for each 16-byte record {ab, code, mask low, mask high}: 0 two entries (code 0), 1 narrow
    (one selector bit per minority voxel), 2 wide (two bits), 3 kTileAskVolume."""
    code = np.asarray(records, dtype=np.uint32)[:, 1]
    return np.where(code == 0, 0, np.where(code >= TILE_ASK_VOLUME, 3, np.where((code >> 30) == 1, 2, 1)))


def decode_tile(record, bit):
    """The palette index flight_locate reads from a record for voxel `bit` = (iz & 3) 16 + (iy & 3) 4 + (ix & 3), or -1: ask the volume."""
    ab, code, lo, hi = (int(v) for v in record)
    mask = lo | (hi << 32)
    if code >= TILE_ASK_VOLUME:
        return -1
    if not (mask >> bit) & 1:
        return ab & 0xFF
    if code == 0:
        return (ab >> 8) & 0xFF
    rank = bin(mask & ((1 << bit) - 1)).count("1")
    wide = code >> 30
    sel = (code >> (rank << wide)) & (1 + 2 * wide)
    return (ab >> (8 + 8 * sel)) & 0xFF


def bracket_bounds(t: Tables, cb, mc):
    """(lo, hi) of a bracket in float32 as the kernel forms them: fmaf(-mid, w, mid), fmaf(mid, w, mid)."""
    mid, w = half_to_f32(t.sig_mid[cb, mc]), t.sig_w[cb]
    return fma32(-mid, w, mid), fma32(mid, w, mid)
