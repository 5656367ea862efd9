"""TEST INFRASTRUCTURE: plain restatements of the two ends of a FAST history -- the source, its entry into the volume, the hop across the
homogeneous exterior and the detector tally (4d-cbct-mc_amd/csrc/track_common.inc: sample_source_energy, sample_source_direction,
move_to_bbox, tally_pixel; track_pool.inc: source_entry, exterior_hop, cylinder_span, classify_real) -- numpy only.  Inputs: the host
tables a context hands out (`scene`) and deviates from a provider (scatter_ref.MwcDeviates for the device's streams, scatter_ref.ArrayDeviates
for RANECU values).  Every routine works on arrays of events and returns, beside its result, the MARGIN of every decision it took: how far
that decision is from falling the other way.  Events below a margin are "fragile": another arithmetic may decide them differently.

  source_energy     the float32 rule word for word (bin selection is a discrete decision): bit-equal to every build
  source_direction  the rejection loop in the beam frame, the cot clamp of the FAST kernels, the pose's rotation; float64 from the
                    float32 dz and phi (their two operations are IEEE in every build)
  move_to_bbox      the reference's entry into the volume (oracle/mcgpu_oracle.c), float64
  exterior_entry    source_entry / exterior_hop: two slab tests, box AND elliptic cylinder, one free path against the target
  tally             tally_image in both detector poses: xd, zd, the image word, rint(E * 100)
  object_region     the object box and the elliptic cylinder the engine fits around everything that is not background
  alias_probabilities  the bin probabilities a Walker table encodes

tests/test_source_law.py pins these to the CPU oracle before any GPU is involved; tests/test_source_gpu.py holds the HIP code to them."""
from __future__ import annotations

import numpy as np

import oracle_lib as ol
import scatter_ref as sr  # noqa: F401  (MwcDeviates / ArrayDeviates: the providers)

F = np.float32
BIG = 3.0e30
EPS_SOURCE = 1.5e-5
PH_FLIGHT, PH_COMPTON, PH_RAYLEIGH, PH_ESCAPED, PH_ABSORBED, PH_NEW = 0, 1, 2, 3, 4, 5
MAXMAT = 25


class Scene:
    """What the restatements read of one context: poses, spectrum, cross sections of the background, the object region."""

    def __init__(self, ctx, region=None):
        self.src = ctx.host_table("source_data").view(ol.SOURCE_DT)
        self.det = ctx.host_table("detector_data").view(ol.DETECTOR_DT)
        self.nbins = ctx.geti("num_spectrum_bins")
        self.espc, self.cutoff = ctx.host_table("espc", "<f4"), ctx.host_table("espc_cutoff", "<f4")
        self.alias = ctx.host_table("espc_alias", "<i2")
        self.e0, self.ide = F(ctx.getf("e0")), F(ctx.getf("ide"))
        self.num_values = ctx.geti("num_energy_values")
        self.bbox = ctx.host_table("size_bbox", "<f4").astype(np.float64)
        self.voxel_size = ctx.host_table("voxel_size", "<f4").astype(np.float64)
        self.mfp_a = ctx.host_table("mfp_a", "<f4").reshape(-1, MAXMAT, 3)      # [bin, material, {total, Compton, Rayleigh}]: a + E b
        self.mfp_b = ctx.host_table("mfp_b", "<f4").reshape(-1, MAXMAT, 3)
        self.wood_coarse = ctx.host_table("woodcock_coarse", "<f4")
        self.region = region

    def fan_ratio(self):
        """TrackCold::fan_ratio_lo / hi by model_device.cpp's formula, in float64: cot at the two ends of the azimuthal aperture, drawn in
        by 2e-6 of their range, rounded to float32."""
        lo = float(self.src[0]["phi_low"])
        hi = lo + float(self.src[0]["D_phi"])
        assert np.all(self.src["phi_low"] == self.src[0]["phi_low"]) and np.all(self.src["D_phi"] == self.src[0]["D_phi"])
        assert 1e-3 < lo < hi < np.pi - 1e-3
        r_hi, r_lo = np.cos(lo) / np.sin(lo), np.cos(hi) / np.sin(hi)
        m = 2.0e-6 * (r_hi - r_lo)
        return F(r_lo + m), F(r_hi - m)


def cold(ctx) -> dict:
    """The TrackCold scalars of a context on a device (host_table "track_cold")."""
    v = ctx.host_table("track_cold", "<f4")
    return dict(fan_lo=v[0], fan_hi=v[1], box_lo=v[2:5].astype(np.float64), box_hi=v[5:8].astype(np.float64), ell_c=v[8:10].astype(np.float64),
                ell_inv=v[10:12].astype(np.float64), bbox=v[12:15].astype(np.float64), has_exterior=int(v[15]), ext_density=float(v[16]),
                ext_material=int(v[17]), ext_compact=int(v[18]))


def object_region(ctx, brick_shift: int = 2):
    """model_device.cpp's mark_exterior_region from the host voxels: bricks of 2^brick_shift voxels; the background is the most frequent
    (material, density) among homogeneous bricks; the object box bounds the bricks that hold anything else; the elliptic cylinder has the
    box's centre and aspect and is scaled until every corner of every object brick is inside, and is kept only if it puts 5 % of the box's
    bricks wholly outside.  Returns the dict of `cold` without the fan ratios, or None where the geometry has no exterior."""
    n = [ctx.geti(f"num_voxels_{a}") for a in "xyz"]
    vs = ctx.host_table("voxel_size", "<f4")
    md = ctx.host_table("voxel_mat_dens", "<f4").reshape(n[2], n[1], n[0], 2)
    _, code = np.unique(md.reshape(-1, 2), axis=0, return_inverse=True)
    code = code.reshape(n[2], n[1], n[0])
    b = 1 << brick_shift
    bn = [(v + b - 1) // b for v in n]
    pad = np.pad(code, [(0, bn[2] * b - n[2]), (0, bn[1] * b - n[1]), (0, bn[0] * b - n[0])], mode="edge")
    blocks = pad.reshape(bn[2], b, bn[1], b, bn[0], b)
    lo_, hi_ = blocks.min(axis=(1, 3, 5)), blocks.max(axis=(1, 3, 5))
    homogeneous = lo_ == hi_
    if not homogeneous.any():
        return None
    counts = np.bincount(lo_[homogeneous])
    background = int(np.argmax(counts))                                       # (ties: the cases have none)
    assert np.sum(counts == counts.max()) == 1
    obj = ~(homogeneous & (lo_ == background))                                  # [z, y, x]
    if not obj.any():
        return None
    iz, iy, ix = np.nonzero(obj)
    lo = np.array([ix.min(), iy.min(), iz.min()])
    hi = np.array([ix.max(), iy.max(), iz.max()])
    box_lo = np.array([F(lo[a] * b) * vs[a] for a in range(3)], dtype=F)
    box_hi = np.array([F(min((hi[a] + 1) * b, n[a])) * vs[a] for a in range(3)], dtype=F)
    ecx, ecy = F(0.5) * (box_lo[0] + box_hi[0]), F(0.5) * (box_lo[1] + box_hi[1])
    ea, eb = F(0.5) * (box_hi[0] - box_lo[0]), F(0.5) * (box_hi[1] - box_lo[1])

    def rect(cx, cy):
        return (F(cx * b) * vs[0], F(min((cx + 1) * b, n[0])) * vs[0], F(cy * b) * vs[1], F(min((cy + 1) * b, n[1])) * vs[1])

    s2 = 0.0
    for cx, cy in set(zip(ix.tolist(), iy.tolist())):
        r = rect(cx, cy)
        for px in r[:2]:
            for py in r[2:]:
                s2 = max(s2, (float(px) - float(ecx)) ** 2 / float(ea) ** 2 + (float(py) - float(ecy)) ** 2 / float(eb) ** 2)
    s2 *= 1.0 + 1.0e-4
    inv = np.array([F(1.0 / (s2 * float(ea) ** 2)), F(1.0 / (s2 * float(eb) ** 2))], dtype=F)

    def outside(cx, cy):
        r = rect(cx, cy)
        px, py = min(max(ecx, r[0]), r[1]) - ecx, min(max(ecy, r[2]), r[3]) - ecy
        return px * px * inv[0] + py * py * inv[1] > F(1.001)

    cols = [(cx, cy) for cx in range(lo[0], hi[0] + 1) for cy in range(lo[1], hi[1] + 1)]
    cut = sum(outside(cx, cy) for cx, cy in cols) * (hi[2] - lo[2] + 1)
    in_box = len(cols) * (hi[2] - lo[2] + 1)
    if cut * 20 < in_box:
        inv[:] = 0
    out_of_box = bn[0] * bn[1] * bn[2] - in_box
    if out_of_box + (cut if inv[0] > 0 else 0) == 0:
        return None
    mat, dens = md.reshape(-1, 2)[np.nonzero(code.reshape(-1) == background)[0][0]]
    return dict(box_lo=box_lo.astype(np.float64), box_hi=box_hi.astype(np.float64), ell_c=np.array([ecx, ecy], dtype=np.float64),
                ell_inv=inv.astype(np.float64), bbox=ctx.host_table("size_bbox", "<f4").astype(np.float64), has_exterior=1,
                ext_density=float(dens), ext_material=int(mat) - 1)


# ----------------------------------------------------------------------------------------------------------------------------------
# source
# ----------------------------------------------------------------------------------------------------------------------------------
def alias_probabilities(cutoff, alias, nbins: int):
    """P(bin) of a Walker table: column ip is drawn with 1 / nbins and yields ip below its cut-off, alias[ip] above."""
    c = np.asarray(cutoff[:nbins], dtype=np.float64)
    p = c.copy()
    np.add.at(p, np.asarray(alias[:nbins], dtype=np.int64), 1.0 - c)
    return p / nbins


def source_energy(sc: Scene, dev, idx):
    """sample_source_energy in float32, operation by operation: (E float32, bin, energy bin of the tables, column ip)."""
    xi = dev.next(idx).astype(F)
    rn = xi * F(sc.nbins)
    ip = np.floor(rn).astype(np.int64)
    fr = rn - ip.astype(F)
    b = np.where(fr < sc.cutoff[ip], ip, sc.alias[ip].astype(np.int64))
    xi2 = dev.next(idx).astype(F)
    e = sc.espc[b] + xi2 * (sc.espc[b + 1] - sc.espc[b])
    assert e.dtype == F and rn.dtype == F and fr.dtype == F
    index = np.floor((e - sc.e0) * sc.ide).astype(np.int64)
    return e, b, index, ip


def source_direction(sc: Scene, p: int, dev, idx, fan=None):
    """sample_source_direction.  dz and phi follow the float32 rule (one multiply, one add, IEEE in every build); everything after them is
    float64.  `fan` = (fan_ratio_lo, fan_ratio_hi): the FAST kernels' clamp of dx / dy; None: the reference's rule, no clamp.
    Returns d (pose frame), beam (beam frame, after the clamp), dz32, phi32, trials, margin = the smallest relative distance of the
    aperture ratio |dz / (dy + 1e-7)| from max_height_at_y1cm over the trials, clamped."""
    s = sc.src[p]
    idx = np.asarray(idx)
    n = idx.size
    beam = np.zeros((n, 3))
    dz32, phi32 = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    trials, margin = np.zeros(n, dtype=np.int64), np.full(n, np.inf)
    mh = float(s["max_height_at_y1cm"])
    active = np.arange(n)
    while active.size:
        ii = idx[active]
        z32 = s["cos_theta_low"] + dev.next(ii).astype(F) * s["D_cos_theta"]
        ph32 = s["phi_low"] + dev.next(ii).astype(F) * s["D_phi"]
        assert z32.dtype == F and ph32.dtype == F
        dz, phi = z32.astype(np.float64), ph32.astype(np.float64)
        sth = np.sqrt(1.0 - dz * dz)
        dy, dx = sth * np.sin(phi), sth * np.cos(phi)
        ratio = np.abs(dz / (dy + 1.0e-7))
        trials[active] += 1
        margin[active] = np.minimum(margin[active], np.abs(ratio - mh) / mh)
        ok = ~(ratio > mh)
        beam[active[ok]] = np.stack([dx, dy, dz], axis=1)[ok]
        dz32[active[ok]], phi32[active[ok]] = z32[ok], ph32[ok]
        active = active[~ok]
    clamped = np.zeros(n, dtype=bool)
    if fan is not None:
        a, b = beam[:, 1] * float(fan[0]), beam[:, 1] * float(fan[1])
        x = np.where(beam[:, 1] > 0, np.clip(beam[:, 0], np.minimum(a, b), np.maximum(a, b)), beam[:, 0])    # the median of the three
        clamped = x != beam[:, 0]
        beam[:, 0] = x
    d = beam.copy()
    if int(sc.det[p]["rotation_flag"]) == 1:
        d = beam @ s["rot_fan"].astype(np.float64).reshape(3, 3).T
    return dict(d=d, beam=beam, dz32=dz32, phi32=phi32, trials=trials, margin=margin, clamped=clamped)


def move_to_bbox(pos, d, bbox):
    """The reference's move_to_bbox (K.cu:714-805, oracle/mcgpu_oracle.c) in float64: (position, miss, margin [cm] = distance of the
    moved point from the nearest face on the axes it did not enter through: what decides `miss`)."""
    pos, d = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    bbox = np.asarray(bbox, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fwd = np.where(pos > 0, 0.0, EPS_SOURCE - pos / d)
        bwd = np.where(pos < bbox, 0.0, EPS_SOURCE + (bbox - pos) / d)
    e = np.where(d > EPS_SOURCE, fwd, np.where(d < -EPS_SOURCE, bwd, -500000.0))
    ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
    axis = np.where((ey > ex) & (ey > ez), 1, np.where(ex > ez, 0, 2))
    step = e[np.arange(e.shape[0]), axis]
    moved = pos + step[:, None] * d
    miss = np.any((moved < 0) | (moved > bbox), axis=1)
    face = np.minimum(np.abs(moved), np.abs(moved - bbox))
    face[np.arange(e.shape[0]), axis] = np.inf
    return np.where(miss[:, None], pos, moved), miss, face.min(axis=1)


# ----------------------------------------------------------------------------------------------------------------------------------
# the homogeneous exterior
# ----------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)


def cylinder_span(region, pos, d):
    """Entry / exit parameters of rays with the elliptic cylinder (a miss gives in > out), and the margin of its decisions: the
    discriminant's distance from 0 relative to its two terms, or qc's from 0 for a ray along the axis."""
    n = pos.shape[0]
    ia, ib = region["ell_inv"]
    if ia == 0.0:
        return np.full(n, -BIG), np.full(n, BIG), np.full(n, np.inf)
    dx, dy = pos[:, 0] - region["ell_c"][0], pos[:, 1] - region["ell_c"][1]
    u, v = d[:, 0], d[:, 1]
    qa, qb, qc = u * u * ia + v * v * ib, dx * u * ia + dy * v * ib, dx * dx * ia + dy * dy * ib - 1.0
    disc = qb * qb - qa * qc
    along = ~(qa > 1.0e-12)
    sq, inv = np.sqrt(np.maximum(disc, 0.0)), 1.0 / np.where(along, 1.0, qa)
    inside = qc <= 0.0
    t_in = np.where(along, np.where(inside, -BIG, BIG), np.where(disc < 0, BIG, (-qb - sq) * inv))
    t_out = np.where(along, np.where(inside, BIG, -BIG), np.where(disc < 0, -BIG, (-qb + sq) * inv))
    margin = np.where(along, np.abs(qc), np.abs(disc) / np.maximum(np.maximum(qb * qb, np.abs(qa * qc)), 1e-300))
    margin = np.minimum(margin, np.abs(qa - 1.0e-12) / np.maximum(qa, 1.0e-12))
    return t_in, t_out, margin


def exterior_entry(sc: Scene, pos, d, energy, index, dev, idx, at_source: bool, mfpw=None):
    """source_entry (at_source: from the focal spot, through the volume's faces, with the deviate of the entry-face shell drawn first) /
    exterior_hop (from a point inside the volume) in float64.  One free path in the background against the target -- the entry into
    the object region (box AND cylinder) or, for a ray that misses it, the exit from the volume -- then classify_real for an
    interaction.  Returns phase, pos, real, shell (at_source: events the kernel sends into entry_face_shell), and `margin`: the
    smallest relative distance of a decision from flipping (hits the volume, hits the region, the cylinder's discriminant, free path
    against target, the classifying deviate against its thresholds)."""
    R = sc.region
    pos, d = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx)
    n = pos.shape[0]
    energy = np.asarray(energy, dtype=np.float64)
    with np.errstate(divide="ignore"):
        inv = np.where(np.abs(d) > 1.0e-12, 1.0 / d, BIG)
    margin = np.full(n, np.inf)
    shell = np.zeros(n, dtype=bool)
    if at_source:
        va, vb = -pos * inv, (sc.bbox - pos) * inv
        near = np.minimum(va, vb)
        v_in = np.maximum(near.max(axis=1), 0.0)
        v_out = np.maximum(va, vb).min(axis=1)
        hits_vol = v_out >= v_in
        margin = np.minimum(margin, _rel(v_out, v_in))
        reach = (1.0 - dev.next(idx)) * np.asarray(mfpw, dtype=np.float64)
        axis = np.where(v_in == near[:, 0], 0, np.where(v_in == near[:, 1], 1, 2))
        shell = hits_vol & (v_in > 0) & (reach <= 6.0e-5 * np.abs(inv[np.arange(n), axis]))
    else:
        v_in, hits_vol = np.zeros(n), np.ones(n, dtype=bool)
        v_out = np.abs((np.where(d > 0, sc.bbox, 0.0) - pos) * inv).min(axis=1)                       # t_exit
    oa, ob = (R["box_lo"] - pos) * inv, (R["box_hi"] - pos) * inv
    c_in, c_out, m_cyl = cylinder_span(R, pos, d)
    o_in = np.maximum(np.maximum(np.minimum(oa, ob).max(axis=1), c_in), 0.0)
    o_out = np.minimum(np.maximum(oa, ob).min(axis=1), c_out)
    hits_obj = o_out >= o_in
    margin = np.minimum(margin, np.minimum(m_cyl, _rel(np.clip(o_out, -1e6, 1e6), np.clip(o_in, -1e6, 1e6))))
    target = np.where(hits_obj, o_in, v_out)
    a_tot, b_tot = sc.mfp_a[index, R["ext_material"], 0].astype(np.float64), sc.mfp_b[index, R["ext_material"], 0].astype(np.float64)
    mu = R["ext_density"] * (a_tot + energy * b_tot)
    s = v_in - np.log(dev.next(idx)) / mu
    margin = np.minimum(margin, np.where(hits_vol, _rel(s, target), np.inf))
    real = hits_vol & (s < target)
    flight = hits_vol & ~real & hits_obj
    m = np.where(real, s, np.where(flight, target + 1.0e-4, 0.0))
    out = pos + m[:, None] * d
    phase = np.where(flight, PH_FLIGHT, PH_ESCAPED)
    if real.any():
        r = np.nonzero(real)[0]
        e = energy[r]
        mat = R["ext_material"]
        s_tot = sc.mfp_a[index[r], mat, 0].astype(np.float64) + e * sc.mfp_b[index[r], mat, 0]
        s_co = sc.mfp_a[index[r], mat, 1].astype(np.float64) + e * sc.mfp_b[index[r], mat, 1]
        s_ra = sc.mfp_a[index[r], mat, 2].astype(np.float64) + e * sc.mfp_b[index[r], mat, 2]
        x = dev.next(idx[r]) * s_tot
        phase[r] = np.where(x < s_co, PH_COMPTON, np.where(x < s_co + s_ra, PH_RAYLEIGH, PH_ABSORBED))
        margin[r] = np.minimum(margin[r], np.minimum(np.abs(x - s_co), np.abs(x - (s_co + s_ra))) / s_tot)
    return dict(phase=phase, pos=out, real=real, flight=flight, shell=shell, margin=margin, s=s, target=target, mu=mu, v_in=v_in, hits_vol=hits_vol,
                hits_obj=hits_obj)


# ----------------------------------------------------------------------------------------------------------------------------------
# detector
# ----------------------------------------------------------------------------------------------------------------------------------
def tally(sc: Scene, p: int, pos, d, energy, state):
    """tally_image (K.cu:482-604) in float64 for float32 inputs, in both detector poses.  Returns xd, zd (pixels from the lower corner),
    reaches, word (-1: none), value = rint(float32(E) * float32(100)) (__float2uint_rn: ties to even), margin_pixel = distance of xd / zd
    from the nearest integer (pixels), margin_reach = distance of cosang from 0.025 / of v from 1e-4."""
    S, D = sc.src[p], sc.det[p]
    pos, d = np.asarray(pos, dtype=F).astype(np.float64).reshape(-1, 3), np.asarray(d, dtype=F).astype(np.float64).reshape(-1, 3)
    corner, centre = D["corner_min_rotated_to_Y"].astype(np.float64), D["center"].astype(np.float64)
    if int(D["rotation_flag"]) == 1:
        sd = S["direction"].astype(np.float64)
        cosang = d @ sd
        reaches = ~(cosang < float(F(0.025)))
        m_reach = np.abs(cosang - float(F(0.025)))
        dist = ((centre - pos) @ sd) / np.where(reaches, cosang, 1.0)
        hit = pos + dist[:, None] * d
        r = hit @ D["rot_inv"].astype(np.float64).reshape(3, 3).T
        rx, rz = r[:, 0], r[:, 2]
    else:
        reaches = ~(d[:, 1] < float(F(0.0001)))
        m_reach = np.abs(d[:, 1] - float(F(0.0001)))
        dist = (centre[1] - pos[:, 1]) / np.where(reaches, d[:, 1], 1.0)
        rx, rz = pos[:, 0] + dist * d[:, 0], pos[:, 2] + dist * d[:, 2]
    xd, zd = (rx - corner[0]) * float(D["inv_pixel_size_X"]), (rz - corner[2]) * float(D["inv_pixel_size_Z"])
    px, pz = np.floor(xd).astype(np.int64), np.floor(zd).astype(np.int64)
    nx, nz = int(D["num_pixels"][0]), int(D["num_pixels"][1])
    inside = reaches & (px > -1) & (px < nx) & (pz > -1) & (pz < nz)
    word = np.where(inside, np.asarray(state, dtype=np.int64) * int(D["total_num_pixels"]) + px + pz * nx, -1)
    value = np.rint(np.asarray(energy, dtype=F) * F(100.0)).astype(np.int64)
    m_pixel = np.minimum(np.abs(xd - np.rint(xd)), np.abs(zd - np.rint(zd)))
    return dict(xd=xd, zd=zd, reaches=reaches, word=word, value=value, margin_pixel=m_pixel, margin_reach=m_reach, px=px, pz=pz)


def tally_f32(sc: Scene, p: int, pos, d):
    """xd, zd as tally_pixel computes them, operation by operation in float32 (no contraction; the quotient IEEE where the kernel
    multiplies by v_rcp_f32's 1-ulp reciprocal): what float32 costs these coordinates, for the margin of the pixel-edge tests."""
    S, D = sc.src[p], sc.det[p]
    P, d = np.asarray(pos, dtype=F).reshape(-1, 3), np.asarray(d, dtype=F).reshape(-1, 3)
    x, y, z, u, v, w = P[:, 0], P[:, 1], P[:, 2], d[:, 0], d[:, 1], d[:, 2]
    c, ctr = D["corner_min_rotated_to_Y"], D["center"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if int(D["rotation_flag"]) == 1:
            sd, r = S["direction"], D["rot_inv"]
            cosang = u * sd[0] + (v * sd[1] + w * sd[2])
            dist = (sd[0] * (ctr[0] - x) + (sd[1] * (ctr[1] - y) + sd[2] * (ctr[2] - z))) / np.where(cosang < F(0.025), F(1), cosang)
            hx, hy, hz = x + dist * u, y + dist * v, z + dist * w
            rx, rz = r[0] * hx + r[1] * hy + r[2] * hz, r[6] * hx + r[7] * hy + r[8] * hz
        else:
            dist = (ctr[1] - y) / np.where(v < F(0.0001), F(1), v)
            rx, rz = x + dist * u, z + dist * w
        xd, zd = (rx - c[0]) * D["inv_pixel_size_X"], (rz - c[2]) * D["inv_pixel_size_Z"]
    assert xd.dtype == F and zd.dtype == F
    return xd, zd


def detector_point(sc: Scene, p: int, xd, zd):
    """The point of the detector plane of projection p at detector coordinates (xd, zd) [pixels from the lower corner], float64."""
    D = sc.det[p]
    xd, zd = np.asarray(xd, dtype=np.float64), np.asarray(zd, dtype=np.float64)
    corner, centre = D["corner_min_rotated_to_Y"].astype(np.float64), D["center"].astype(np.float64)
    rx, rz = corner[0] + xd / float(D["inv_pixel_size_X"]), corner[2] + zd / float(D["inv_pixel_size_Z"])
    if int(D["rotation_flag"]) == 1:
        rot = D["rot_inv"].astype(np.float64).reshape(3, 3)
        ry = np.full(rx.shape, (rot @ centre)[1])
        return np.stack([rx, ry, rz], axis=1) @ rot                              # rot is orthonormal: its transpose maps back
    return np.stack([rx, np.full(rx.shape, centre[1]), rz], axis=1)
