"""Helpers shared by the parity tests: oracle tables from the product's own host model."""
from __future__ import annotations

import numpy as np

import oracle_lib as ol


def tables_from_context(ctx) -> ol.TableSet:
    """Feed the CPU oracle with the host tables the product parsed (reference layouts via the C ABI).
    The tables themselves are pinned against the reference by tests/test_host_tables.py."""
    a = {
        "voxel_mat_dens": ctx.host_table("voxel_mat_dens", "<f4"),
        "mfp_woodcock": ctx.host_table("mfp_woodcock", "<f4"),
        "mfp_a": ctx.host_table("mfp_a", "<f4"), "mfp_b": ctx.host_table("mfp_b", "<f4"),
        "xco": ctx.host_table("xco", "<f4"), "pco": ctx.host_table("pco", "<f4"),
        "aco": ctx.host_table("aco", "<f4"), "bco": ctx.host_table("bco", "<f4"),
        "pmax": ctx.host_table("pmax", "<f4"), "itlco": ctx.host_table("itlco"), "ituco": ctx.host_table("ituco"),
        "fco": ctx.host_table("fco", "<f4"), "uico": ctx.host_table("uico", "<f4"), "fj0": ctx.host_table("fj0", "<f4"),
        "noscco": ctx.host_table("noscco", "<i4"), "espc": ctx.host_table("espc", "<f4"),
        "espc_cutoff": ctx.host_table("espc_cutoff", "<f4"), "espc_alias": ctx.host_table("espc_alias", "<i2"),
        "source_data": ctx.host_table("source_data"), "detector_data": ctx.host_table("detector_data"),
    }
    nvox = (ctx.geti("num_voxels_x"), ctx.geti("num_voxels_y"), ctx.geti("num_voxels_z"))
    return ol.TableSet(a, nvox, ctx.host_table("inv_voxel_size", "<f4"), ctx.host_table("size_bbox", "<f4"),
                       ctx.geti("num_energy_values"), np.float32(ctx.getf("e0")), np.float32(ctx.getf("ide")),
                       ctx.geti("num_spectrum_bins"))


def measured_z(img_a: np.ndarray, n_a: int, img_b: np.ndarray, w2_b: np.ndarray, n_b: int, min_hits: float = 30.0, w2_a=None):
    """Per-word z-scores between two energy-weighted tallies (units of 0.01 eV) of n_a / n_b histories, with MEASURED
    variances.  A tally word is a sum over histories of a weight w_i (0 for most): its variance per history is
    E[w^2] - E[w]^2.  `w2_b` is the sum of squared weights tallied beside `img_b` (oracle_lib.track_with_variance); sample a
    (the GPU's, which tallies no squares) uses `w2_a` if given.

    Under the hypothesis being tested (same distribution) the best estimate of a word's rate is the POOLED one,
    m = (a + b) / (n_a + n_b), and E[w^2] = m * rho with rho = sum w^2 / sum w the measured mean-square-to-mean weight of
    that word: var(a/n_a - b/n_b) = (m rho - m^2) (1/n_a + 1/n_b).  Pooling matters: a variance taken from sample b alone
    is correlated with b's own fluctuation and biases the mean z by ~1/(2 sqrt(hits)), and a mask on b's hits selects the
    words where b fluctuated up (seen as a -0.09 sigma mean offset over 1.2e4 blocks before this form was used).
    Words expected to hold fewer than `min_hits` effective hits (m n_b / rho) in sample b are masked out.
    Arrays may be block sums (both sums are additive)."""
    a, b, q = img_a.astype(np.float64), img_b.astype(np.float64), np.asarray(w2_b, dtype=np.float64)
    if w2_a is not None:
        q = q + np.asarray(w2_a, dtype=np.float64)
        base = a + b
    else:
        base = b
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(base > 0, q / base, 0.0)
        m = (a + b) / float(n_a + n_b)
        hits = np.where(rho > 0, m * n_b / rho, 0.0)
    var = np.maximum(m * rho - m * m, 0.0) * (1.0 / n_a + 1.0 / n_b)
    mask = (hits >= min_hits) & (var > 0)
    z = np.zeros_like(a)
    z[mask] = (a[mask] / n_a - b[mask] / n_b) / np.sqrt(var[mask])
    return z, mask


def blocks(img: np.ndarray, k: int = 3) -> np.ndarray:
    """Sum [4, nz, nx] tallies over k x k pixel blocks (ragged edges dropped)."""
    c, nz, nx = img.shape
    return img[:, : nz // k * k, : nx // k * k].reshape(c, nz // k, k, nx // k, k).sum(axis=(2, 4))


def class_energy_z(img_a, n_a, img_b, w2_b, n_b):
    """z of the detected energy per history of each scatter class (whole-image sums), measured variances as above;
    NaN for a class the reference sample holds fewer than 200 effective hits of."""
    out = []
    for k in range(img_a.shape[0]):
        z, m = measured_z(np.array([img_a[k].sum(dtype=np.float64)]), n_a, np.array([img_b[k].sum(dtype=np.float64)]),
                          np.array([np.asarray(w2_b[k], dtype=np.float64).sum()]), n_b, min_hits=200.0)
        out.append(float(z[0]) if m[0] else float("nan"))
    return out


# ---- dose tallies
def whole_roi(nvox):
    """The 0-based inclusive ROI that covers a volume of nvox = (nx, ny, nz) voxels."""
    return [0, nvox[0] - 1, 0, nvox[1] - 1, 0, nvox[2] - 1]


def roi6(dose_roi):
    """((x0, x1), (y0, y1), (z0, z1)) in the input file's 1-based inclusive indices -> the engine's 0-based roi6."""
    return [int(v) - 1 for axis in dose_roi for v in axis]


DOSE_STAT_CASES = ["slab_angles", "tissue22", "thorax64"]
WHOLE_ROI_INPUT = ((1, 500), (1, 500), (1, 500))  # clipped to the whole volume


def water_arrays(n):
    """A water box of n = (nx, ny, nz) voxels as set_geometry_arrays takes it."""
    import cases
    shape = (n[2], n[1], n[0])
    return n, (0.4, 0.4, 0.4), np.full(shape, cases.materials.material_number("h2o"), np.uint8), np.ones(shape, np.float32)


def edge_rois(nvox):
    """The fixed sub-ROI of the dose tests, 0-based: one voxel thick in z, reaching the +x face (the single-voxel one follows the tally)."""
    nx, ny, nz = nvox
    return [roi6(((3, nx), (2, ny - 3), (nz // 2, nz // 2)))]


def single_voxel_roi(vox_whole):
    """The ROI of the one voxel with the largest deposit of a whole-volume voxel tally."""
    iz, iy, ix = np.unravel_index(int(np.argmax(vox_whole[..., 0])), vox_whole.shape[:3])
    return [int(ix), int(ix), int(iy), int(iy), int(iz), int(iz)]


def every_projection(ctx):
    return [(p, 42 + 1000 * p) for p in range(ctx.num_projections)]


def _golden_dose(g, tag):
    shape = tuple(int(v) for v in g["dose_voxels_shape"])
    vox = np.zeros(int(np.prod(shape)), dtype=np.uint64)
    vox[g[f"dose_voxels_{tag}_idx"]] = g[f"dose_voxels_{tag}_val"]
    return vox.reshape(shape)


def crop(vox, roi, within):
    """The part of a voxel tally [Dz, Dy, Dx, 2] taken under ROI `within` that lies in the ROI `roi` inside it."""
    x0, y0, z0 = roi[0] - within[0], roi[2] - within[2], roi[4] - within[4]
    return vox[z0:z0 + roi[5] - roi[4] + 1, y0:y0 + roi[3] - roi[2] + 1, x0:x0 + roi[1] - roi[0] + 1]


def oracle_dose(T, roi, runs, nbatch, hpt, math_mode, voxels=True, materials=True, n_threads=8):
    """Fresh oracle tallies over `runs` = [(projection, seed), ...]: (images, voxels uint64[Dz, Dy, Dx, 2] or None, materials
    uint64[25, 2] or None).  Whatever tallies an earlier call attached to `T` are detached."""
    T.dose_voxels = T.dose_materials = None
    T.ct.voxels_edep = T.ct.materials_dose = None
    T.ct.dose_roi = type(T.ct.dose_roi)(32500, -32500, 32500, -32500, 32500, -32500)
    vox, mat = T.enable_dose(roi if voxels else None, materials)
    images = [T.track(p, seed, 0, nbatch, hpt, math_mode, n_threads=n_threads)[0] for p, seed in runs]
    return images, vox, mat


def voxel_sums_per_material(vox, voxel_mat_dens):
    """Row m: the sums of a whole-volume voxel tally [nz, ny, nx, 2] over the voxels that hold material m + 1, from the
    (material, density) pairs of the host table `voxel_mat_dens`: what the material tally [25, 2] has to hold."""
    mat = np.asarray(voxel_mat_dens, dtype=np.float32).reshape(-1, 2)[:, 0].astype(np.int64) - 1
    v = vox.reshape(-1, 2)
    assert mat.size == v.shape[0]
    out = np.zeros((ol.MAXMAT, 2), dtype=np.uint64)
    for m in np.unique(mat):
        out[m] = v[mat == m].sum(axis=0, dtype=np.uint64)
    return out


def _dose_words_z(a, n_a, b, n_b, min_hits):
    """z of tally words [..., 2] = (sum of deposits in 0.01 eV, sum of squared deposits in eV^2) between samples of n_a / n_b
    histories.  Both samples carry their squares, so mean and second moment per history are the POOLED ones (see measured_z for
    why): m = (A + B) / (n_a + n_b) in eV, s = (A2 + B2) / (n_a + n_b) in eV^2, var(a/n_a - b/n_b) = (s - m^2)(1/n_a + 1/n_b).
    Words expected to hold fewer than `min_hits` effective hits (m^2 n / s, n the smaller sample) are masked out."""
    a1, b1 = a[..., 0].astype(np.float64) / 100.0, b[..., 0].astype(np.float64) / 100.0
    a2, b2 = a[..., 1].astype(np.float64), b[..., 1].astype(np.float64)
    n = float(n_a + n_b)
    m, s = (a1 + b1) / n, (a2 + b2) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        hits = np.where(s > 0, m * m * min(n_a, n_b) / s, 0.0)
    var = np.maximum(s - m * m, 0.0) * (1.0 / n_a + 1.0 / n_b)
    mask = (hits >= min_hits) & (var > 0)
    z = np.zeros_like(m)
    z[mask] = (a1[mask] / n_a - b1[mask] / n_b) / np.sqrt(var[mask])
    return z, mask


def dose_blocks(vox: np.ndarray, k: int = 4) -> np.ndarray:
    """Sum a voxel tally [Dz, Dy, Dx, 2] over k x k x k voxel blocks; ragged edges make smaller blocks (nothing is dropped: the
    faces of the volume are where an indexing fault would show)."""
    dz, dy, dx, _ = vox.shape
    pz, py, px = (-dz) % k, (-dy) % k, (-dx) % k
    v = np.pad(vox.astype(np.float64), ((0, pz), (0, py), (0, px), (0, 0)))
    return v.reshape((dz + pz) // k, k, (dy + py) // k, k, (dx + px) // k, k, 2).sum(axis=(1, 3, 5))


def dose_z(vox_a, n_a: int, vox_b, n_b: int, block: int = 4, min_hits: float = 30.0):
    """(z, mask) per block of `block`^3 voxels between two voxel dose tallies of n_a / n_b histories, measured variances: block
    sums of column 0 (sum of deposits, 0.01 eV) and column 1 (sum of squared deposits, eV^2) of both samples.  The squares are
    those of single deposits, as the reference tallies them for its own 2-sigma report (K.cu:418-443)."""
    return _dose_words_z(dose_blocks(vox_a, block), n_a, dose_blocks(vox_b, block), n_b, min_hits)


def dose_material_z(mat_a, n_a: int, mat_b, n_b: int, min_hits: float = 200.0):
    """(z, mask) per row of two material dose tallies [25, 2], as dose_z."""
    return _dose_words_z(np.asarray(mat_a), n_a, np.asarray(mat_b), n_b, min_hits)


def dose_figures(vox_a, mat_a, n_a, vox_b, mat_b, n_b, block=4):
    """The figures the dose criteria are about, of two samples (voxel tally, material tally, histories)."""
    z, mask = dose_z(vox_a, n_a, vox_b, n_b, block)
    zm, mm = dose_material_z(mat_a, n_a, mat_b, n_b)
    zz = z[mask]
    return dict(blocks=int(mask.sum()), frac3=float(np.mean(np.abs(zz) > 3.0)) if zz.size else 0.0,
                zmax=float(np.abs(zz).max()) if zz.size else 0.0, zmean=float(zz.mean()) if zz.size else 0.0,
                materials=int(mm.sum()), mat_zmax=float(np.abs(zm[mm]).max()) if mm.any() else 0.0)


def dose_criteria_missed(fig):
    """The criteria of test_fast_kernel_within_3_sigma_of_oracle, on the dose tallies: at least 50 blocks in the mask, fewer than
    1 % of them beyond 3 sigma, none beyond 6, |mean z| < 0.25; every material of at least 200 effective hits within 3.5 sigma.
    Returns the names of those `fig` misses (none: the samples agree)."""
    missed = []
    if fig["blocks"] < 50: missed.append("blocks")
    if not fig["frac3"] < 0.01: missed.append("frac3")
    if not fig["zmax"] < 6.0: missed.append("zmax")
    if not abs(fig["zmean"]) < 0.25: missed.append("zmean")
    if fig["materials"] < 1 or not fig["mat_zmax"] < 3.5: missed.append("materials")
    return missed


_DOSE_SAMPLES = {}


def oracle_dose_sample(ctx, name, seed, nbatch=3000, hpt=150):
    """(voxels, materials, histories) of the libm oracle on the last projection of case `name`, the whole volume as ROI: the
    reference sample of the statistical dose tests, computed once per (case, seed) and left unchanged."""
    key = (name, seed, nbatch, hpt)
    if key not in _DOSE_SAMPLES:
        T = tables_from_context(ctx)
        _, vox, mat = oracle_dose(T, whole_roi(T.num_voxels), [(ctx.num_projections - 1, seed)], nbatch, hpt, ol.MATH_LIBM)
        vox.setflags(write=False)
        mat.setflags(write=False)
        _DOSE_SAMPLES[key] = (vox, mat, nbatch * hpt)
    return _DOSE_SAMPLES[key]
