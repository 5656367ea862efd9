"""CPU tests of the per-pixel variance: the host finalize against a numpy restatement of its formula, bit for bit, and the scan
options that carry `write_variance` (refusals by name, the struct's layout, a caller compiled before the field existed)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mcgpu_amd.h"
W_MAX = 12_500_000  # 125 keV in 0.01 eV


def variance_planes(ctx, image, w2, n, crop_nx=0):
    """mcgpu_finalize_variance restated in numpy float64: per pixel and plane group {total, unscattered, scattered}, with W / Q the
    integer sums of the group's image / w2 words, var = c^2 (2^20 Q - W W / N) / (N (N - 1)) evaluated left to right, negative -> 0,
    N < 2 -> 0, cast to float32; rows flipped, columns cropped."""
    nz, nx = ctx.detector_shape
    cx = crop_nx if 0 < crop_nx < nx else nx
    t = np.asarray(image, dtype=np.uint64).reshape(4, nz, nx)
    q = np.asarray(w2, dtype=np.uint64).reshape(4, nz, nx)
    c = 0.01 * ctx.getf("inv_pixel_size_x") * ctx.getf("inv_pixel_size_z")
    ws, qs = t[1] + t[2] + t[3], q[1] + q[2] + q[3]
    out = np.zeros((3, nz, cx), dtype=np.float32)
    if n >= 2:
        nd = float(n)
        for k, (W, Q) in enumerate(((t[0] + ws, q[0] + qs), (t[0], q[0]), (ws, qs))):
            W, Q = W.astype(np.float64), Q.astype(np.float64)
            var = c * c * (1048576.0 * Q - W * W / nd) / (nd * (nd - 1.0))
            out[k] = np.where(var > 0.0, var, 0.0).astype(np.float32)[::-1, :cx]
    return out


def random_tallies(ctx, rng, n_hist):
    """Tallies as a launch of n_hist histories could leave them: per word h hits (most words few, some none) of weights in
    [5e5, W_MAX]; image = their sum, w2 = the sum of (w >> 10)^2."""
    nz, nx = ctx.detector_shape
    hits = rng.poisson(n_hist / (8.0 * nz * nx), size=(4, nz, nx))
    image = np.zeros((4, nz, nx), dtype=np.uint64)
    w2 = np.zeros((4, nz, nx), dtype=np.uint64)
    for _ in range(int(hits.max())):
        w = rng.integers(500_000, W_MAX + 1, size=hits.shape, dtype=np.uint64)
        live = hits > 0
        image += np.where(live, w, 0).astype(np.uint64)
        w2 += np.where(live, (w >> np.uint64(10)) ** 2, 0).astype(np.uint64)
        hits = hits - live
    return image, w2


def test_host_finalize_equals_the_formula_bit_for_bit(engine, case_dir):
    rng = np.random.default_rng(20261017)
    with engine.create(case_dir("air"), device=-1) as ctx:
        nz, nx = ctx.detector_shape
        n = 400_000
        image, w2 = random_tallies(ctx, rng, n)
        assert int(np.count_nonzero(image)) > 1000 and int(np.count_nonzero(image == 0)) > 1000
        # a pixel where the clamp bites at N = 2: both histories score the same weight, the spread is zero and the bits the shift
        # dropped leave 2^20 Q below W^2 / N
        image[:, 5, 7] = (2 * W_MAX, 0, 0, 0)
        w2[:, 5, 7] = (2 * (W_MAX >> 10) ** 2, 0, 0, 0)
        for crop in (0, nx - 100, nx, nx + 9):  # full width, smaller than, equal to and larger than Nx
            got = ctx.finalize_variance_host(image, w2, n, crop_nx=crop)
            want = variance_planes(ctx, image, w2, n, crop)
            assert got.dtype == np.float32 and got.shape == want.shape == (3, nz, crop if 0 < crop < nx else nx)
            assert got.tobytes() == want.tobytes(), crop
        assert float(got[0].max()) > 0.0
        # scattered = classes 1..3 summed as integers, unscattered = class 0, z flipped
        one = np.zeros_like(image)
        one[2, 3, 4] = image[2, 3, 4] or 777_777
        sq = np.zeros_like(w2)
        sq[2, 3, 4] = (int(one[2, 3, 4]) >> 10) ** 2
        v = ctx.finalize_variance_host(one, sq, 1000)
        assert v[0, nz - 1 - 3, 4] == v[2, nz - 1 - 3, 4] > 0 and v[1, nz - 1 - 3, 4] == 0 and np.count_nonzero(v) == 2
        # the clamp
        two = ctx.finalize_variance_host(image, w2, 2)
        assert 1048576.0 * float(2 * (W_MAX >> 10) ** 2) - float(2 * W_MAX) ** 2 / 2.0 < 0.0
        assert two[1, nz - 1 - 5, 7] == 0.0 and two[0, nz - 1 - 5, 7] == 0.0
        assert two.tobytes() == variance_planes(ctx, image, w2, 2).tobytes()
        # N = 1 and N = 0: no variance from one history
        for few in (1, 0):
            assert not ctx.finalize_variance_host(image, w2, few).any() and not variance_planes(ctx, image, w2, few).any()
        # Q = 0 (an image without squares): every term is negative or zero
        zero = ctx.finalize_variance_host(image, np.zeros_like(w2), n)
        assert not zero.any() and zero.tobytes() == variance_planes(ctx, image, np.zeros_like(w2), n).tobytes()


def test_variance_is_the_unbiased_sample_variance_of_the_plane_value(engine, case_dir):
    """The formula against its meaning, on explicit per-history scores without truncation (weights that are multiples of 1024):
    numpy's var(ddof=1) of the per-history pixel value, over N."""
    with engine.create(case_dir("air"), device=-1) as ctx:
        nz, nx = ctx.detector_shape
        c = 0.01 * ctx.getf("inv_pixel_size_x") * ctx.getf("inv_pixel_size_z")
        n = 5000
        rng = np.random.default_rng(3)
        w = np.where(rng.random(n) < 0.3, rng.integers(500, 12_000, size=n) * 1024, 0).astype(np.uint64)
        image = np.zeros((4, nz, nx), dtype=np.uint64)
        w2 = np.zeros_like(image)
        image[0, 10, 20] = w.sum()
        w2[0, 10, 20] = ((w >> np.uint64(10)) ** 2).sum()
        got = float(ctx.finalize_variance_host(image, w2, n)[0, nz - 1 - 10, 20])
        want = np.var(c * w.astype(np.float64), ddof=1) / n
        assert abs(got - want) <= 1e-6 * want, (got, want)


def variance_ratio(W_runs, Q_runs, n, min_hits=200.0, block=8):
    """rho = sum_b s_b^2 / sum_b n sigma_b^2 over the block x block pixel blocks of the TOTAL image (the four classes summed; ragged
    edges dropped) that expect at least `min_hits` effective hits per run, and the number of those blocks.  W_runs, Q_runs:
    uint64 [M, 4, nz, nx], the image and w2 of M independent runs of n histories.  s_b^2 is the sample variance of the block sum over
    the runs; sigma_b^2 = E[w^2] - E[w]^2 the per-history variance from the pooled W, 2^20 Q and M n; the effective hits a run
    expects are W^2 / (2^20 Q M) of the pooled sums."""
    m = W_runs.shape[0]

    def blocks(a):
        t = a.sum(axis=1, dtype=np.uint64)
        _, nz, nx = t.shape
        k = block
        return t[:, :nz // k * k, :nx // k * k].reshape(m, nz // k, k, nx // k, k).sum(axis=(2, 4), dtype=np.uint64).astype(np.float64)

    Wb, Qb = blocks(W_runs), blocks(Q_runs) * 1048576.0
    Wp, Qp = Wb.sum(axis=0), Qb.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        hits = np.where(Qp > 0, Wp * Wp / (m * Qp), 0.0)
    mask = hits >= min_hits
    s2 = Wb.var(axis=0, ddof=1)
    sigma2 = Qp / (m * n) - (Wp / (m * n)) ** 2
    return float(s2[mask].sum() / (n * sigma2[mask]).sum()), int(mask.sum())


def variance_ratio_bound(blocks, m):
    """Five standard deviations of a variance ratio with blocks * (m - 1) degrees of freedom, plus the 0.5 % the shift in w2 can drop."""
    return 5.0 * np.sqrt(2.0 / (blocks * (m - 1))) + 0.005


def test_variance_ratio_on_the_oracle():
    """The statistic of the GPU suite's "the variance is the variance" with the CPU oracle in place of the kernel: 32 runs of
    1334 x 150 histories of the `air` case (disjoint batch ranges of one seed).  It passes as it is (rho = 0.9514 over 192 blocks,
    bound 0.0967) and fails with w2 doubled (0.4746) or halved (1.9116)."""
    import tempfile
    import cases
    import oracle_lib as ol
    import parity
    m, nbatch, hpt = 32, 1334, 150
    with tempfile.TemporaryDirectory() as tmp:
        with cases.pkg.engine.create(cases.build_case("air", tmp), device=-1) as ctx:
            T = parity.tables_from_context(ctx)
            shape = (4,) + ctx.detector_shape
    W, Q = np.zeros((m,) + shape, dtype=np.uint64), np.zeros((m,) + shape, dtype=np.uint64)
    for r in range(m):
        img, _ = T.track(0, 4242, r * nbatch, nbatch, hpt, ol.MATH_LIBM, n_threads=8, w2=Q[r].reshape(-1))
        W[r] = img.reshape(shape)
    rho, blocks = variance_ratio(W, Q, nbatch * hpt)
    bound = variance_ratio_bound(blocks, m)
    print(f"oracle air: rho = {rho:.4f} over B = {blocks} blocks, bound {bound:.4f}")
    assert blocks >= 100 and abs(rho - 1.0) <= bound, (rho, blocks, bound)
    doubled, _ = variance_ratio(W, 2 * Q, nbatch * hpt)
    halved, _ = variance_ratio(W, Q // 2, nbatch * hpt)
    assert abs(doubled - 1.0) > bound and abs(halved - 1.0) > bound, (doubled, halved)


def _options(engine, **fields):
    o = engine.ScanOptions()
    o.struct_size = C.sizeof(engine.ScanOptions)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def test_scan_refuses_variance_it_cannot_write(engine, case_dir):
    """write_variance without write_stacks, with shared_stacks, and through mcgpu_run_scan_multi: -1 and a message that names the
    field, before the context's device is looked at (a host-only context gets the same answers)."""
    lib = engine.load_library()
    r = engine.ScanReport()
    with engine.create(case_dir("air"), device=-1) as ctx:
        o = _options(engine, write_variance=1, write_stacks=0)
        assert lib.mcgpu_run_scan(ctx.h, C.byref(o), C.byref(r)) == -1
        msg = lib.mcgpu_last_error().decode()
        assert "write_variance" in msg and "write_stacks" in msg and "no device" not in msg, msg
        stacks = (C.c_void_p * 3)(1, 2, 3)  # never dereferenced: the call is refused first
        slices = (C.c_int * 1)(0)
        o = _options(engine, write_variance=1, write_stacks=1, shared_stacks=stacks, slice_of_projection=slices)
        assert lib.mcgpu_run_scan(ctx.h, C.byref(o), C.byref(r)) == -1
        msg = lib.mcgpu_last_error().decode()
        assert "write_variance" in msg and "shared_stacks" in msg and "no device" not in msg, msg
        o = _options(engine, write_variance=1, write_stacks=1)
        hs = (C.c_void_p * 1)(ctx.h)
        assert lib.mcgpu_run_scan_multi(hs, 1, C.byref(o), C.byref(r)) == -1
        msg = lib.mcgpu_last_error().decode()
        assert "write_variance" in msg and "mcgpu_run_scan_multi" in msg and "no device" not in msg, msg
        # an acceptable combination gets as far as the device check
        assert lib.mcgpu_run_scan(ctx.h, C.byref(o), C.byref(r)) != 0
        assert "no device" in lib.mcgpu_last_error().decode()
        with pytest.raises(engine.EngineError) as e:
            ctx.run_scan(write_variance=True, write_stacks=False)
        assert e.value.code == -1 and "write_variance" in e.value.message


def test_a_struct_that_ends_before_write_variance_reads_it_as_zero(engine, case_dir):
    """A caller compiled against the header before `write_variance` passes struct_size = its offset: whatever follows the shorter
    struct in memory is not looked at -- the scan is not refused for the variance (no write_stacks here), it goes on to the device
    check."""
    lib = engine.load_library()
    r = engine.ScanReport()
    with engine.create(case_dir("air"), device=-1) as ctx:
        o = _options(engine, write_variance=1, write_stacks=0)
        o.struct_size = engine.ScanOptions.write_variance.offset
        assert lib.mcgpu_run_scan(ctx.h, C.byref(o), C.byref(r)) != 0
        msg = lib.mcgpu_last_error().decode()
        assert "no device" in msg and "write_variance" not in msg, msg
        o.struct_size = C.sizeof(engine.ScanOptions)
        assert lib.mcgpu_run_scan(ctx.h, C.byref(o), C.byref(r)) == -1
        assert "write_variance" in lib.mcgpu_last_error().decode()


def test_scan_options_layout_is_the_headers(engine):
    """Field names in the header's order, `write_variance` appended after `reduce`, and the size the C layout rules give."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct mcgpu_scan_options \{(.*?)\} mcgpu_scan_options;", text, re.S).group(1)
    names = []
    for decl in body.split(";"):
        parts = [p.replace("*", " ").split() for p in decl.split(",")]
        if parts[0]:
            names += [parts[0][-1]] + [p[0] for p in parts[1:]]
    fields = [f[0] for f in engine.ScanOptions._fields_]
    assert names == fields and fields[-2:] == ["reduce", "write_variance"] and fields[0] == "struct_size"
    assert engine.ScanOptions.write_variance.offset == engine.ScanOptions.reduce.offset + 4
    assert engine.ScanOptions.write_variance.size == 4
    assert C.sizeof(engine.ScanOptions) % 8 == 0 and C.sizeof(engine.ScanOptions) >= engine.ScanOptions.write_variance.offset + 4
    assert engine.load_library().mcgpu_abi_version() == 1
