"""The tally of squared weights beside the detector image (mcgpu_launch_projection_w2) and the variance planes made from it.

w2[i] is the sum of (w >> 10)^2 over the histories that scored w in word i.  Exact tests: COMPAT against the CPU oracle word for
word; the image untouched in every mode; every FAST route (direct atomics, staged records folded, the full-block fallback,
sub-launches, both schedulers) the same w2; sharding and accumulation; support and bounds per word; the device finalize against
its host twin; the scan's variance stacks.  Statistical tests: the variance that w2 gives is the variance seen over repeated
launches, and FAST's second moments per scatter class agree with the libm oracle's."""
import numpy as np
import pytest

import oracle_lib as ol
import parity
from test_tally_variance import variance_ratio, variance_ratio_bound

pytestmark = pytest.mark.gpu

KNOBS = ("MCGPU_TALLY_STAGE", "MCGPU_TALLY_STAGE_CAP", "MCGPU_TALLY_STAGE_MAX_HISTORIES")
W_MIN, W_MAX = 500_000, 12_500_000  # 5 keV (the tables' floor) and 125 keV in 0.01 eV


def _set(ctx, monkeypatch, **env):
    """The staging knobs as given, all others unset (the default: a launch with w2 stages wherever the detector has a plan)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx.reload_env_knobs()


# ---------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("name,p,nbatch", [("air", 0, 256), ("water", 0, 512), ("catphan64", 0, 512), ("slab_angles", 1, 512), ("cirs76", 2, 384)])
def test_compat_w2_is_the_oracles_word_for_word(engine, case_dir, name, p, nbatch):
    """1. slab_angles projection 1 (300.5 degrees) is a rotated detector pose, cirs76 projection 2 (240 degrees) another."""
    with engine.create(case_dir(name), device=0) as ctx:
        T = parity.tables_from_context(ctx)
        seed = 42 + 1000 * p
        want_w2 = np.zeros(T.image_size(), dtype=np.uint64)
        want_img, _ = T.track(p, seed, 0, nbatch, 150, ol.MATH_PORTABLE, n_threads=8, w2=want_w2)
        img, w2, _, done = ctx.run_projection_with_variance(p, nbatch, mode="compat", seed=seed, hpt=150)
        plain, _, _ = ctx.run_projection(p, nbatch, mode="compat", seed=seed, hpt=150)
        assert done == nbatch * 150 and int(want_w2.sum()) > 0
        assert np.array_equal(plain.reshape(-1), want_img) and np.array_equal(img, plain)
        bad = np.count_nonzero(w2.reshape(-1) != want_w2)
        assert bad == 0, f"{name} projection {p}: {bad} words of w2 differ from the oracle's"
        if name == "slab_angles":
            assert int(T.detector[p]["rotation_flag"]) == 1


@pytest.mark.parametrize("mode,count,hpt", [("fast", 300_000, None), ("fast64", 300_000, None), ("compat", 300, 150)])
def test_image_of_a_launch_with_w2_is_the_image_without(engine, case_dir, monkeypatch, mode, count, hpt):
    """2. In every mode; FAST with the default routes (w2 staged, plain by the rule) and with both forced to the direct atomics."""
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        for env in ({}, {"MCGPU_TALLY_STAGE": 0}):
            _set(ctx, monkeypatch, **env)
            plain, _, _ = ctx.run_projection(0, count, mode=mode, seed=9, hpt=hpt)
            img, w2, _, _ = ctx.run_projection_with_variance(0, count, mode=mode, seed=9, hpt=hpt)
            assert np.array_equal(img, plain) and int(plain.sum()) > 0 and int(w2.sum()) > 0, env
        _set(ctx, monkeypatch)


def test_a_launch_with_w2_stages_where_the_default_rule_keeps_the_atomics(engine, case_dir, monkeypatch):
    """The water box has no exterior bricks: plain launches take the direct atomics (tally_stage_bins 0), a launch with w2 stages
    anyway -- and MCGPU_TALLY_STAGE=0 still forces it onto the atomics."""
    with engine.create(case_dir("water"), device=0) as ctx:
        _set(ctx, monkeypatch)
        assert ctx.geti("tally_stage_bins") == 0
        ctx.run_projection(0, 50_000, mode="fast", seed=3)
        assert ctx.geti("tally_stage_staged_hits") == 0
        img, w2, _, _ = ctx.run_projection_with_variance(0, 50_000, mode="fast", seed=3)
        staged = ctx.geti("tally_stage_staged_hits")
        assert 0 < staged <= 50_000 and int(w2.sum()) > 0
        _set(ctx, monkeypatch, MCGPU_TALLY_STAGE=0)
        f0 = ctx.geti("tally_stage_fallback_hits")
        img0, w20, _, _ = ctx.run_projection_with_variance(0, 50_000, mode="fast", seed=3)
        assert ctx.geti("tally_stage_fallback_hits") == f0
        assert np.array_equal(img0, img) and np.array_equal(w20, w2)
        _set(ctx, monkeypatch)


@pytest.mark.parametrize("sched", [0, 1])
@pytest.mark.parametrize("mode", ["fast", "fast64"])
def test_fast_routes_give_one_w2(engine, case_dir, monkeypatch, mode, sched):
    """3. The direct atomics are the reference; staged, nearly everything through the full-block fallback, three and more
    sub-launches, a launch smaller than a workgroup, two threshold presets -- and both schedulers (the parameter)."""
    monkeypatch.setenv("MCGPU_FAST_SCHED", str(sched))
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        assert ctx.geti("fast_scheduler") == sched
        n = 300_000
        _set(ctx, monkeypatch, MCGPU_TALLY_STAGE=0)
        ref_img, ref, _, _ = ctx.run_projection_with_variance(0, n, mode=mode, seed=11)
        small_img, small, _, _ = ctx.run_projection_with_variance(0, 63, mode=mode, seed=11, first=17)
        for k in range(4):
            assert int(np.count_nonzero(ref[k])) > 0, k
        assert int(small.sum()) > 0
        for env, what in (({"MCGPU_TALLY_STAGE": 1}, "staged"), ({}, "default"), ({"MCGPU_TALLY_STAGE_CAP": 2}, "fallback"),
                          ({"MCGPU_TALLY_STAGE_MAX_HISTORIES": 70_001}, "sub-launches")):
            _set(ctx, monkeypatch, **env)
            f0 = ctx.geti("tally_stage_fallback_hits")
            img, w2, _, done = ctx.run_projection_with_variance(0, n, mode=mode, seed=11)
            fell = ctx.geti("tally_stage_fallback_hits") - f0
            assert done == n and np.array_equal(img, ref_img), what
            assert np.array_equal(w2, ref), f"{what}: {np.count_nonzero(w2 != ref)} words of w2 differ"
            if what == "fallback":
                assert fell > ctx.geti("tally_stage_staged_hits") > 0, what  # almost every hit fell back, some were staged
            elif what in ("staged", "default"):
                assert fell == 0 and ctx.geti("tally_stage_staged_hits") > 0, what
            img, w2, _, _ = ctx.run_projection_with_variance(0, 63, mode=mode, seed=11, first=17)
            assert np.array_equal(img, small_img) and np.array_equal(w2, small), what
        assert engine.tally_stage_plan(ctx.image_words, n, 512, limit=70_001)["sub_launches"] >= 3
        _set(ctx, monkeypatch)
        if sched == 0:  # the threshold presets belong to the per-wave scheduler
            for preset in ((32, 8, 36, 12, 40), (36, 16, 44, 12, 44)):
                assert ctx.lib.mcgpu_set_fast_schedule(ctx.h, *preset) == 0
                img, w2, _, _ = ctx.run_projection_with_variance(0, n, mode=mode, seed=11)
                assert np.array_equal(img, ref_img) and np.array_equal(w2, ref), preset


@pytest.mark.parametrize("mode,total,hpt", [("fast", 240_000, None), ("compat", 400, 150)])
def test_shards_sum_and_launches_accumulate(engine, case_dir, monkeypatch, mode, total, hpt):
    """4. Disjoint ranges sum to the whole; a second launch into a w2 that holds a first adds to it."""
    import torch
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        _set(ctx, monkeypatch)
        whole_img, whole, _, _ = ctx.run_projection_with_variance(0, total, mode=mode, seed=5, hpt=hpt)
        cuts = [0, total // 3 + 1, total // 2, total]
        parts = [ctx.run_projection_with_variance(0, b - a, mode=mode, seed=5, first=a, hpt=hpt) for a, b in zip(cuts, cuts[1:])]
        assert all(int(p[1].sum()) > 0 for p in parts)
        assert np.array_equal(sum(p[1] for p in parts), whole) and np.array_equal(sum(p[0] for p in parts), whole_img)
        img_dev = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        w2_dev = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        for a, b in zip(cuts, cuts[1:]):
            ctx.launch(0, img_dev.data_ptr(), b - a, mode=mode, seed=5, first=a, hpt=hpt, w2_dev_ptr=w2_dev.data_ptr())
        assert np.array_equal(ctx.download_image(w2_dev.data_ptr()), whole) and np.array_equal(ctx.download_image(img_dev.data_ptr()), whole_img)
        ctx.launch(0, img_dev.data_ptr(), cuts[1], mode=mode, seed=5, hpt=hpt, w2_dev_ptr=w2_dev.data_ptr())  # the first range again
        assert np.array_equal(ctx.download_image(w2_dev.data_ptr()), whole + parts[0][1])
        assert np.array_equal(ctx.download_image(img_dev.data_ptr()), whole_img + parts[0][0])
        ctx.launch(0, img_dev.data_ptr(), cuts[1], mode=mode, seed=5, hpt=hpt)  # ... and without w2: only the image moves
        assert np.array_equal(ctx.download_image(w2_dev.data_ptr()), whole + parts[0][1])
        assert np.array_equal(ctx.download_image(img_dev.data_ptr()), whole_img + 2 * parts[0][0])


@pytest.mark.parametrize("mode,count,hpt", [("fast", 200_000, None), ("fast64", 200_000, None), ("compat", 256, 150)])
def test_support_and_bounds_per_word(engine, case_dir, monkeypatch, mode, count, hpt):
    """5. w2 > 0 exactly where the image is; 2^20 w2 <= image * w_max (every term (w >> 10)^2 2^20 <= w^2 <= w w_max); and where
    plane 3 holds a single hit for certain (image < 2 w_min) w2 is that hit's term.  With the filtered 125 kVp spectrum of the cases
    no detected photon is below 22 keV (the CPU oracle's smallest word over 2e6 histories of water: 2 208 088), so no word is
    below 2 w_min = 1e6 and that last check selects nothing; test_single_history_launches states it on words that hold one hit
    by construction."""
    with engine.create(case_dir("water"), device=0) as ctx:
        _set(ctx, monkeypatch)
        img, w2, _, _ = ctx.run_projection_with_variance(0, count, mode=mode, seed=21, hpt=hpt)
        assert np.array_equal(w2 > 0, img > 0) and int(np.count_nonzero(img)) > 1000
        lhs = [int(q) << 20 for q in w2.reshape(-1)]
        rhs = [int(w) * W_MAX for w in img.reshape(-1)]
        assert all(a <= b for a, b in zip(lhs, rhs))
        single = (img[3] > 0) & (img[3] < 2 * W_MIN)
        assert np.array_equal(w2[3][single], (img[3][single] >> np.uint64(10)) ** 2)
        assert int(img[3].max()) >= 2 * W_MIN and int(np.count_nonzero(img[3])) > 100


@pytest.mark.parametrize("mode,launches", [("fast", 2000), ("fast64", 300), ("compat", 300)])
def test_single_history_launches(engine, case_dir, monkeypatch, mode, launches):
    """5, on words that hold a single hit by construction: a launch of one history scores in one word at most, and there
    w2 == (image >> 10)^2; the launches add up to the w2 of the range (FAST; COMPAT: batch b of one history is not history b of a
    longer batch).  Among the 2000 FAST histories some score in plane 3."""
    with engine.create(case_dir("water"), device=0) as ctx:
        _set(ctx, monkeypatch)
        hpt = 1 if mode == "compat" else None
        total_img, total_w2, per_plane = 0, 0, np.zeros(4, dtype=int)
        for i in range(launches):
            img, w2, _, done = ctx.run_projection_with_variance(0, 1, mode=mode, seed=21, first=i, hpt=hpt)
            hit = np.flatnonzero(img.reshape(-1))
            assert done == 1 and hit.size <= 1 and np.array_equal(np.flatnonzero(w2.reshape(-1)), hit), i
            if hit.size:
                w = int(img.reshape(-1)[hit[0]])
                assert W_MIN <= w <= W_MAX and int(w2.reshape(-1)[hit[0]]) == (w >> 10) ** 2, (i, w)
                per_plane[hit[0] // (img.size // 4)] += 1
            total_img, total_w2 = total_img + img, total_w2 + w2
        print(f"{mode}: hits per plane of {launches} single-history launches: {per_plane.tolist()}")
        assert per_plane.sum() > launches // 10
        if mode != "compat":
            img, w2, _, _ = ctx.run_projection_with_variance(0, launches, mode=mode, seed=21)
            assert np.array_equal(img, total_img) and np.array_equal(w2, total_w2)
        if mode == "fast":
            assert per_plane[3] > 0 and per_plane[0] > 0


def test_device_finalize_is_the_host_twin(engine, case_dir, monkeypatch):
    """6. mcgpu_finalize_variance == mcgpu_finalize_variance_host bit for bit on a real tally; clear_w2 zeroes w2 alone."""
    import torch
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        _set(ctx, monkeypatch)
        nz, nx = ctx.detector_shape
        n = 300_000
        img_dev = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        w2_dev = torch.zeros(ctx.image_words, dtype=torch.int64, device="cuda:0")
        ctx.launch(0, img_dev.data_ptr(), n, mode="fast", seed=6, w2_dev_ptr=w2_dev.data_ptr())
        img, w2 = ctx.download_image(img_dev.data_ptr()), ctx.download_image(w2_dev.data_ptr())
        assert int(w2.sum()) > 0
        for crop, hist in ((0, n), (128, n), (nx, n), (nx + 5, n), (100, 2), (100, 1)):
            cx = crop if 0 < crop < nx else nx
            planes = torch.full((3, nz, cx), -1.0, dtype=torch.float32, device="cuda:0")
            ctx.finalize_variance_device(img_dev.data_ptr(), w2_dev.data_ptr(), hist, planes.data_ptr(), crop_nx=crop)
            torch.cuda.synchronize()
            want = ctx.finalize_variance_host(img, w2, hist, crop_nx=crop)
            assert planes.cpu().numpy().tobytes() == want.tobytes(), (crop, hist)
        assert float(want.max()) == 0.0  # one history: no variance
        assert np.array_equal(ctx.download_image(w2_dev.data_ptr()), w2)
        planes = torch.zeros((3, nz, nx), dtype=torch.float32, device="cuda:0")
        ctx.finalize_variance_device(img_dev.data_ptr(), w2_dev.data_ptr(), n, planes.data_ptr(), clear_w2=True)
        torch.cuda.synchronize()
        got = planes.cpu().numpy()
        assert got.tobytes() == ctx.finalize_variance_host(img, w2, n).tobytes() and float(got[0].max()) > 0 and float(got[2].max()) > 0
        assert int(w2_dev.abs().sum().item()) == 0 and np.array_equal(ctx.download_image(img_dev.data_ptr()), img)


def test_scan_writes_the_variance_stacks_and_leaves_the_rest(engine, case_dir, tmp_path, monkeypatch):
    """7. One scan of catphan64 with write_variance: the three variance stacks are finalize_variance_host of the tallies of
    run_projection_with_variance at the scan's seed; stacks and ASCII data of a scan without the option are the same bytes."""
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        _set(ctx, monkeypatch)
        n, crop = 300_000, 200
        seed = ctx.geti("seed")
        plain, var = tmp_path / "plain", tmp_path / "variance"
        for folder, flag in ((plain, False), (var, True)):
            folder.mkdir()
            rep = ctx.run_scan(mode="fast", histories=n, crop_nx=crop, write_ascii=False, output_folder=folder, write_variance=flag)
            assert rep["projections"] == 1 and rep["histories_per_projection"] == n
        names = ("total", "unscattered", "scattered")
        for m in names:
            assert (var / f"projections_{m}.mha").read_bytes() == (plain / f"projections_{m}.mha").read_bytes(), m
            assert not (plain / f"projections_{m}_variance.mha").exists()
        img, w2, _, _ = ctx.run_projection_with_variance(0, n, mode="fast", seed=seed)
        want = ctx.finalize_variance_host(img, w2, n, crop_nx=crop)
        for k, m in enumerate(names):
            got = engine.stack_read(var / f"projections_{m}_variance.mha")
            assert got.shape == (1,) + want[k].shape and got[0].tobytes() == want[k].tobytes(), m
        assert float(want[0].max()) > 0 and int(np.count_nonzero(want[2] == 0)) > 0  # zeros stay zeros: no replacement
        mean = engine.stack_read(var / "projections_total.mha")[0]
        header = lambda f: f.read_bytes().split(b"ElementDataFile")[0]
        assert header(var / "projections_total_variance.mha") == header(var / "projections_total.mha")  # same size and spacing
        assert mean.shape == want[0].shape
        # the ASCII files: a scan with both outputs against the plain tally's file
        both = tmp_path / "both"
        both.mkdir()
        ctx.run_scan(mode="fast", histories=n, crop_nx=crop, write_ascii=True, output_folder=both, write_variance=True)
        ref_file = tmp_path / "ref_ascii"
        ctx.write_projection(0, img, n, file_name=str(ref_file))
        data = lambda f: [l for l in open(f).read().rstrip("\n").split("\n") if not l.startswith("#")]
        assert data(ctx.projection_file_name(0)) == data(ref_file)
        assert (both / "projections_total_variance.mha").read_bytes() == (var / "projections_total_variance.mha").read_bytes()


# ---------------------------------------------------------------------------------------------------------------- statistical
def test_the_variance_is_the_variance(engine, case_dir, monkeypatch):
    """8. M = 32 FAST launches of `air` with different seeds, N = 200 100 histories each.  Over the 8 x 8 pixel blocks of the total
    image that expect at least 200 hits per launch, rho = sum_b s_b^2 / sum_b N sigma_b^2 (s_b^2: sample variance of the block sum
    over the launches; sigma_b^2: per-history variance from the pooled W, Q and M N) must lie within
    5 sqrt(2 / (B (M - 1))) + 0.005 of 1: five standard deviations of a variance ratio with B (M - 1) degrees of freedom, plus the
    bound on what the shift in w2 drops.

    Rehearsed with the libm oracle in place of the kernel (32 batch ranges of 1334 x 150 histories of seed 4242;
    tests/test_tally_variance.py keeps that run): rho = 0.9514 over B = 192 blocks, bound 0.0967; with w2 doubled rho = 0.4746, halved
    1.9116 -- both fail.  Ten such oracle ensembles gave rho = 0.996 +- 0.022.
    FAST on the MI355X (seeds 1000 .. 1031): rho = 1.0019 over B = 192 blocks, bound 0.0967."""
    m_runs, n = 32, 200_100
    with engine.create(case_dir("air"), device=0) as ctx:
        _set(ctx, monkeypatch)
        runs = [ctx.run_projection_with_variance(0, n, mode="fast", seed=1000 + r) for r in range(m_runs)]
    W, Q = np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])
    rho, blocks = variance_ratio(W, Q, n)
    bound = variance_ratio_bound(blocks, m_runs)
    print(f"FAST air: rho = {rho:.4f} over B = {blocks} blocks, bound {bound:.4f}")
    assert blocks >= 100
    assert abs(rho - 1.0) <= bound, (rho, blocks, bound)


# |dR_k| / R_k between two libm-oracle runs of `water` at 13 000 x 150 = 1.95e6 histories, largest of six pairs of seeds
# (777 + 1000 r, r = 0 .. 11, paired (0, 1), (2, 3), ...), per scatter class: measured 0.00099, 0.01043, 0.01479, 0.00832.
# Times 3, because six pairs only sample the spread.
ORACLE_SPREAD = (0.00099, 0.01043, 0.01479, 0.00832)
R_TOLERANCE = tuple(3.0 * s for s in ORACLE_SPREAD)


def _class_ratio(img, w2):
    """R_k = sum Q_k / sum W_k per scatter class: the energy-weighted mean energy, in units of 2^20 / 100 eV."""
    return w2.reshape(4, -1).sum(axis=1).astype(np.float64) / img.reshape(4, -1).sum(axis=1).astype(np.float64)


def test_fast_second_moments_agree_with_the_oracle(engine, case_dir, monkeypatch):
    """9. R_k of FAST against the libm oracle at equal histories, per scatter class, within three times the spread the oracle
    shows against itself (ORACLE_SPREAD).  A w2 built with a shift of 9 or 11 is four times / a quarter of this one up to the
    dropped bits: both must miss the tolerance in every class.
    Measured on the MI355X: |dR_k| / R_k = 0.00016, 0.00058, 0.00109, 0.00030 against tolerances of 0.00297, 0.03129, 0.04437, 0.02496."""
    nbatch, hpt = 13_000, 150
    n = nbatch * hpt
    with engine.create(case_dir("water"), device=0) as ctx:
        _set(ctx, monkeypatch)
        T = parity.tables_from_context(ctx)
        want_w2 = np.zeros(T.image_size(), dtype=np.uint64)
        want_img, _ = T.track(0, 777, 0, nbatch, hpt, ol.MATH_LIBM, n_threads=16, w2=want_w2)
        img, w2, _, done = ctx.run_projection_with_variance(0, n, mode="fast", seed=31)
    assert done == n
    r_oracle, r_fast = _class_ratio(want_img, want_w2), _class_ratio(img, w2)
    d = np.abs(r_fast - r_oracle) / r_oracle
    print("FAST against the libm oracle, |dR_k| / R_k:", np.round(d, 5), "tolerance", np.round(R_TOLERANCE, 5))
    assert np.all(d <= np.array(R_TOLERANCE)), (d, R_TOLERANCE)
    for factor in (4.0, 0.25):  # shift 9, shift 11
        assert np.all(np.abs(factor * r_fast - r_oracle) / r_oracle > np.array(R_TOLERANCE)), factor
