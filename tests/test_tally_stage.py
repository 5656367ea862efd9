"""The plan of the staged detector tally (csrc/tally_stage.hpp) through the C ABI: pure host arithmetic, no GPU.

The FAST kernels store a detected photon as a record in the block of (workgroup, bin) and a second kernel folds the blocks into
the image.  The mapping tally word -> (bin, bin-relative word) must be a bijection onto the real words, whatever the detector's
shape; the buffer's size must be what the plan says; and the sub-launches of a large launch must tile its range of histories."""
import numpy as np
import pytest

import cases

BENCH_WORDS = 1848 * 768 * 4
SMALL_DETS = sorted({tuple(kw["n_detector_pixels"]) for _, kw in cases.CASES.values()})


def _check_bijection(eng, words, bins=0):
    plan = eng.tally_stage_plan(words, 1_000_000, 512, bins=bins)
    n_bins, wpb = plan["bins"], plan["words_per_bin"]
    assert n_bins > 0 and (bins == 0 or n_bins == bins)
    assert wpb == 4 * plan["bin_pixels"] and plan["bin_pixels"] % 64 == 0
    b, r = eng.tally_stage_map(words, bins=bins)
    assert b.size == words and int(b.max()) < n_bins and int(r.max()) < wpb
    key = b.astype(np.uint64) * np.uint64(wpb) + r.astype(np.uint64)
    assert np.unique(key).size == words  # injective; the images lie in [0, n_bins) x [0, words_per_bin) by the line above
    # the mapping is the one the issue states: runs of 64 pixels dealt round-robin, the four planes of a pixel in one bin
    pixels = words // 4
    w = np.arange(words, dtype=np.uint64)
    plane, pixel = w // np.uint64(pixels), w % np.uint64(pixels)
    run = pixel // np.uint64(64)
    assert np.array_equal(b, (run % np.uint64(n_bins)).astype(np.uint32))
    off = (run // np.uint64(n_bins)) * np.uint64(64) + pixel % np.uint64(64)
    assert np.array_equal(r, (plane * np.uint64(plan["bin_pixels"]) + off).astype(np.uint32))
    return plan


def test_bench_detector_mapping_is_a_bijection(engine):
    plan = _check_bijection(engine, BENCH_WORDS)
    assert plan["words_per_bin"] * 8 <= 128 * 1024  # a bin's words as 64-bit counters fit the fold's LDS
    assert (plan["bins"] + 1) * 4 <= 2048           # and the cursor table fits what the Catphan LDS image leaves free


@pytest.mark.parametrize("nx,nz", [(100, 7), (1000, 1), (333, 3), (65, 3), (64, 1), (1, 1), (63, 2)] + SMALL_DETS)
def test_odd_detector_shapes(engine, nx, nz):
    _check_bijection(engine, nx * nz * 4)


@pytest.mark.parametrize("nx,nz,bins", [(100, 1, 5), (64, 1, 3), (231, 96, 1000), (200, 3, 7)])
def test_forced_bin_counts_including_fewer_runs_than_bins(engine, nx, nz, bins):
    runs = (nx * nz + 63) // 64
    if (nx, nz) != (200, 3) and (nx, nz) != (231, 96):
        assert runs < bins
    _check_bijection(engine, nx * nz * 4, bins=bins)


@pytest.mark.parametrize("words,hist,wg", [(BENCH_WORDS, 100_000_000, 512), (BENCH_WORDS, 1, 1), (231 * 96 * 4, 60_000, 59), (4, 10, 3),
                                           (BENCH_WORDS, 1 << 27, 537)])
def test_reported_bytes_are_capacity_times_streams(engine, words, hist, wg):
    plan = engine.tally_stage_plan(words, hist, wg)
    assert plan["bytes"] == plan["capacity"] * wg * plan["bins"] * 8
    assert plan["capacity"] % 2 == 0                                     # blocks start on 16 bytes
    assert plan["capacity"] * wg * plan["bins"] >= 1.25 * hist           # a history scores at most one hit


def test_plan_needs_no_device(engine, case_dir):
    with engine.create(case_dir("water"), device=-1) as ctx:
        nz, nx = ctx.detector_shape
        a = engine.tally_stage_plan(ctx.image_words, 60_000, 512, ctx=ctx)
    assert a == engine.tally_stage_plan(nx * nz * 4, 60_000, 512)


def test_a_context_without_a_device_stages_nothing_and_refuses_to_launch(engine, case_dir):
    """The staged tally's host state of a context created with device = -1 is the empty one: every key that reads it answers 0
    without touching a device, no grid size has been asked, and a launch is refused before anything else is looked at."""
    with engine.create(case_dir("catphan64"), device=-1) as ctx:
        for key in ("tally_stage_bins", "tally_stage_capacity", "tally_stage_bytes", "tally_stage_fallback_hits", "tally_stage_staged_hits",
                    "blocks_per_cu"):
            assert ctx.geti(key) == 0, key
        with pytest.raises(engine.EngineError) as e:
            ctx.launch(0, 0, 1000, mode="fast", seed=3)
        assert e.value.code == -1 and "has no device" in e.value.message


@pytest.mark.parametrize("limit", [1, 7, 1000, 1 << 27])
def test_sub_launches_tile_the_launch(engine, limit):
    first = 2 ** 32 - 5
    for count in (0, 1, limit - 1, limit, limit + 1, 10 * limit + 7):
        n = engine.tally_stage_plan(BENCH_WORDS, count, 512, limit=limit)["sub_launches"]
        assert n == max(1, -(-count // limit))
        at, total = first, 0
        for k in range(n):
            f, c = engine.tally_stage_sub_launch(first, count, limit, k)
            assert f == at and c <= limit and (c > 0 or count == 0)
            at += c
            total += c
        assert total == count
        assert engine.tally_stage_sub_launch(first, count, limit, n) == (first + count, 0)
