"""The end of a FAST launch (csrc/id_tickets.hpp; track_pool.inc: deal_history_ids): ids dealt as tickets, dispensers skipped
through the exhaustion mask, and the staged tally's `counts` no longer cleared between launches.

History ids are explicit (first + id) and a history's stream depends on its id alone, so the uint64 image of a launch of N is the sum
of the images of two launches that split its range anywhere: an id dealt twice, or not at all, changes a tally word.  The counts
straddle what the dealing distinguishes: fewer ids than dispensers (1, 63), dispensers of 16 and 17 ids (1025), the launch of
64 * 256 ids that is one whole ticket per dispenser and its neighbours, and one with a ragged last ticket on every dispenser
(100 003).  In all of them most waves of the grid find every dispenser exhausted at once: the walk along the mask is what they run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MCGPU_TALLY_STAGE", "MCGPU_TALLY_STAGE_CAP", "MCGPU_TALLY_STAGE_MAX_HISTORIES")
COUNTS = (1, 63, 1025, 16_383, 16_384, 16_385, 100_003)
FIRST = 2 ** 32 - 1000


def _stage(ctx, monkeypatch, on):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCGPU_TALLY_STAGE", "1" if on else "0")
    ctx.reload_env_knobs()
    assert (ctx.geti("tally_stage_bins") > 0) == on


@pytest.mark.parametrize("sched", [0, 1])
def test_split_launches_sum_to_the_whole_staged_and_direct(engine, case_dir, monkeypatch, sched):
    monkeypatch.setenv("MCGPU_FAST_SCHED", str(sched))
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        assert ctx.geti("fast_scheduler") == sched

        def image(first, n):
            img, _, done = ctx.run_projection(0, n, mode="fast", seed=9, first=first)
            assert done == n
            return img

        whole = {}
        for staged in (False, True):
            _stage(ctx, monkeypatch, staged)
            for n in COUNTS:
                whole[staged, n] = image(FIRST, n)
                for k in sorted({1, n // 2, n - 1} - {0, n}):
                    parts = image(FIRST, k) + image(FIRST + k, n - k)
                    assert np.array_equal(parts, whole[staged, n]), (staged, n, k)
        for n in COUNTS:
            assert np.array_equal(whole[True, n], whole[False, n]), n
        assert int(whole[False, 100_003].sum()) > int(whole[False, 16_384].sum()) > int(whole[False, 1025].sum()) > 0


def test_a_smaller_staged_launch_after_a_larger_one(engine, case_dir, monkeypatch):
    """60 000 histories fill the grid's workgroups and leave their record counts behind; the 1025 that follow launch two workgroups
    into a fresh image.  Nothing clears the counts in between: the fold must read the two launched workgroups' entries only."""
    with engine.create(case_dir("catphan64"), device=0) as ctx:
        _stage(ctx, monkeypatch, False)
        ref, _, _ = ctx.run_projection(0, 1025, mode="fast", seed=9, first=FIRST)
        _stage(ctx, monkeypatch, True)
        big, _, done = ctx.run_projection(0, 60_000, mode="fast", seed=9, first=FIRST)
        assert done == 60_000 and ctx.geti("tally_stage_staged_hits") > 1025
        small, _, done = ctx.run_projection(0, 1025, mode="fast", seed=9, first=FIRST)
        assert done == 1025 and np.array_equal(small, ref) and 0 < int(ref.sum()) < int(big.sum())
