"""How a FAST launch deals its history ids (csrc/id_tickets.hpp), through the C ABI queries that call the kernels' own functions: the
ticket schedule of the 64 dispensers tiles the launch exactly once, and the walk over the dispensers follows the exhaustion mask.
Pure host arithmetic: no GPU."""
import numpy as np
import pytest

N_COUNTERS, CHUNK = 64, 256
COUNTS = [0, 1, 63, 64, 255, 256, 257, 1025, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, 60_000, 100_000_007]


def _random_counts():
    """200 seeded counts below 2^33, log-uniform: 190 below 2^24 and 10 between 2^24 and 2^33 (a count of 2^33 has 3.4e7 tickets, every
    one of which is checked)."""
    rng = np.random.default_rng(20240611)
    small = np.exp2(rng.uniform(0, 24, 190)).astype(np.uint64)
    large = np.exp2(rng.uniform(24, 33, 10)).astype(np.uint64)
    return [int(c) for c in small] + [int(min(c, 2 ** 33 - 1)) for c in large]


def _check_count(engine, count):
    at = 0
    for ctr in range(N_COUNTERS):
        lo, hi, n = engine.id_tickets(count, ctr)  # every non-empty ticket and the one after
        assert len(lo) == n + 1
        q, r = divmod(count, N_COUNTERS)
        assert n == 0 or int(lo[0]) == q * ctr + min(ctr, r) == at, (count, ctr)
        size = hi[:n] - lo[:n]
        assert np.all(hi[:n] > lo[:n]) and np.all(size <= CHUNK), (count, ctr)  # ascending, none empty, none above kChunk
        assert np.array_equal(lo[1:n], hi[: max(n - 1, 0)]), (count, ctr)       # contiguous
        if n:
            at = int(hi[n - 1])
        assert at == q * (ctr + 1) + min(ctr + 1, r), (count, ctr)              # ... up to the end of the dispenser's part
        assert lo[n] == hi[n], (count, ctr)
        # past the last: the next few, and ticket numbers as large as a counter can get
        for first in (n, n + 8192 * 64, 2 ** 63, 2 ** 64 - 5):
            l2, h2, n2 = engine.id_tickets(count, ctr, first, 4)
            assert n2 == n and np.array_equal(l2, h2), (count, ctr, first)
    assert at == count


@pytest.mark.parametrize("count", COUNTS)
def test_tickets_tile_the_launch(engine, count):
    _check_count(engine, count)


def test_tickets_tile_random_launches(engine):
    for count in _random_counts():
        _check_count(engine, count)


def test_tickets_are_whole_chunks_up_to_the_last(engine):
    lo, hi, n = engine.id_tickets(100_000_000, 5)
    size = (hi - lo)[:n].astype(np.int64)
    assert n == -(-1_562_500 // CHUNK) and np.all(size[:-1] == CHUNK) and size[-1] == 1_562_500 % CHUNK


def _next_counter(mask, ctr):
    for k in range(1, N_COUNTERS + 1):
        if not (mask >> ((ctr + k) % N_COUNTERS)) & 1:
            return (ctr + k) % N_COUNTERS
    return N_COUNTERS


def test_next_counter_follows_the_mask(engine):
    rng = np.random.default_rng(7)
    full = 2 ** 64 - 1
    masks = [0, full] + [1 << b for b in range(64)] + [full ^ (1 << b) for b in range(64)]
    masks += [int(m) for m in rng.integers(0, 2 ** 64, 300, dtype=np.uint64)]
    masks += [int(a & b & c) for a, b, c in rng.integers(0, 2 ** 64, (100, 3), dtype=np.uint64)]  # sparse
    masks += [int(a | b | c) for a, b, c in rng.integers(0, 2 ** 64, (100, 3), dtype=np.uint64)]  # dense
    for mask in masks:
        for ctr in range(N_COUNTERS):
            assert engine.id_next_counter(mask, ctr) == _next_counter(mask, ctr), (hex(mask), ctr)
    for ctr in range(N_COUNTERS):
        assert engine.id_next_counter(0, ctr) == (ctr + 1) % N_COUNTERS and engine.id_next_counter(full, ctr) == N_COUNTERS
        assert engine.id_next_counter(full ^ (1 << ctr), ctr) == ctr  # the counter itself comes last
    for bad in (-1, 64):
        with pytest.raises(ValueError):
            engine.id_next_counter(0, bad)
