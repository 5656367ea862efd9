"""tests/fixed_sum_ref.py, the numpy statement of csrc/fixed_sum.inc's order of additions: its vectorised form against the plain
thread-by-thread one, and that the order it states can be told from numpy's own at the sizes the GPU tests use."""
import numpy as np
import pytest

from fixed_sum_ref import grid_sum, grid_sum_by_thread


def _squares(n, c):
    """Squares of float32 normal deviates, as float64, [n, c] laid out as the GPU tests lay out a residual (the transpose of [c, n]):
    the kind of term the kernels add."""
    return np.random.default_rng(1).normal(size=(c, n)).astype(np.float32).T.astype(np.float64) ** 2


# 1 170 items: less than one block row of the 256 x 256 grid is busy; 67 240 x 3: 1 704 threads add a second item; 64 blocks: more sweeps
@pytest.mark.parametrize("n, c, blocks", [(1170, 1, 256), (67240, 3, 256), (2431, 3, 256), (67240, 3, 64), (5, 2, 3)])
def test_grid_sum_equals_the_thread_by_thread_sum(n, c, blocks):
    terms = _squares(n, c)
    assert grid_sum(terms, blocks) == grid_sum_by_thread(terms, blocks)
    if c == 1:
        assert grid_sum(terms[:, 0], blocks) == grid_sum(terms, blocks)


@pytest.mark.parametrize("n", [67240, 2431])
def test_the_order_can_be_told_from_numpys(n):
    """An == against grid_sum says something only where another order gives another double.  Whether two orders round alike is a
    matter of the draw: with the same deviates laid out [n, c] the two coincide at 2 431 x 3; laid out as here they differ at both sizes."""
    terms = _squares(n, 3)
    ours, pairwise = grid_sum(terms, 256), float(terms.sum())
    print(f"{n} x 3: grid order {ours!r}, numpy {pairwise!r}, relative difference {abs(ours - pairwise) / pairwise:.3g}")
    # both are sums of positive terms: at most 6 + 8 + 256 additions lie on a path of ours, some 150 on one of numpy's
    assert ours != pairwise and ours == pytest.approx(pairwise, rel=420 * 2.0 ** -53)
