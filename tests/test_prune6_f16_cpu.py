"""CPU: what the 6-bit shadow's numpy twin says about binary16 rows (the GPU test tests/test_prune6_f16_gpu.py compares
k_q6_build_h16 with it): on the widened rounding W of the binary16-specific rows, `shadow6(W)` refuses exactly the rows
`unbounded_rows(W)` names, and the row whose largest element is the largest binary16 gets the step 65504 / 31.  This only
documents the twin; it runs no product code."""
import numpy as np
import pytest

from _prune6_f16_helpers import SMALL_ORDER, f16_rows, small_block, widen
from _prune6_helpers import LEVELS, shadow6
from _prune_f16_helpers import N_ROWS, N_UNBOUNDED, f16_adversarial_rows, unbounded_rows


@pytest.mark.parametrize("dim", (256, 512, 1024))
def test_the_twin_refuses_exactly_the_unbounded_widened_rows(dim):
    W = widen(f16_adversarial_rows(np.random.default_rng(0), dim))
    c, s, a = shadow6(W)
    unb = unbounded_rows(W)
    assert int(unb.sum()) == N_UNBOUNDED and np.array_equal(np.isinf(a), unb)
    assert np.all(s[unb] == 0) and not c[unb].any() and np.abs(c).max() == LEVELS
    assert np.isfinite(a[49]) and s[49] == np.float32(65504) / np.float32(LEVELS)  # max |x| = 65504
    assert np.isinf(a[50])                                                        # 70000 rounds to +inf
    assert np.isfinite(a[52]) and s[52] > 0                                       # all binary16 subnormals: bounded
    assert s[53] == 0 and a[53] == 0                                              # 1e-9 rounds to the zero row


def test_the_rows_of_the_gpu_test_hold_both_kinds_at_every_size():
    dim = 256
    assert len(set(SMALL_ORDER)) == len(SMALL_ORDER) and small_block(dim).shape == (N_ROWS, dim)
    assert unbounded_rows(f16_rows(1, dim)[1]).all() and not unbounded_rows(f16_rows(1, dim, lead=1)[1]).any()
    for n in (2, 15, 16, 17, 31, 63, 200, 1000):
        for lead in (0, 1):
            X, W = f16_rows(n, dim, lead=lead)
            unb = unbounded_rows(W)
            assert X.shape == W.shape == (n, dim) and unb.any() and not unb.all(), (n, lead)
    X, W = f16_rows(1000, dim)
    assert int(unbounded_rows(W).sum()) == 3 * N_UNBOUNDED  # the first rows, a tile boundary, the last rows
    plain = W[100:400]  # Gaussian rows of mixed scale: nothing overflows, no row rounds to the zero row
    assert np.all(np.isfinite(plain)) and np.abs(plain).max() < 65504 and np.all(np.abs(plain).max(axis=1) > 2.0 ** -14)
