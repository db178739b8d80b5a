"""CPU: the int8 shadow's error bound (tests/test_prune_cpu.py) on the rows an f16 index holds.  The shadow of an f16
index is the shadow of its widened rows W = round_vectors(X, np.float16), and S is the f32 scan's score of W
(oracle.scores_kernel_order): the f16 scan returns those bits.  This is the numpy statement
tests/test_prune_f16_gpu.py compares the device against, on the binary16-specific rows of tests/_prune_f16_helpers.py:
the largest binary16, overflow to +inf, binary16 subnormals, values that round to zero, -0.0, exact rint ties."""
import numpy as np
import pytest

from _prune_f16_helpers import N_ROWS, N_UNBOUNDED, f16_adversarial_rows, unbounded_rows
from _prune_helpers import PAD_ABS, queries, shadow

DIMS = (256, 512, 1024)


@pytest.mark.parametrize("dim", DIMS)
def test_bound_holds_on_widened_binary16_rows(oracle, dim):
    from seesaw_amd.device_index import round_vectors
    rng = np.random.default_rng(0)
    X = f16_adversarial_rows(rng, dim)
    with np.errstate(over="ignore"):
        W = round_vectors(X, np.float16)
    assert W.dtype == np.float32 and W.shape == (N_ROWS, dim)
    c, s, a = shadow(W)
    unb = unbounded_rows(W)
    expect = np.zeros(N_ROWS, dtype=bool)
    expect[26:29] = expect[33:49] = expect[50] = True
    assert np.array_equal(unb, expect) and int(unb.sum()) == N_UNBOUNDED
    assert np.array_equal(np.isinf(a), unb) and not np.isnan(a).any()
    assert np.all(s[unb] == 0) and not c[unb].any()
    # what binary16 did to the rows: the largest value kept, 70000 gone to +inf, subnormals kept, 1e-9 gone to zero
    assert np.max(np.abs(W[49])) == 65504 and W[50, 11] == np.inf
    assert not W[24:26].any() and not W[53].any() and a[24] == 0 and a[53] == 0
    assert np.array_equal(W[52], X[52]) and 0 < np.max(np.abs(W[52])) < 2.0 ** -14 and np.isfinite(a[52]) and s[52] > 0
    assert np.array_equal(W[51, ::3], X[51, ::3]) and np.array_equal(W[55], X[55])
    assert 0 < np.max(np.abs(W[51, ::3])) <= 2.0 ** -15 < 2.0 ** -14 <= np.max(np.abs(W[51]))
    assert s[55] == np.float32(2.0 ** -7)
    assert np.all(np.signbit(W[54, ::2])) and not W[54, ::2].any()
    # the ties are ties: x / s lies exactly halfway between two codes, and rint takes the even one
    t = W[55, 1:].astype(np.float64) * 128
    assert np.all(t - np.floor(t) == 0.5) and np.all(c[55, 1:] % 2 == 0)
    Wf = np.where(np.isfinite(W), W, 0).astype(np.float32)
    fin = np.isfinite(a)
    for q in queries(rng, W):
        S = oracle.scores_kernel_order(Wf, q).astype(np.float64)
        Q = np.sqrt(np.sum(q.astype(np.float64) ** 2)) * (1 + 2.0 ** -40)
        prods = c.astype(np.float32) * q[None, :]
        for A in (prods.sum(1, dtype=np.float32),                       # pairwise
                  np.cumsum(prods, axis=1, dtype=np.float32)[:, -1]):  # sequential
            approx = s.astype(np.float64) * A.astype(np.float64)
            err = np.abs(S[fin] - approx[fin])
            lim = a[fin].astype(np.float64) * Q + PAD_ABS
            assert np.all(err <= lim), float((err / lim).max())
