"""CPU: the error bound of the int8 shadow (csrc/prune.hip) re-derived in numpy.  For every row the
shadow keeps codes c = rint(x / s) (|c| <= 127, s = max|x| / 127), the scale s and a_r; the claim is

    |S - s * A| <= a_r * ||q||        S = the f32 scan's score (oracle.scores_kernel_order, the bits of scan.hip),
                                      A = any f32 summation of c_i q_i

on adversarial rows: one huge element, all-equal elements, subnormals, zero rows, rows exactly on quantisation-step
boundaries; rows with a non-finite element or an out-of-range scale get a_r = +inf (always rescored)."""
import numpy as np
import pytest

from _prune_helpers import PAD_ABS, adversarial_rows, queries, shadow

DIMS = (256, 512, 1024)


@pytest.mark.parametrize("dim", DIMS)
def test_bound_holds_on_adversarial_rows(oracle, dim):
    rng = np.random.default_rng(0)
    X = adversarial_rows(rng, dim)
    c, s, a = shadow(X)
    bad = ~np.all(np.isfinite(X), axis=1)
    m = np.max(np.abs(np.where(np.isfinite(X), X, 0)), axis=1)
    out_of_range = (m > 0) & ((m < 2.0 ** -60) | (m > 2.0 ** 60))
    assert bad.sum() == 3 and out_of_range.sum() == 10
    assert np.all(np.isinf(a[bad | out_of_range])) and np.all(np.isfinite(a[~(bad | out_of_range)]))
    Xf = np.where(np.isfinite(X), X, 0).astype(np.float32)
    fin = np.isfinite(a)
    for q in queries(rng, X):
        S = oracle.scores_kernel_order(Xf, q).astype(np.float64)
        Q = np.sqrt(np.sum(q.astype(np.float64) ** 2)) * (1 + 2.0 ** -40)
        prods = c.astype(np.float32) * q[None, :]
        for A in (prods.sum(1, dtype=np.float32),                       # pairwise
                  np.cumsum(prods, axis=1, dtype=np.float32)[:, -1]):  # sequential
            approx = s.astype(np.float64) * A.astype(np.float64)
            err = np.abs(S[fin] - approx[fin])
            lim = a[fin].astype(np.float64) * Q + PAD_ABS
            assert np.all(err <= lim), float((err / lim).max())


@pytest.mark.parametrize("dim", DIMS)
def test_bound_is_tight_enough_on_unit_rows(oracle, dim):
    """a unit Gaussian row's a_r is its quantisation error, ~0.0072 at dim 512: the width that lets ~10^3 of 10^8
    synthetic rows survive (the same window holds at dim 256 and 1024)"""
    X = oracle.synth_rows(5, 0, 2000, dim)
    _, _, a = shadow(X)
    assert 0.005 < float(np.median(a)) < 0.0095
