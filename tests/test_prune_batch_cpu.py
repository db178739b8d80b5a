"""CPU: the certificate of the pruned batch (csrc/prune.hip, k_q8_query_mq / k_q8_bounds_mq; DESIGN.md section 4,
"Pruned batch") re-derived in numpy.  A query is quantised to two int8 planes, q ~ t2 (256 d_hi + d_lo); with the exact
integer sums I_hi, I_lo of a row's codes with them the claim is

    lb < S < ub      S = the f32 scan's score (oracle.scores_kernel_order, the bits of scan.hip),
                     lb = s t2 (256 I_hi + I_lo) - w - pads,  ub = lb + 2 w + pads,  w = a Q + s 127 sqrt(dim) e

for every row that can be bounded and every query that can, on the adversarial rows of test_prune_cpu.py and on queries
that strain the quantisation (_prune_batch_helpers.edge_queries).  Queries that cannot be bounded are flagged.  The
entry point is declared, exported and bound."""
import numpy as np
import pytest

from _prune_batch_helpers import (edge_queries, flagged_queries, lower_bound, quantise_query, upper_bound)
from _prune_helpers import adversarial_rows, queries, shadow

DIMS = (256, 512, 1024)


@pytest.mark.parametrize("dim", DIMS)
def test_interval_holds_for_every_row_and_query(oracle, dim):
    rng = np.random.default_rng(0)
    X = adversarial_rows(rng, dim)
    c, s, a = shadow(X)
    fin = np.isfinite(a)
    assert fin.sum() == X.shape[0] - 13
    Xf = np.where(np.isfinite(X), X, 0).astype(np.float32)
    # (the zero query and the one of norm 1e-30 among them cannot be bounded: test_unboundable_queries_are_flagged)
    qs = [q for q in queries(rng, X) if np.abs(q).max() >= 2.0 ** -60] + edge_queries(rng, dim)
    assert len(qs) == 12
    clamped = ties = 0
    for qi, q in enumerate(qs):
        qq = quantise_query(q)
        assert not qq["bad"], qi
        clamped += int(np.sum(np.abs(qq["d_lo"]) == 127))
        ties += int(np.sum(np.abs(q.astype(np.float64) / np.float64(qq["t"]) % 1.0) == 0.5))
        # the residual the error term pays for, the clamp of d_lo included
        res = q.astype(np.float64) - np.float64(qq["t2"]) * (256.0 * qq["d_hi"] + qq["d_lo"])
        assert np.sqrt(np.sum(res * res)) <= float(qq["e"]), qi
        S = oracle.scores_kernel_order(Xf, q).astype(np.float64)
        lb, w, _, _ = lower_bound(c, s, a, qq)
        ub = upper_bound(lb, w)
        lbd = lb.astype(np.float64)
        assert np.all(np.isfinite(lbd[fin])) and np.all(np.isfinite(ub[fin])), qi
        assert np.all(lbd[fin] < S[fin]), (qi, np.nonzero(fin & ~(lbd < S))[0][:8])
        assert np.all(S[fin] < ub[fin]), (qi, np.nonzero(fin & ~(S < ub))[0][:8])
        assert np.all(lb[~fin] == -np.inf) and np.all(np.isnan(ub[~fin]))  # they survive every threshold
    assert clamped > dim and ties > dim // 2  # the tie and clamp queries are what they claim to be


@pytest.mark.parametrize("dim", DIMS)
def test_two_planes_keep_the_bound_narrow(oracle, dim):
    """on unit-norm rows the query's error term adds a few percent to the width a Q, not a multiple"""
    X = oracle.synth_rows(5, 0, 500, dim)
    _, s, a = shadow(X)
    q = oracle.synth_query(3, dim)
    qq = quantise_query(q)
    assert float(qq["e"]) < 1e-4 * float(qq["Q"])
    from _prune_batch_helpers import width
    ratio = width(s, a, qq, dim) / (a.astype(np.float64) * float(qq["Q"]))
    assert 1.0 <= ratio.min() and ratio.max() < 1.05, (ratio.min(), ratio.max())


@pytest.mark.parametrize("dim", DIMS)
def test_unboundable_queries_are_flagged(dim):
    for q in flagged_queries(dim):
        qq = quantise_query(q)
        assert qq["bad"] and not qq["d_hi"].any() and not qq["d_lo"].any()
    assert not quantise_query(np.full(dim, 2.0 ** -59, np.float32))["bad"]


def test_entry_point_is_declared_exported_and_bound():
    from seesaw_amd import _lib
    name = "ssw_index_topk_batch_pruned"
    assert name in _lib.declared_symbols()
    assert name in _lib._SIGNATURES and _lib._SIGNATURES[name] == _lib._SIGNATURES["ssw_index_topk_batch"]
    assert hasattr(_lib.load(), name)
    hooks = set(_lib.declared_symbols(_lib.DEBUG_HEADER_PATH))
    for hook in ("ssw_tune_prune_scan_mq", "ssw_debug_prune_scan_mq_shape", "ssw_debug_prune_bounds_mq",
                 "ssw_debug_prune_survivors_mq"):
        assert hook in hooks and hook in _lib._DEBUG_SIGNATURES
    import inspect
    from seesaw_amd.device_index import DeviceIndex
    assert inspect.signature(DeviceIndex.topk_batch).parameters["prune"].default is False
