"""GPU: the pruned batch on the packed 5-bit shadow (csrc/prune.hip: k_q5_bounds_mq, k_candidate_rows_slot,
k_exact_threshold_mq; csrc/rescore_dev.hip: k_score_candidates; csrc/index_prune.hip: prune_batch_shadow), on the lab
build with ssw_tune_prune5(1, 0) / ssw_tune_prune5_batch(0), so that small indexes qualify.

The integer sums of every slot against numpy's int64 dot and lb <= s <= ub for every (query, row) with s in float64; the
batch's results against the plain batch and against a float64 lexsort of the scan's scores, through ties at the
threshold, per-query exclusions and a query that cannot be bounded; and the shadow the batch ran on.  The host-waiting
batch has no lab switch for SURV_CAP (ssw_tune_surv_cap is the device batch's), so no case passes the cap here."""
import ctypes

import numpy as np
import pytest

from _prune5_helpers import hook_shadow5, integer_sums, mode5, quantise_query, upper_bound, width5
from _prune6_helpers import mode6
from _prune_helpers import mode, same, stats

pytestmark = pytest.mark.gpu


def bytes5(n, dim):
    return (n + 15) // 16 * 16 * (dim * 5 // 8 + 8)


@pytest.fixture()
def five(lab_build):
    """single queries and pruned batches of every eligible index take the 5-bit shadow; the three-launch top-k of small
    indexes (it never prunes) is off; the defaults again afterwards"""
    from seesaw_amd import _lib
    mode(lab_build, True)
    mode6(True, -1)
    mode5(True, 0)
    _lib.call("ssw_tune_prune5_batch", 0)
    _lib.call("ssw_tune_topk", 2)
    try:
        yield lab_build
    finally:
        _lib.call("ssw_tune_topk", 3)
        _lib.call("ssw_tune_prune5_batch", -1)
        mode5(True, -1)
        mode(lab_build, True)


def unit_rows(n, dim, seed):
    X = np.random.default_rng(seed).standard_normal((n, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(X)


def the_queries(nq, dim, seed):
    """directions all different, norms over orders of magnitude"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, dim)) * np.exp2(rng.integers(-12, 13, nq))[:, None]
    return np.ascontiguousarray(Q, dtype=np.float32)


def hook_bounds5_mq(idx, Q):
    """k_q6_query_mq + k_q5_bounds_mq: (I int64 [nq, n], lb f32 [nq, n], Qe f32 [nq, 4] = Q, e, t2, flag)"""
    from seesaw_amd import _lib
    nq, n = Q.shape[0], idx.n_rows
    I, lb, qe = np.empty((nq, n), np.int64), np.empty((nq, n), np.float32), np.empty((nq, 4), np.float32)
    _lib.call("ssw_debug_prune5_bounds_mq", idx._h, ctypes.c_void_p(Q.ctypes.data), nq, ctypes.c_void_p(I.ctypes.data),
              ctypes.c_void_p(lb.ctypes.data), ctypes.c_void_p(qe.ctypes.data), None)
    return I, lb, qe


@pytest.mark.parametrize("nq", (1, 15, 16))
@pytest.mark.parametrize("n", (16 * 257 + 5, 16 * 64))
@pytest.mark.parametrize("dim", (512, 1024))
def test_sums_and_certificate_of_every_slot(five, dim, n, nq):
    from seesaw_amd.device_index import DeviceIndex
    X = unit_rows(n, dim, seed=dim + n)
    Q = the_queries(nq, dim, seed=nq)
    idx = DeviceIndex.from_numpy(X)
    try:
        I, lb, qe = hook_bounds5_mq(idx, Q)
        c, s5, a5 = hook_shadow5(idx)
        for j in range(nq):
            assert qe[j, 3] == 0
            want = integer_sums(c, quantise_query(Q[j]))
            assert np.array_equal(I[j], want), (j, np.argwhere(I[j] != want)[:4])
            s = X.astype(np.float64) @ Q[j].astype(np.float64)
            ub = upper_bound(lb[j], width5(s5, a5, dict(Q=qe[j, 0], e=qe[j, 1]), dim))
            ok = (lb[j].astype(np.float64) <= s) & (s <= ub)
            assert ok.all(), (j, np.nonzero(~ok)[0][:8])
    finally:
        idx.close()


# ---- end to end -----------------------------------------------------------------------------------------------------
N, DIM = 20_011, 512


@pytest.fixture(scope="module")
def row_sets(oracle):
    """rows with 51 copies of one row (ties at the threshold of the query that points at it), 17 queries, and their
    scores in the scan's order, computed once"""
    orc = oracle
    X = unit_rows(N, DIM, seed=9)
    X[5000:5051] = X[77]
    Q = the_queries(17, DIM, seed=4)
    Q[2] = X[77] * np.float32(3.0) + Q[2] * np.float32(2.0 ** -20)  # the copies lead query 2, tied
    S = np.stack([orc.scores_kernel_order(X, q) for q in Q])
    return X, Q, S


def lexsort_topk(S, k, excluded):
    """(rows, scores): the larger score first in float64, the smaller row first among equals"""
    alive = np.setdiff1d(np.arange(S.shape[0]), np.asarray([] if excluded is None else excluded, dtype=np.int64))
    order = alive[np.lexsort((alive, -S[alive].astype(np.float64)))[:k]]
    return order, S[order]


@pytest.mark.parametrize("k", (1, 100))
@pytest.mark.parametrize("nq", (1, 2, 16, 17))
@pytest.mark.parametrize("rows", ("duplicates", "unboundable"))
def test_results_and_the_shadow_that_was_used(five, oracle, row_sets, rows, nq, k):
    """prune=True == the plain batch == the float64 lexsort; after single queries built the 5-bit shadow the batch's
    chunks run on it (every query counted, no other shadow allocated) and exactly the forced slots fall back"""
    from seesaw_amd.device_index import DeviceIndex
    X, Q, S = row_sets
    Q, S = Q[:nq].copy(), S[:nq].copy()
    forced = []
    if rows == "unboundable":  # one query of the batch scaled by 2^66: its norm is out of the certificate's range
        forced = [nq - 1]
        Q[nq - 1] = Q[nq - 1] / np.linalg.norm(Q[nq - 1]) * np.float32(2.0 ** 66)
        S[nq - 1] = oracle.scores_kernel_order(X, Q[nq - 1])
    ex = [None if b % 3 == 0 else np.arange(b, N, 7 + b) for b in range(nq)]  # a list of its own for every query
    ex[min(2, nq - 1)] = np.arange(5000, 5020)  # some of the tied copies
    idx, ref = DeviceIndex.from_numpy(X), DeviceIndex.from_numpy(X)
    try:
        idx.topk(Q[0], k)  # a single query builds the 5-bit shadow
        before = stats(idx)
        assert before[0] == 1 and before[5] == bytes5(N, DIM), before
        got = idx.topk_batch(Q, k, excluded=ex, prune=True)
        st = stats(idx)
        want = ref.topk_batch(Q, k, excluded=ex)
        for b in range(nq):
            same(want[b], got[b])
            r, s = lexsort_topk(S[b], k, ex[b])
            assert np.array_equal(got[b][2], r) and np.array_equal(got[b][1].view(np.uint32), s.view(np.uint32)), b
        assert st[3] - before[3] == nq, (before, st)              # every query of the batch went through a pruned chunk
        assert st[0] == 1 and st[5] == bytes5(N, DIM), st         # ... on the 5-bit shadow: no 6-bit, no int8 one
        assert st[4] - before[4] == len(forced), (before, st)     # ... and only the forced slots took the full scan
    finally:
        idx.close()
        ref.close()
