"""CPU: the pruned batch's chunk on the packed 6-bit shadow (csrc/prune.hip, k_q6_query_mq / k_q6_bounds_mq), on numpy
twins only.

The query operand of the chunk: with (u, g, j) = q6_slot(i), the code of element i, plane p (0 hi, 1 lo) of query b is
byte (((u 2 + p) 64 + 16 g + b) 16 + j).  The matrix core pairs the 16 bytes of lane l of the row operand (row l & 15 of
the tile, lane group l >> 4: _prune6_helpers.operand_words) with the 16 bytes of lane l of the query operand (column
l & 15, the same lane group); summed over the k-steps and the four lane groups that is one row's sum with one query's
plane.  The tests pair the two operands exactly so, byte for byte, and compare with the integer dot of the codes."""
import numpy as np
import pytest

from _prune6_helpers import (integer_sums, lower_bound6, operand_words, pack, quantise_query, shadow6, slot, upper_bound)
from _prune_batch_helpers import MQ_WIDTH, edge_queries
from _prune_helpers import adversarial_rows, queries

DIMS = (256, 512, 1024)


def query_operand(twins, dim):
    """numpy twin of k_q6_query_mq's buffer for a chunk of len(twins) <= 16 queries: int8 [dim / 64, 2, 64, 16] =
    [k-step u, plane p, lane 16 g + b, byte j]; slots past the chunk hold zero codes"""
    out = np.zeros((dim // 64) * 2 * 64 * 16, dtype=np.int8)
    u, g, j = slot(np.arange(dim))
    for b, t in enumerate(twins):
        for p, plane in enumerate((t["d_hi"], t["d_lo"])):
            out[(((u * 2 + p) * 64 + 16 * g + b) * 16 + j)] = plane
    return out.reshape(dim // 64, 2, 64, 16)


def chunk_sums(packed, n, dim, opnd):
    """what the two MFMAs a k-step accumulate: (hi, lo) int64 [16, n], the sums of row r's operand bytes (4 c) with the
    bytes of column b's plane, over every k-step and lane group"""
    hi, lo = np.zeros((MQ_WIDTH, n), np.int64), np.zeros((MQ_WIDTH, n), np.int64)
    q = opnd.astype(np.int64)
    for r in range(n):
        for g in range(4):
            lanes = 16 * g + np.arange(MQ_WIDTH)  # the lanes of this lane group: one column each
            for u in range(dim // 64):
                a = operand_words(packed[r >> 4], 16 * g + (r & 15), u)
                hi[:, r] += q[u, 0, lanes] @ a
                lo[:, r] += q[u, 1, lanes] @ a
    return hi, lo


def plane_sums(c, t):
    """the same two sums from the codes in natural order: 4 c . d_hi and 4 c . d_lo"""
    zero = np.zeros_like(t["d_hi"])
    return integer_sums(c, dict(d_hi=t["d_hi"], d_lo=zero)) // 256, integer_sums(c, dict(d_hi=zero, d_lo=t["d_lo"]))


def int_rows(n, dim, seed):
    """integer rows in [-31, 31] with a 31 in every row: codes = rows"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-31, 32, (n, dim))
    X[np.arange(n), np.arange(n) % dim] = 31
    return X


def sixteen_queries(dim, seed=5):
    """16 queries that all differ, in direction and by orders of magnitude in norm; one on the rint ties"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((MQ_WIDTH, dim)) * np.exp2(rng.integers(-12, 13, MQ_WIDTH))[:, None]
    Q[3] = edge_queries(rng, dim)[3]
    return np.ascontiguousarray(Q, dtype=np.float32)


@pytest.mark.parametrize("dim", DIMS)
def test_operand_pairing_gives_every_querys_sums_in_its_column(dim):
    n = 19  # two tiles, the second ragged
    X = int_rows(n, dim, seed=dim)
    packed = pack(X)
    twins = [quantise_query(q) for q in sixteen_queries(dim)]
    assert not any(t["bad"] for t in twins)
    hi, lo = chunk_sums(packed, n, dim, query_operand(twins, dim))
    for b, t in enumerate(twins):
        want_hi, want_lo = plane_sums(X, t)
        assert np.array_equal(hi[b], want_hi) and np.array_equal(lo[b], want_lo), (dim, b)
        assert np.array_equal(256 * hi[b] + lo[b], integer_sums(X, t)), (dim, b)
    # a narrower chunk: another query in slot 0, zero codes and zero sums in the slots past it
    hi, lo = chunk_sums(packed, n, dim, query_operand(twins[13:], dim))
    for b, t in enumerate(twins[13:]):
        assert np.array_equal(256 * hi[b] + lo[b], integer_sums(X, t)), (dim, b)
    assert not hi[3:].any() and not lo[3:].any()


@pytest.mark.parametrize("dim", DIMS)
def test_a_wrong_query_placement_changes_some_sum(dim):
    """the argument tests/test_prune6_cpu.py makes for the rows, for the query operand: each mutation of the placement
    changes some sum of these rows and queries, so a kernel that wrote or read the operand that way would fail the
    GPU lane-map test"""
    n = 16
    X = int_rows(n, dim, seed=7)
    packed = pack(X)
    twins = [quantise_query(q) for q in sixteen_queries(dim)]
    opnd = query_operand(twins, dim)
    want = chunk_sums(packed, n, dim, opnd)
    cols = opnd.reshape(dim // 64, 2, 4, 16, 16)  # [k-step, plane, lane group, column, byte]
    perm = np.arange(16)
    perm[[2, 9]] = [9, 2]
    mutations = {"two columns swapped": cols[:, :, :, perm, :], "hi and lo swapped": cols[:, ::-1],
                 "lane groups 1 and 2 swapped": cols[:, :, [0, 2, 1, 3]]}
    for name, mut in mutations.items():
        got = chunk_sums(packed, n, dim, np.ascontiguousarray(mut).reshape(opnd.shape))
        assert np.any(got[0] != want[0]) or np.any(got[1] != want[1]), name


@pytest.mark.parametrize("dim", DIMS)
def test_bound_holds_per_slot_on_adversarial_rows(oracle, dim):
    """lb < S < ub in float64 for every slot of a chunk, with the sums taken through the chunk's operand pairing"""
    rng = np.random.default_rng(0)
    X = adversarial_rows(rng, dim)
    n = X.shape[0]
    c, s, a = shadow6(X)
    fin = np.isfinite(a)
    assert fin.sum() >= 30 and (~fin).sum() >= 13
    Xf = np.where(np.isfinite(X), X, 0).astype(np.float32)
    Q = (edge_queries(rng, dim) + queries(rng, X) + [sixteen_queries(dim)[0], sixteen_queries(dim)[1]])[:MQ_WIDTH]
    assert len(Q) == MQ_WIDTH
    twins = [quantise_query(q) for q in Q]
    hi, lo = chunk_sums(pack(c), n, dim, query_operand(twins, dim))
    checked = 0
    for b, (q, t) in enumerate(zip(Q, twins)):
        if t["bad"]:  # the zero query: zero codes, and the slot takes the full scan
            assert not hi[b].any() and not lo[b].any()
            continue
        lb, w, I = lower_bound6(c, s, a, t)
        assert np.array_equal(256 * hi[b] + lo[b], I), (dim, b)
        assert np.abs(I).max() < 2 ** 33 and np.abs(hi[b]).max() < 2 ** 31 and np.abs(lo[b]).max() < 2 ** 31
        S = oracle.scores_kernel_order(Xf, q).astype(np.float64)
        ub = upper_bound(lb, w)
        l = lb.astype(np.float64)
        assert np.all(np.isfinite(l[fin])) and np.all(l[fin] < S[fin]) and np.all(S[fin] < ub[fin]), (dim, b)
        assert np.all(lb[~fin] == -np.inf) and not np.any(ub[~fin] < np.inf)  # always rescored
        checked += 1
    assert checked >= 14
