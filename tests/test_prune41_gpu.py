"""GPU: the two-stage 4 + 1-bit shadow of single queries on large f32 indexes without an image map (csrc/prune.hip,
"two-stage 4 + 1-bit shadow"), on the lab build, which reaches the path on small indexes through ssw_tune_prune41: the
builder and the first stage's sums against the numpy twin, the coarse certificate row by row against the device's full scan
at every launch shape, the refine's bound against the 5-bit scan's bit for bit (list, dense, repeats), a block's stage
flushed and reused, pruned == full byte for byte through the fallbacks, and the handle's state."""
import ctypes
import functools

import numpy as np
import pytest

from _prune41_helpers import (COARSE_CAP, E2E_QUERY_SEED, SURV_CAP, SURV_STAGE, big_rows, bytes41, coarse_stats,
                              exact_threshold, gaussian, hook_refine, hook_shadow41, hook_stage1, hook_survivors1,
                              launch_shape41, lower_bound4, lower_bound5_from_parts, mid_rows, mode41, pack_fine,
                              positive_query, quantise_query, shadow41, sums41, survivors, tune_scan41, ulps_apart,
                              upper_bound, width4, width5)
from _prune5_helpers import hook_bounds5, hook_shadow5, mode5
from _prune6_helpers import mode6
from _prune_helpers import mode, query, same, stats
from test_prune5_gpu import bytes5, bytes6, edge_rows, small_counts, tiles_of

pytestmark = pytest.mark.gpu

DIMS = (512, 1024)


def f64(a):
    return np.asarray(a, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def twin_of(dim):
    return shadow41(mid_rows(dim))


@pytest.fixture()
def two(lab_build):
    """every eligible index takes the two-stage path from one row on (the 5-bit path is next in line, from one row on as
    well); the three-launch top-k of small indexes is off; the defaults again afterwards"""
    from seesaw_amd import _lib
    mode(lab_build, True)
    mode6(True, -1)
    mode5(True, 1)
    mode41(True, 1)
    tune_scan41(0, 0)
    _lib.call("ssw_tune_topk", 2)
    try:
        yield lab_build
    finally:
        _lib.call("ssw_tune_topk", 3)
        _lib.call("ssw_tune_surv_cap", -1)
        tune_scan41(0, 0)
        mode41(True, -1)
        mode5(True, -1)
        mode6(True, -1)
        mode(lab_build, True)


def both(lib, idx, fn):
    """fn() with pruning off, then on: (full, pruned, stats after the pruned call)"""
    mode(lib, False)
    full = fn()
    mode(lib, True)
    got = fn()
    return full, got, stats(idx)


def full_scores(lib, idx, q):
    mode(lib, False)
    S = idx.scores(q)
    mode(lib, True)
    return S


def five_bit_bounds(X, q):
    """s5, a5 and k_q5_bounds' lb of the same rows on an index that takes the 5-bit path"""
    from seesaw_amd.device_index import DeviceIndex
    mode41(False)
    idx = DeviceIndex.from_numpy(X)
    try:
        _, s, a = hook_shadow5(idx, codes=False)
        return s, a, hook_bounds5(idx, q, sums=False)["lb"]
    finally:
        idx.close()
        mode41(True, 1)


@pytest.mark.parametrize("dim", DIMS)
def test_builder_against_the_twin(two, dim):
    from seesaw_amd.device_index import DeviceIndex
    X = mid_rows(dim)
    n = X.shape[0]
    th, tb, ts, ta5, ta4 = twin_of(dim)
    s5, a5, _ = five_bit_bounds(X, query(1, dim))
    idx = DeviceIndex.from_numpy(X)
    try:
        h, fine, s, a, a4 = hook_shadow41(idx)
        assert np.array_equal(h.astype(np.int64), th), np.argwhere(h != th)[:4]
        assert np.array_equal(fine, pack_fine(tb))
        assert np.array_equal(s.view(np.uint32), ts.view(np.uint32))
        assert np.array_equal(s.view(np.uint32), s5.view(np.uint32))
        assert np.array_equal(a.view(np.uint32), a5.view(np.uint32))  # k_q5_build's a5, bit for bit
        inf = np.isinf(ta4)
        assert np.array_equal(np.isinf(a4), inf) and np.array_equal(np.isinf(a), inf)
        assert np.all(np.abs(f64(a4[~inf]) - f64(ta4[~inf])) <= 2.0 ** -20 * f64(ta4[~inf]))
        st = stats(idx)
        assert st[0] == 1 and st[5] == bytes41(n, dim), st  # the two-stage shadow is current, and the only one
    finally:
        idx.close()


def check_stage1(idx, X, lib, q, twin=True):
    """One query through k_q41_query + k_q4_bounds against the twin: the query's words and sum D; H integer for integer;
    lb4 against lower_bound4 of the shadow's own nibbles and constants (the builder test holds those to the twin; twin
    True: the nibbles are compared here as well); lb4 <= the device's full-scan score <= ub4 row by row.
    lb4 and the twin's differ by at most one unit in the last place, and almost nowhere: the kernel's s t2q I - w and
    a wQ + s wE are contracted to fused multiply-adds, numpy rounds each product, so the two doubles differ by a few 2^-53
    of |lb| + w, which the padding and the rounding down to f32 carry across a boundary of the f32 grid for one row in
    millions.  (A wrong offset or code norm moves lb4 by thousands of units.)"""
    dim = X.shape[1]
    S = full_scores(lib, idx, q)
    out = hook_stage1(idx, q)
    t = quantise_query(q)
    assert not out["bad"] and not t["bad"]
    got = np.array([out["Q"], out["e"], out["t2"]], np.float32)
    want = np.array([t["Q"], t["e"], t["t2"]], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert out["sumD"] == (int(t["d_hi"].astype(np.int64).sum()), int(t["d_lo"].astype(np.int64).sum()))
    h, _, s, _, a4 = hook_shadow41(idx)
    if twin:
        assert np.array_equal(h.astype(np.int64), shadow41(X)[0])
    lb_twin, w, H = lower_bound4(h.astype(np.int64), s, a4, t)
    assert np.array_equal(out["H"].astype(np.int64), H), np.argwhere(out["H"] != H)[:4]
    fin = np.isfinite(a4)
    assert np.all(out["lb"][~fin] == -np.inf) and np.all(lb_twin[~fin] == -np.inf) and (~fin).sum() == min(2, max(len(X) - 2, 0))
    apart = ulps_apart(out["lb"][fin], lb_twin[fin])
    assert apart.max(initial=0) <= 1 and (apart != 0).sum() <= max(1, fin.sum() // 1000), (dim, len(X), int(apart.max()), int((apart != 0).sum()))
    l, sv, ub = f64(out["lb"])[fin], f64(S)[fin], upper_bound(out["lb"], w)[fin]
    assert np.all(l <= sv) and np.all(sv <= ub), (dim, len(X), np.nonzero(~((l <= sv) & (sv <= ub)))[0][:8])
    return out


def queries_of(seed, dim):
    """a Gaussian query and one without a negative element (the per-query offset of the coarse bound at its largest)"""
    return (query(seed, dim), positive_query(seed + 1000, dim))


@pytest.mark.parametrize("dim", DIMS)
def test_first_stage_at_the_group_edges_of_every_launch_shape(two, dim):
    """16 T g + r rows for g in {0, 1, 3}, r in {0, 1, 15}, the ragged group included; H and lb4 are the same at every shape"""
    from seesaw_amd.device_index import DeviceIndex
    counts = sorted({n for T in tiles_of(dim) for n in small_counts(T)})
    src = np.concatenate([edge_rows(dim), gaussian(max(counts), dim, seed=7)])
    for n in counts:
        X = np.ascontiguousarray(src[:n])
        idx = DeviceIndex.from_numpy(X)
        try:
            for q in queries_of(n, dim):
                ref = None
                for T in tiles_of(dim):
                    for blocks in (1, 2):
                        tune_scan41(blocks, T)
                        assert launch_shape41(idx)[1] == T
                        out = check_stage1(idx, X, two, q) if blocks == 1 else hook_stage1(idx, q)
                        ref = out if ref is None else ref
                        assert np.array_equal(out["lb"].view(np.uint32), ref["lb"].view(np.uint32)), (dim, n, T, blocks)
                        assert np.array_equal(out["H"], ref["H"]), (dim, n, T, blocks)
        finally:
            tune_scan41(0, 0)
            idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_first_stage_many_groups(two, dim):
    """100 008 rows: every wave of the grid walks several groups"""
    from seesaw_amd.device_index import DeviceIndex
    X = big_rows(dim)
    idx = DeviceIndex.from_numpy(X)
    try:
        for q in queries_of(5, dim):
            ref = None
            for T in tiles_of(dim):
                for blocks in (1, 2):
                    tune_scan41(blocks, T)
                    out = check_stage1(idx, X, two, q, twin=False) if ref is None else hook_stage1(idx, q)
                    ref = out if ref is None else ref
                    assert np.array_equal(out["lb"].view(np.uint32), ref["lb"].view(np.uint32)), (dim, T, blocks)
                    assert np.array_equal(out["H"], ref["H"]), (dim, T, blocks)
    finally:
        tune_scan41(0, 0)
        idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_refine_gives_the_five_bit_scans_bound_bit_for_bit(two, dim):
    """list mode (every row once, shuffled), a list with repeats that ends on the last row of a ragged tile, and dense
    mode forced with a coarse cap of 1; B against the twin; the survivors are the twin's"""
    from seesaw_amd.device_index import DeviceIndex
    X = np.ascontiguousarray(mid_rows(dim)[:20_003])  # 20 003 = 16 * 1250 + 3: the last tile is ragged
    n = X.shape[0]
    q = query(21, dim)
    s5, a5, lb_ref = five_bit_bounds(X, q)
    h, b, _, _, _ = shadow41(X)
    t = quantise_query(q)
    _, B, _ = sums41(h, b, t)
    w5 = width5(s5, a5, t, dim)
    ub = upper_bound(lb_ref, w5)
    T = np.float32(np.sort(ub[np.isfinite(ub)])[-300])  # a threshold a few hundred upper bounds reach
    want = survivors(lb_ref, w5, T)
    assert 200 <= want.size < n // 2
    idx = DeviceIndex.from_numpy(X)
    try:
        hook_stage1(idx, q)
        rows = np.random.default_rng(0).permutation(n).astype(np.uint32)
        lb5, Bd, cnt, surv = hook_refine(idx, rows, T, 100)
        assert np.array_equal(lb5.view(np.uint32), lb_ref[rows].view(np.uint32))
        assert np.array_equal(Bd.astype(np.int64), B[rows])
        assert cnt == want.size and np.array_equal(np.sort(surv), want)
        rep = np.concatenate([rows[:777], rows[:777], [n - 1, n - 1, 0, n - 1]]).astype(np.uint32)
        lb5, Bd, cnt, surv = hook_refine(idx, rep, T, 100)
        assert np.array_equal(lb5.view(np.uint32), lb_ref[rep].view(np.uint32))
        assert cnt == np.isin(rep, want).sum() and set(surv.tolist()) == set(rep[np.isin(rep, want)].tolist())
        mode41(True, 1, 1)  # more than one listed row: every row is walked instead
        lb5, Bd, cnt, surv = hook_refine(idx, rows[:5], T, 100, dense=True)
        assert np.array_equal(lb5.view(np.uint32), lb_ref.view(np.uint32))
        assert np.array_equal(Bd.astype(np.int64), B)
        assert cnt == want.size and np.array_equal(np.sort(surv), want)
    finally:
        mode41(True, 1)
        idx.close()


def test_a_blocks_stage_is_flushed_and_used_again(two):
    """one block walks all 20 008 rows and finds thousands of survivors, several times SURV_STAGE: the list is the
    twin's set, each row once; the product's grid gives the same set"""
    from seesaw_amd.device_index import DeviceIndex
    dim = 512
    X = mid_rows(dim)
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(E2E_QUERY_SEED, dim)
        out = hook_stage1(idx, q)
        _, _, s, _, a4 = hook_shadow41(idx, planes=False)
        w4 = width4(s, a4, quantise_query(q), dim)
        T = np.sort(out["lb"][np.isfinite(out["lb"])])[-50]
        want = survivors(out["lb"], w4, T)
        assert want.size > 4 * SURV_STAGE, want.size
        for blocks in (1, 3, 0):
            cnt, rows = hook_survivors1(idx, T, 100, blocks)
            assert cnt == want.size and np.array_equal(np.sort(rows.astype(np.int64)), want), (blocks, cnt, want.size)
    finally:
        idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_pruned_equals_full(two, dim):
    """100 008 rows (rows 2 and 3 score inf / NaN), k = 1, 100 and 1000, with and without exclusions; then a query
    without a negative element"""
    from seesaw_amd.device_index import DeviceIndex
    X = big_rows(dim)
    n = X.shape[0]
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(E2E_QUERY_SEED, dim)
        calls = 0
        for k in (1, 100, 1000):
            for ex in (None, np.arange(0, n, 7)):
                full, got, st = both(two, idx, lambda: idx.topk(q, k, excluded=ex))
                calls += 1
                same(full, got)
                cs = coarse_stats(idx)
                assert len(got[0]) == k and st[0] == 1 and st[3] == calls and st[4] == 0, (k, st)
                assert k <= st[2] <= SURV_CAP and st[2] <= cs[0] <= COARSE_CAP, (k, st, cs)
                assert cs[1] == 0 and cs[2] == calls, cs  # no dense refine at the default cap
                if ex is not None:
                    assert not np.isin(got[0], ex).any()
        assert st[5] == bytes41(n, dim)  # no 5-bit, 6-bit or int8 shadow
        qp = positive_query(E2E_QUERY_SEED + 1000, dim)
        for ex in (None, np.arange(0, n, 7)):
            full, got, st = both(two, idx, lambda: idx.topk(qp, 100, excluded=ex))
            calls += 1
            same(full, got)
            cs = coarse_stats(idx)
            assert st[3] == calls and st[4] == 0 and 100 <= st[2] <= cs[0] <= COARSE_CAP and cs[1] == 0, (st, cs)
        # the same call with the refine forced dense
        mode41(True, 1, 1)
        full, got, st = both(two, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[4] == 0 and coarse_stats(idx)[1] == 1
        mode41(True, 1)
        # the buffer after a pruned call: every reader sees the full scan's
        want = full_scores(two, idx, q)
        idx.topk(q, 100)
        assert np.array_equal(idx.gather_scores(np.arange(n, dtype=np.int64)).view(np.uint32), want.view(np.uint32))
    finally:
        mode41(True, 1)
        idx.close()


def test_the_calls_survivors_are_the_twins(two):
    """the threshold from the coarse bounds' candidates, the first stage's count and the refine's, against the twin"""
    from seesaw_amd.device_index import DeviceIndex
    dim, k = 512, 100
    X = mid_rows(dim)
    idx = DeviceIndex.from_numpy(X)
    try:
        for q in queries_of(E2E_QUERY_SEED, dim):
            S = full_scores(two, idx, q)
            out = hook_stage1(idx, q)
            h, b, s, a5, _ = twin_of(dim)
            _, _, ds, da5, da4 = hook_shadow41(idx, planes=False)
            t = quantise_query(q)
            w4 = width4(ds, da4, t, dim)
            _, B, sumD = sums41(h, b, t)
            lb5, w5, _ = lower_bound5_from_parts(out["H"], B, sumD, ds, da5, t, dim)
            T, T_lb, T_x = exact_threshold(out["lb"], S, k)
            assert T_lb < T_x and T == T_x
            s1 = survivors(out["lb"], w4, T)
            lb5_dev, _, _, _ = hook_refine(idx, s1.astype(np.uint32), T, k)
            s2 = s1[~(upper_bound(lb5_dev, w5[s1]) < np.float64(T))]
            idx.topk(q, k)
            st, cs = stats(idx), coarse_stats(idx)
            assert cs[0] == s1.size and st[2] == s2.size and k <= s2.size < s1.size, (st, cs, s1.size, s2.size)
    finally:
        idx.close()


def test_small_indexes_pruned_equal_full(two):
    from seesaw_amd.device_index import DeviceIndex
    for dim in DIMS:
        for n in small_counts(max(tiles_of(dim))):
            idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=n))
            try:
                q = query(n, dim)
                for k in (1, 100):
                    full, got, st = both(two, idx, lambda: idx.topk(q, k))
                    same(full, got)
                    assert st[0] == 1 and (st[2] == -1) == (n < k), (dim, n, k, st)
            finally:
                idx.close()


def test_duplicates_fall_back_and_a_stale_shadow_is_rebuilt(two):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 60_000
    X = gaussian(n, dim, seed=4)
    q = query(9, dim)
    X[1000:31000] = (q * 0.9).astype(np.float32)  # 30 000 duplicate rows at the top: the threshold selection overflows
    idx = DeviceIndex.from_numpy(X)
    try:
        full, got, st = both(two, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert got[0][0] == 1000 and st[2] == -1 and st[4] == 1, st
        fresh = gaussian(30000, dim, seed=5)
        _lib.call("ssw_index_upload", idx._h, fresh.ctypes.data_as(ctypes.c_void_p), 1000, fresh.shape[0])
        assert stats(idx)[0] == 2  # stale
        full, got, st = both(two, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and st[2] >= 100 and st[5] == bytes41(n, dim), st
        one = (q * 1.5).astype(np.float32)[None, :]
        _lib.call("ssw_index_upload", idx._h, one.ctypes.data_as(ctypes.c_void_p), n - 5, 1)
        full, got, st = both(two, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert got[0][0] == n - 5 and st[2] >= 100
    finally:
        idx.close()


def test_fewer_than_k_finite_candidates_and_queries_that_cannot_be_bounded(two):
    """(a query with a non-finite element never reaches a scan: the entry refuses it, pruned or not; the queries the
    kernels flag are the zero query and one whose norm passes 2^40)"""
    from seesaw_amd.device_index import DeviceIndex
    dim, n, k = 512, 3000, 100
    X = gaussian(n, dim, seed=8)
    X[60:, 3] = np.nan
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(3, dim)
        full, got, st = both(two, idx, lambda: idx.topk(q, k))
        same(full, got)
        assert st[2] == n and st[4] == 0, st  # T = -inf: every row survives both stages
    finally:
        idx.close()
    idx = DeviceIndex.from_numpy(gaussian(5000, dim, seed=9))
    try:
        bad = query(3, dim)
        bad[17] = np.inf
        with pytest.raises(Exception, match="non-finite"):
            idx.topk(bad, k)
        for fb, q in enumerate((query(3, dim) * np.float32(2.0 ** 45), np.zeros(dim, np.float32)), start=1):
            full, got, st = both(two, idx, lambda: idx.topk(q, k))
            same(full, got)
            assert st[2] == -1 and st[4] == fb, st  # the flagged query takes the full scan
    finally:
        idx.close()


def test_more_final_survivors_than_a_lowered_cap_fall_back(two):
    """ssw_tune_surv_cap below the refine's survivors: the call is the full scan's, counted as a fallback; with T = -inf
    the refine lists every row it is given"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    dim = 512
    X = mid_rows(dim)
    n = X.shape[0]
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(2, dim)
        _, got, st = both(two, idx, lambda: idx.topk(q, 100))
        assert st[2] >= 100 and st[4] == 0, st
        _lib.call("ssw_tune_surv_cap", int(st[2]) - 1)
        full, got, st = both(two, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[2] == -1 and st[4] == 1, st
        _lib.call("ssw_tune_surv_cap", -1)
        hook_stage1(idx, q)
        _, _, cnt, surv = hook_refine(idx, np.arange(n, dtype=np.uint32), -np.inf, 100)
        assert cnt == n and np.array_equal(np.sort(surv), np.arange(n))
    finally:
        _lib.call("ssw_tune_surv_cap", -1)
        idx.close()


def test_refusal_for_memory_falls_through_to_the_five_bit_shadow(two):
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 50_000
    idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=12))
    try:
        q = query(4, dim)
        mode5(False)
        mode(two, True, -1, 1 << 50)  # no shadow leaves this reserve free
        full = idx.topk(q, 100)
        st = stats(idx)
        assert st[0] == 0 and st[3] == 0 and st[5] == 0, st  # refused: no shadow is in use, the call was the full scan
        mode(two, True)
        mode5(True, 1)  # the refusal holds until the rows change: the next shadow in line is the 5-bit one
        got = idx.topk(q, 100)
        same(full, got)
        st = stats(idx)
        assert st[0] == 1 and st[3] == 1 and st[4] == 0 and st[5] == bytes5(n, dim), st
        assert coarse_stats(idx)[2] == 0
    finally:
        idx.close()


def test_other_indexes_keep_their_paths(two):
    """an image map, f16 rows, dims 256 and 768, and an index below the two-stage path's row count"""
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 50_000
    mode6(True, 1)
    idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=13))
    try:
        q = query(6, dim)
        idx.set_row2image((np.arange(n, dtype=np.int64) // 3).astype(np.int32))
        full, got, st = both(two, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and st[3] == 1 and st[5] == bytes6(n, dim), st  # the 6-bit shadow alone
        with pytest.raises(Exception, match="two-stage"):
            hook_shadow41(idx)
    finally:
        idx.close()
    for d, dtype in ((512, np.float16), (256, np.float32), (768, np.float32)):
        idx = DeviceIndex.synthetic(20_000, d, seed=d, dtype=dtype)
        try:
            full, got, st = both(two, idx, lambda: idx.topk(query(1, d), 50))
            same(full, got)
            assert st[0] == 1 and st[5] == bytes6(20_000, d), (d, dtype, st)
        finally:
            idx.close()
    mode41(True, n + 1)  # below min_rows: the 5-bit path, as the 5-bit tests set it
    idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=14))
    try:
        full, got, st = both(two, idx, lambda: idx.topk(query(8, dim), 100))
        same(full, got)
        assert st[0] == 1 and st[5] == bytes5(n, dim) and coarse_stats(idx)[2] == 0, st
    finally:
        mode41(True, 1)
        idx.close()
