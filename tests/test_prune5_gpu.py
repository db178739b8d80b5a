"""GPU: the packed 5-bit shadow of single queries on large f32 indexes without an image map and its exact threshold
(csrc/prune.hip, "5-bit shadow"), on the lab build, which reaches the path on small indexes through ssw_tune_prune5: the
builder and the scan's integer sums against the numpy twin, the certificate row by row against the device's full scan,
every launch shape, pruned == full byte for byte through the fallbacks, the threshold against the twin's, and the
handle's state."""
import ctypes

import numpy as np
import pytest

from _prune5_helpers import (SURV_CAP, exact_threshold, hook_bounds5, hook_shadow5, hook_survivors5, integer_sums,
                             launch_shape5, mode5, quantise_query, shadow5, survivors, tune_scan5, upper_bound, width5)
from _prune6_helpers import mode6
from _prune_helpers import mode, query, same, stats

pytestmark = pytest.mark.gpu

DIMS = (512, 1024)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def bytes5(n, dim):
    return (n + 15) // 16 * 16 * (dim * 5 // 8 + 8)


def bytes6(n, dim):
    return (n + 15) // 16 * 16 * (dim * 3 // 4 + 8)


@pytest.fixture()
def five(lab_build):
    """every eligible index takes the 5-bit path from one row on, the three-launch top-k of small indexes (it never
    prunes) is off; the defaults again afterwards"""
    from seesaw_amd import _lib
    mode(lab_build, True)
    mode6(True, -1)
    mode5(True, 1)
    tune_scan5(0, 0)
    _lib.call("ssw_tune_topk", 2)
    try:
        yield lab_build
    finally:
        _lib.call("ssw_tune_topk", 3)
        tune_scan5(0, 0)
        mode5(True, -1)
        mode6(True, -1)
        mode(lab_build, True)


def both5(lib, idx, fn):
    """fn() with pruning off, then on the 5-bit path: (full, pruned, stats after the pruned call)"""
    mode(lib, False)
    full = fn()
    mode(lib, True)
    got = fn()
    return full, got, stats(idx)


def edge_rows(dim):
    """all-zero, one huge element, an inf, a NaN, and a row whose max lands exactly on a code boundary"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X[0] = 0
    X[1, 7] = 3.0e4
    X[2, 9] = np.inf
    X[3, 0] = np.nan
    X[4] = (rng.integers(-30, 31, dim) / 2.0 * 2.0 ** -7).astype(np.float32)
    X[4, 5] = 15 * 2.0 ** -7
    return X


def gaussian(n, dim, seed):
    X = np.random.default_rng(seed).standard_normal((n, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(X)


def big_rows(dim):
    """5 edge rows + 100 003 unit Gaussian rows"""
    return np.ascontiguousarray(np.concatenate([edge_rows(dim), gaussian(100_003, dim, seed=dim)]))


def small_counts(T):
    """16 T g + r for g in {0, 1, 3}, r in {0, 1, 15}: whole groups of a wave's request, a ragged group, both"""
    return sorted({16 * T * g + r for g in (0, 1, 3) for r in (0, 1, 15)} - {0})


def tiles_of(dim):
    return (1, 2) if dim == 512 else (1,)


def check_against_twin(idx, X, lib):
    """codes, s5 and I integer for integer, a5 within its band, lb <= exact score <= ub row by row"""
    n, dim = X.shape
    c, s, a = hook_shadow5(idx)
    tc, ts, ta = shadow5(X)
    assert np.array_equal(c, tc), np.argwhere(c != tc)[:4]
    assert np.array_equal(s.view(np.uint32), ts.view(np.uint32))
    inf = np.isinf(ta)
    assert np.array_equal(np.isinf(a), inf)
    assert np.all(np.abs(f64(a[~inf]) - f64(ta[~inf])) <= 2.0 ** -20 * f64(ta[~inf]))
    st = stats(idx)
    assert st[0] == 1 and st[5] == bytes5(n, dim), st  # the 5-bit shadow is current, and the only one
    for qi in range(2):
        q = query(60 + qi, dim) * np.float32(1.0 if qi == 0 else 2.0 ** -9)
        mode(lib, False)
        S = idx.scores(q)  # the device's full scan
        mode(lib, True)
        out = hook_bounds5(idx, q)
        t = quantise_query(q)
        assert not out["bad"] and not t["bad"]
        assert np.array_equal(out["codes"][0], t["d_hi"]) and np.array_equal(out["codes"][1], t["d_lo"])
        got = np.array([out["Q"], out["e"], out["t2"]], np.float32)
        want = np.array([t["Q"], t["e"], t["t2"]], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
        I = integer_sums(c, t)
        assert np.array_equal(out["I"], I), (dim, n, np.argwhere(out["I"] != I)[:4])
        fin = ~inf
        w = width5(s, a, t, dim)
        l, sv, ub = f64(out["lb"])[fin], f64(S)[fin], upper_bound(out["lb"], w)[fin]
        assert np.all(out["lb"][inf] == -np.inf)
        assert np.all(l <= sv) and np.all(sv <= ub), (dim, n, np.nonzero(~((l <= sv) & (sv <= ub)))[0][:8])


@pytest.mark.parametrize("dim", DIMS)
def test_shadow_sums_and_certificate_against_the_twin(five, dim):
    from seesaw_amd.device_index import DeviceIndex
    X = big_rows(dim)
    idx = DeviceIndex.from_numpy(X)
    try:
        check_against_twin(idx, X, five)
    finally:
        idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_group_edges_against_the_twin_at_every_launch_shape(five, dim):
    """the row counts at the ends of a wave's request, for every tile count; lb is the same bits at every launch shape"""
    from seesaw_amd.device_index import DeviceIndex
    counts = sorted({n for T in tiles_of(dim) for n in small_counts(T)})
    src = np.concatenate([edge_rows(dim), gaussian(max(counts), dim, seed=7)])
    for n in counts:
        X = np.ascontiguousarray(src[:n])
        idx = DeviceIndex.from_numpy(X)
        try:
            q, ref = query(n, dim), None
            for T in tiles_of(dim):
                for blocks in (1, 2):
                    tune_scan5(blocks, T)
                    assert launch_shape5(idx)[1] == T
                    if blocks == 1:
                        check_against_twin(idx, X, five)
                    lb = hook_bounds5(idx, q, sums=False)["lb"]
                    ref = lb if ref is None else ref
                    assert np.array_equal(lb.view(np.uint32), ref.view(np.uint32)), (dim, n, T, blocks)
        finally:
            tune_scan5(0, 0)
            idx.close()


def test_lb_identical_at_every_launch_shape_many_groups(five):
    """100 008 rows: every wave of the grid walks several groups"""
    from seesaw_amd.device_index import DeviceIndex
    for dim in DIMS:
        idx = DeviceIndex.from_numpy(big_rows(dim))
        try:
            q, ref = query(5, dim), None
            for T in tiles_of(dim):
                for blocks in (1, 2):
                    tune_scan5(blocks, T)
                    lb = hook_bounds5(idx, q, sums=False)["lb"]
                    ref = lb if ref is None else ref
                    assert np.array_equal(lb.view(np.uint32), ref.view(np.uint32)), (dim, T, blocks)
        finally:
            tune_scan5(0, 0)
            idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_pruned_equals_full(five, dim):
    """k = 1, 100 and 4096; exclusions; rows that score NaN; an excluded set that leaves fewer than k rows"""
    from seesaw_amd.device_index import DeviceIndex
    X = big_rows(dim)  # rows 2 and 3 score inf / NaN
    n = X.shape[0]
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(11, dim)
        calls = 0
        for k in (1, 100, 4096):
            full, got, st = both5(five, idx, lambda: idx.topk(q, k))
            calls += 1
            same(full, got)
            assert len(got[0]) == k and st[0] == 1 and st[3] == calls and st[4] == 0 and k <= st[2] < SURV_CAP, (k, st)
        assert st[5] == bytes5(n, dim)  # no 6-bit, no int8 shadow
        ex = np.concatenate([full[0][:50], np.arange(0, n, 7)])
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100, excluded=ex))
        same(full, got)
        assert st[4] == 0 and not np.isin(got[0], ex).any()
        keep = np.random.default_rng(0).choice(n, 40, replace=False)
        few = np.setdiff1d(np.arange(n), keep)
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100, excluded=few))
        same(full, got)
        assert len(got[0]) == 40 and st[2] == -1 and st[4] == 1, st
        # the buffer after a pruned call: every reader sees the full scan's
        mode(five, False)
        want = idx.scores(q)
        mode(five, True)
        idx.topk(q, 100)
        assert np.array_equal(idx.gather_scores(np.arange(n, dtype=np.int64)).view(np.uint32), want.view(np.uint32))
    finally:
        idx.close()


def test_small_indexes_pruned_equal_full(five):
    """the ends of the scan's loop through the whole call (fewer rows than k: the fallback)"""
    from seesaw_amd.device_index import DeviceIndex
    for dim in DIMS:
        for n in small_counts(max(tiles_of(dim))):
            idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=n))
            try:
                q = query(n, dim)
                for k in (1, 100):
                    full, got, st = both5(five, idx, lambda: idx.topk(q, k))
                    same(full, got)
                    assert st[0] == 1 and (st[2] == -1) == (n < k), (dim, n, k, st)
            finally:
                idx.close()


def test_duplicates_fall_back_and_a_stale_shadow_is_rebuilt(five):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 60_000
    X = gaussian(n, dim, seed=4)
    q = query(9, dim)
    X[1000:21000] = (q * 0.9).astype(np.float32)  # mass ties at the top: the threshold selection overflows
    idx = DeviceIndex.from_numpy(X)
    try:
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert got[0][0] == 1000 and st[2] == -1 and st[4] == 1, st
        fresh = gaussian(20000, dim, seed=5)
        _lib.call("ssw_index_upload", idx._h, fresh.ctypes.data_as(ctypes.c_void_p), 1000, fresh.shape[0])
        assert stats(idx)[0] == 2  # stale
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and st[2] >= 100, st
        one = (q * 1.5).astype(np.float32)[None, :]
        _lib.call("ssw_index_upload", idx._h, one.ctypes.data_as(ctypes.c_void_p), n - 5, 1)
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert got[0][0] == n - 5 and st[2] >= 100
    finally:
        idx.close()


def test_exact_threshold_above_the_kth_lower_bound(five):
    """T_x > T_lb strictly, and the call's survivors are the twin's rows with ub >= T_x; the survivor kernel with the
    5-bit code norm lists that very set"""
    from seesaw_amd.device_index import DeviceIndex
    dim, k = 512, 100
    X = big_rows(dim)
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(21, dim)
        mode(five, False)
        S = idx.scores(q)
        mode(five, True)
        _, s, a = hook_shadow5(idx, codes=False)
        out = hook_bounds5(idx, q, sums=False)
        w = width5(s, a, quantise_query(q), dim)
        for ex in (None, np.argsort(-np.nan_to_num(S, nan=-9.0))[:30]):  # ... and with the best rows excluded
            T, T_lb, T_x = exact_threshold(out["lb"], S, k, excluded=ex)
            assert T_lb < T_x and T == T_x
            want = survivors(out["lb"], w, T)
            idx.topk(q, k, excluded=ex)
            st = stats(idx)
            assert st[2] == want.size and st[2] < survivors(out["lb"], w, T_lb).size, (st, want.size)
        hook_bounds5(idx, q, sums=False)
        pub, got, rows = hook_survivors5(idx, T, k)
        assert pub == got == want.size and np.array_equal(np.sort(rows), want)
    finally:
        idx.close()


def test_fewer_than_k_finite_candidate_scores(five):
    """most rows hold a NaN: they score NaN and cannot be bounded.  The candidates hold fewer than k scores that are not
    NaN, so T_x = -inf and T = T_lb = -inf: every row survives and the result is the full scan's"""
    from seesaw_amd.device_index import DeviceIndex
    dim, n, k = 512, 3000, 100
    X = gaussian(n, dim, seed=8)
    X[60:, 3] = np.nan
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(3, dim)
        mode(five, False)
        S = idx.scores(q)
        mode(five, True)
        lb = hook_bounds5(idx, q, sums=False)["lb"]
        T, T_lb, T_x = exact_threshold(lb, S, k)
        assert T_x == -np.inf and T_lb == -np.inf and T == T_lb
        full, got, st = both5(five, idx, lambda: idx.topk(q, k))
        same(full, got)
        assert st[2] == n and st[4] == 0, st
    finally:
        idx.close()


def test_refusal_for_memory_falls_through_to_the_six_bit_shadow(five):
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 50_000
    idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=12))
    try:
        q = query(4, dim)
        mode(five, True, -1, 1 << 50)  # no shadow leaves this reserve free
        full = idx.topk(q, 100)
        st = stats(idx)
        assert st[0] == 0 and st[3] == 0 and st[5] == 0, st  # refused: no shadow is in use, the call was the full scan
        mode(five, True)
        mode6(True, 1)  # the refusal holds until the rows change: the next shadow in line is the 6-bit one
        got = idx.topk(q, 100)
        same(full, got)
        st = stats(idx)
        assert st[0] == 1 and st[3] == 1 and st[4] == 0 and st[5] == bytes6(n, dim), st
    finally:
        idx.close()


def test_an_index_with_an_image_map_never_takes_the_path(five):
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 50_000
    idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=13))
    try:
        q = query(6, dim)
        mode6(True, 1)
        idx.set_row2image((np.arange(n, dtype=np.int64) // 3).astype(np.int32))
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and st[3] == 1 and st[5] == bytes6(n, dim), st  # the 6-bit shadow alone
        with pytest.raises(Exception, match="5-bit"):
            hook_shadow5(idx)
        idx.set_row2image(None)  # without the map the same index takes the 5-bit path
        full, got, st = both5(five, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and st[5] == bytes6(n, dim) + bytes5(n, dim), st
    finally:
        idx.close()


def test_f16_rows_and_other_dims_keep_their_path(five):
    from seesaw_amd.device_index import DeviceIndex
    mode6(True, 1)
    for dim, dtype in ((512, np.float16), (256, np.float32), (768, np.float32)):
        n = 20_000
        idx = DeviceIndex.synthetic(n, dim, seed=dim, dtype=dtype)
        try:
            q = query(1, dim)
            full, got, st = both5(five, idx, lambda: idx.topk(q, 50))
            same(full, got)
            assert st[0] == 1 and st[5] == bytes6(n, dim), (dim, dtype, st)
        finally:
            idx.close()


def test_an_attached_exchange_target_of_small_k_max_keeps_the_path(five):
    """the flagship workload's shape: the selection writes a rank's message with k_max = 128, fewer than the 1024 keys of
    the threshold selection, which writes no message: the call is pruned on the 5-bit shadow and message and result are
    the full scan's"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.sharded import ShardedTopK
    dim, n, k = 512, 50_000, 100
    idx = DeviceIndex.from_numpy(gaussian(n, dim, seed=14))
    try:
        x = ShardedTopK(rank=0, world=1, device=torch.device("cuda", 0), image_offset=0, k_max=128, with_best=False)
        x.attach(idx)
        q = query(8, dim)
        msgs = []

        def call():
            out = idx.topk(q, k)
            torch.cuda.synchronize()
            msgs.append(x.send_buf.cpu().numpy().copy())
            return out
        full, got, st = both5(five, idx, call)
        same(full, got)
        assert np.array_equal(msgs[0], msgs[1])
        assert st[0] == 1 and st[3] == 1 and st[4] == 0 and st[5] == bytes5(n, dim), st
    finally:
        idx.close()
