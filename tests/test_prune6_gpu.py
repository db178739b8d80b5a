"""GPU: the packed 6-bit shadow of single queries on large f32 indexes (csrc/prune.hip, "6-bit shadow"), on the lab build:
the builder against the numpy twin, the lane map of the matrix-core scan on exact integers, the certificate row by row
against the device's full scan, the loop's ends (pruned == full, byte for byte), the fallbacks and the handle's state,
and one index at the product's threshold."""
import numpy as np
import pytest

from _prune6_helpers import (hook_bounds6, hook_shadow6, integer_sums, launch_shape6, mode6, quantise_query, shadow6,
                             width6)
from _prune_batch_helpers import edge_queries
from _prune_helpers import adversarial_rows, mode, query, same, stats

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
SURV_CAP = 1 << 18


def f64(a):
    return np.asarray(a, dtype=np.float64)


@pytest.fixture()
def six(lab_build):
    """every f32 index takes the 6-bit path from one row on; the defaults again afterwards"""
    mode(lab_build, True)
    mode6(True, 1)
    try:
        yield lab_build
    finally:
        mode6(True, -1)
        mode(lab_build, True)


def shape(dim):
    """(G rows of one request of a wave, W waves of a full launch)"""
    from seesaw_amd.device_index import DeviceIndex
    probe = DeviceIndex(1 << 20, dim)
    try:
        blocks, tiles = launch_shape6(probe)
    finally:
        probe.close()
    return 16 * tiles, 4 * blocks


def float_rows(n, dim, seed):
    """Gaussian rows of mixed scale with the adversarial rows over the first rows, a tile boundary and the last rows"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    adv = adversarial_rows(rng, dim)
    m = adv.shape[0]
    X[:min(m, n)] = adv[:min(m, n)]
    if n >= 6 * m:
        at = ((n // 2) // 16) * 16 - m // 2  # straddles a tile boundary
        X[at:at + m] = adv
    if n >= 2 * m:
        X[n - m:] = adv[::-1]
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("n,dim", [((1 << 16) + 1, 256), (100_003, 512), ((1 << 16) + 1, 1024)])
def test_shadow_equals_the_twin(six, n, dim):
    from seesaw_amd.device_index import DeviceIndex
    X = float_rows(n, dim, seed=dim)
    idx = DeviceIndex.from_numpy(X)
    try:
        c, s, a = hook_shadow6(idx)
        tc, ts, ta = shadow6(X)
        assert np.array_equal(c, tc), np.argwhere(c != tc)[:4]
        assert np.array_equal(s.view(np.uint32), ts.view(np.uint32))
        inf = np.isinf(ta)
        assert np.array_equal(np.isinf(a), inf) and inf.sum() >= 26
        # a6's double sums are taken in the device's order: the band of the int8 shadow's test
        assert np.all(np.abs(f64(a[~inf]) - f64(ta[~inf])) <= 2.0 ** -20 * f64(ta[~inf])), dim
        st = stats(idx)
        assert st[0] == 1 and st[5] == (n + 15) // 16 * 16 * (dim * 3 // 4 + 8), st  # 6-bit bytes, no int8 shadow
    finally:
        idx.close()


def int_rows(n, dim, seed):
    """f32 rows that ARE their codes: integers in [-31, 31], every row with a 31 (s6 = 1), all patterns different"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-31, 32, (n, dim)).astype(np.float32)
    X[np.arange(n), np.arange(n) % dim] = 31.0
    return X


@pytest.mark.parametrize("dim", DIMS)
def test_lane_map_on_exact_integers(six, dim):
    """every I of the scan equals the numpy integer dot.  The kernel itself was not mutated.  That these rows and queries
    tell a wrong lane map apart is checked on the numpy twin's packed bytes only (tests/test_prune6_cpu.py,
    test_integer_rows_expose_a_wrong_placement): rows r and r ^ 1 of a tile swapped, lane groups 1 and 2 swapped, and the
    low-bit bytes of a k-step rotated each change some I."""
    from seesaw_amd.device_index import DeviceIndex
    G, W = shape(dim)
    rng = np.random.default_rng(5)
    qs = [rng.integers(-3, 4, dim).astype(np.float32), edge_queries(rng, dim)[3], rng.standard_normal(dim).astype(np.float32)]
    for n in (1, 17, G + 1, W * G + 1, 50_003):
        X = int_rows(n, dim, seed=n)
        idx = DeviceIndex.from_numpy(X)
        try:
            c, s, _ = hook_shadow6(idx)
            assert np.array_equal(c, X.astype(np.int8)) and np.all(s == 1)
            for q in qs:
                out = hook_bounds6(idx, q)
                t = quantise_query(q)
                assert not out["bad"] and not t["bad"]
                assert np.array_equal(out["codes"][0], t["d_hi"]) and np.array_equal(out["codes"][1], t["d_lo"])
                got = np.array([out["Q"], out["e"], out["t2"]], np.float32)
                want = np.array([t["Q"], t["e"], t["t2"]], np.float32)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
                I = integer_sums(c, t)
                assert np.array_equal(out["I"], I), (dim, n, np.argwhere(out["I"] != I)[:4])
        finally:
            idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_certificate_row_by_row(six, dim):
    from seesaw_amd.device_index import DeviceIndex
    G, W = shape(dim)
    rng = np.random.default_rng(11)
    Q = edge_queries(rng, dim) + [query(40 + i, dim) * np.float32(2.0 ** (7 * i - 10)) for i in range(4)]
    for n in (17, G - 1, W * G + 1, 100_003):
        X = float_rows(n, dim, seed=n)
        idx = DeviceIndex.from_numpy(X)
        try:
            mode(six, False)
            S = [idx.scores(q) for q in Q]  # the device's full scan
            mode(six, True)
            _, s, a = hook_shadow6(idx, codes=False)
            fin = np.isfinite(a)
            rows = np.nonzero(fin)[0]
            for q, Sq in zip(Q, S):
                out = hook_bounds6(idx, q, sums=False)
                t = quantise_query(q)
                assert not t["bad"] and not out["bad"]
                assert np.all(out["lb"][~fin] == -np.inf), (dim, n)
                w = width6(s, a, t, dim)[fin]
                l, sv = f64(out["lb"])[fin], f64(Sq)[fin]
                assert np.all(np.isfinite(l)) and np.all(np.isfinite(sv)), (dim, n)
                assert np.all(l < sv), (dim, n, rows[~(l < sv)][:8])
                slack = 2 * w * (1 + 2.0 ** -19) + np.abs(l) * 2.0 ** -19 + 2.0 ** -98
                wide = ~(sv - l <= slack)
                assert not wide.any(), (dim, n, rows[wide][:8], float(((sv - l) / slack).max()))
        finally:
            idx.close()


def edge_rows(n, dim, seed):
    """unit Gaussian rows; at the ragged edge rows with norms 2^40 apart and rows that cannot be bounded"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    tail = min(n, 6)
    for i in range(tail):
        X[n - 1 - i] *= np.float32(2.0 ** (20 if i % 2 else -20))
    if n >= 4:
        X[n - 2, 1] = np.inf
        X[n - 4] *= np.float32(2.0 ** 70)
    return np.ascontiguousarray(X)


def both6(lib, idx, fn):
    """fn() with pruning off, then on the 6-bit path: (full, pruned, stats after the pruned call)"""
    mode(lib, False)
    full = fn()
    mode(lib, True)
    got = fn()
    return full, got, stats(idx)


@pytest.mark.parametrize("dim", DIMS)
def test_loop_ends_pruned_equals_full(six, dim):
    """with the three-launch top-k of small indexes switched off (ssw_tune_topk(2)): it never prunes"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    G, W = shape(dim)
    counts = sorted({1, 15, 16, 17, G - 1, G + 1, W * G - 1, W * G + 1, 2 * W * G + 5, 3 * W * G - G + 3})
    try:
        _lib.call("ssw_tune_topk", 2)
        for n in counts:
            idx = DeviceIndex.from_numpy(edge_rows(n, dim, seed=n))
            try:
                q = query(n, dim)
                for calls, k in enumerate((1, 100), 1):
                    full, got, st = both6(six, idx, lambda: idx.topk(q, k))
                    same(full, got)
                    assert st[0] == 1 and st[3] == calls, (dim, n, k, st)  # the shadow is current, the call was pruned
                if n >= 3:  # multi-row images, a seventh of them excluded
                    idx.set_row2image((np.arange(n, dtype=np.int64) // 3).astype(np.int32))
                    ex = np.arange(0, (n + 2) // 3, 7)
                    for calls, k in enumerate((1, 100), 3):
                        full, got, st = both6(six, idx, lambda: idx.topk(q, k, excluded=ex))
                        same(full, got)
                        assert st[3] == calls, (dim, n, k, st)
            finally:
                idx.close()
    finally:
        _lib.call("ssw_tune_topk", 3)


def test_fallbacks_and_state(six):
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, SURV_CAP + 4096
    rng = np.random.default_rng(2)
    row = rng.standard_normal(dim).astype(np.float32) / np.float32(np.sqrt(dim))
    X = np.tile(row, (n, 1))  # identical rows: every one reaches the threshold -> more than SURV_CAP survivors
    X[::1000] *= np.float32(1.5)
    idx = DeviceIndex.from_numpy(X)
    try:
        q = query(1, dim)
        full, got, st = both6(six, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[2] == -1 and st[4] == 1, st
    finally:
        idx.close()
    n = 200_000
    idx = DeviceIndex.synthetic(n, dim, seed=9)
    try:
        q = query(2, dim)
        full, got, st = both6(six, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and 100 <= st[2] <= SURV_CAP and st[4] == 0, st
        assert st[5] == (n + 15) // 16 * 16 * (dim * 3 // 4 + 8)  # 6-bit bytes and no int8 shadow
        assert idx.prune_stats()["shadow"] == "current" and idx.prune_stats()["shadow_bytes"] == st[5]
        # the buffer after a pruned call: every reader sees the full scan's
        mode(six, False)
        want_scores, want_top = idx.scores(q), idx.topk(None, 50)
        mode(six, True)
        idx.topk(q, 100)
        same(idx.topk(None, 50), want_top)
        idx.topk(q, 100)
        got_scores = idx.gather_scores(np.arange(n, dtype=np.int64))
        assert np.array_equal(got_scores.view(np.uint32), want_scores.view(np.uint32))
        # queries that cannot be bounded take the full scan
        before = stats(idx)[4]
        z = np.zeros(dim, np.float32)
        full, got, st = both6(six, idx, lambda: idx.topk(z, 10))
        same(full, got)
        assert st[4] == before + 1, st
        # the first pruned batch builds the int8 shadow; its results equal the plain batch's
        mode(six, True, 1)
        Q = np.stack([query(20 + i, dim) for i in range(4)])
        plain = idx.topk_batch(Q, 20)
        pruned = idx.topk_batch(Q, 20, prune=True)
        for a, b in zip(plain, pruned):
            same(a, b)
        assert stats(idx)[5] == (n + 15) // 16 * 16 * (dim * 3 // 4 + 8) + n * (dim + 8)
    finally:
        idx.close()


def test_non_finite_query_takes_the_full_scan(six):
    """a NaN or inf query reaches the pre-scan only through the device entry (ssw_index_topk refuses it on the host):
    k_q6_query flags it, the call is the full scan's bit for bit and `fallbacks` counts it"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 256, 100_000
    idx = DeviceIndex.synthetic(n, dim, seed=4)
    try:
        for v in (np.nan, np.inf, -np.inf):
            q = query(3, dim)
            q[17] = v
            with pytest.raises(Exception, match="non-finite"):
                idx.topk(q, 10)
            assert hook_bounds6(idx, q, sums=False)["bad"]
            qd = torch.from_numpy(q).cuda()
            torch.cuda.synchronize()
            mode(six, False)
            idx.topk_dev(qd.data_ptr(), 10)
            full = idx.topk_fetch(10)
            mode(six, True)
            before = stats(idx)
            idx.topk_dev(qd.data_ptr(), 10)
            got = idx.topk_fetch(10)
            st = stats(idx)
            same(full, got)
            assert st[3] == before[3] + 1 and st[4] == before[4] + 1 and st[2] == -1, (v, before, st)
    finally:
        idx.close()


def test_product_threshold(lab_build):
    """the default constants: an index of MIN_ROWS (6-bit single call, f32) rows filled on the device is pruned on the 6-bit shadow
    without a fallback and answers with the full scan's bits"""
    from seesaw_amd.device_index import DeviceIndex
    n = 1 << 24
    mode(lab_build, True)
    mode6(True, -1)
    idx = DeviceIndex.synthetic(n, 512, seed=7)
    try:
        for i in range(4):
            q = query(300 + i)
            full, got, st = both6(lab_build, idx, lambda: idx.topk(q, 100))
            same(full, got)
            assert st[0] == 1 and 100 <= st[2] <= SURV_CAP and st[4] == 0, st
            assert st[5] == n * (512 * 3 // 4 + 8), st
            print(f"2^24 rows, query {i}: {st[2]} survivors")
    finally:
        mode(lab_build, True)
        idx.close()
