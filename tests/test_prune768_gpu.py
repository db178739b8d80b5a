"""GPU: the packed 6-bit shadow on dim-768 indexes, f32 and float16 rows (csrc/prune.hip: the C = 3 instantiations of
k_q6_build / k_q6_build_h16 / k_q6_bounds / k_q6_bounds_mq; csrc/index_prune.hip: prune6_eligible with q6_dim_supported;
csrc/rescore_dev.hip: k_rescore_survivors<R, 3>), on the lab build.  tests/test_prune6_gpu.py at the dim that has no int8
shadow:

1. the builder against the numpy twin;
2. the matrix core's lane map on exact integers, single query and chunk;
3. the certificate row by row against the device's own full scan;
4. the ends of the scan's loop: pruned == full, byte for byte, and the call did not silently fall back;
5. the pruned batch against the loop of single calls, and the two-stage batch against the unpruned one;
6. the chunk that never waits, against the plain device batch;
7. the fallbacks;
8. the product's own thresholds, without the lab switches;
9. the int8 side keeps refusing the dim, and ssw_tune_prune's min_rows does not govern it.

Every comparison of results is exact: the pruned path returns the full scan's bits, so there is no tolerance to choose.
The bands of (1) and (3) are those of tests/test_prune6_gpu.py."""
import numpy as np
import pytest

from _prune6_f16_helpers import f16_rows
from _prune768_helpers import (DIM, batch6, hook_bounds6, hook_bounds6_mq, hook_shadow6, integer_sums, launch_shape6,
                               launch_shape6_mq, mode6, quantise_query, shadow6, shadow_bytes, width6)
from _prune_batch_helpers import edge_queries
from _prune_helpers import adversarial_rows, hook_bounds, hook_shadow, mode, query, same, stats

pytestmark = pytest.mark.gpu

SURV_CAP = 1 << 18
DTYPES = [np.float32, np.float16]
# the product's constants (csrc/index_prune.hip): MIN_ROWS of the 6-bit single call and of the 6-bit batch at dim 768
MIN_ROWS_768 = {np.float32: 1 << 20, np.float16: 1 << 20}
BATCH_MIN_ROWS_768 = {np.float32: 1 << 20, np.float16: 1 << 20}


def f64(a):
    return np.asarray(a, dtype=np.float64)


@pytest.fixture()
def six(lab_build):
    """single queries and batches take the 6-bit path from one row on (ssw_tune_prune6(1, 1), ssw_tune_prune6_batch(1));
    ssw_tune_prune stays at its defaults: its min_rows is the int8 shadow's.  The defaults again afterwards."""
    mode(lab_build, True)
    mode6(True, 1)
    batch6(1)
    try:
        yield lab_build
    finally:
        batch6(-1)
        mode6(True, -1)
        mode(lab_build, True)


def unpruned(lib, fn):
    """fn() with the pruning off (the reference), then on again"""
    mode(lib, False)
    try:
        return fn()
    finally:
        mode(lib, True)


def both6(lib, idx, fn):
    """fn() with pruning off, then on the 6-bit path: (full, pruned, stats after the pruned call)"""
    full = unpruned(lib, fn)
    got = fn()
    return full, got, stats(idx)


_SHAPES = {}


def shapes():
    """(G rows of one request of a wave, W waves of a full launch) of k_q6_bounds and of k_q6_bounds_mq at dim 768"""
    if not _SHAPES:
        from seesaw_amd.device_index import DeviceIndex
        probe = DeviceIndex(1 << 20, DIM)  # large enough for an unclamped grid; nothing is computed on it
        try:
            blocks, tiles = launch_shape6(probe)
            blocks_mq, tiles_mq = launch_shape6_mq(probe)
        finally:
            probe.close()
        assert tiles == 1 and tiles_mq == 1, (tiles, tiles_mq)  # the only count two register sets admit at C = 3
        _SHAPES["single"] = (16 * tiles, 4 * blocks)
        _SHAPES["mq"] = (16 * tiles_mq, 4 * blocks_mq)
    return _SHAPES["single"], _SHAPES["mq"]


def make(X, dtype):
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex.from_numpy(X, dtype=dtype)


def float_rows(n, seed):
    """Gaussian rows of mixed scale with the adversarial rows over the first rows, a tile boundary and the last rows"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, DIM)).astype(np.float32) / np.float32(np.sqrt(DIM))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    adv = adversarial_rows(rng, DIM)
    m = adv.shape[0]
    X[:min(m, n)] = adv[:min(m, n)]
    if n >= 6 * m:
        at = ((n // 2) // 16) * 16 - m // 2  # straddles a tile boundary
        X[at:at + m] = adv
    if n >= 2 * m:
        X[n - m:] = adv[::-1]
    return np.ascontiguousarray(X)


def rows_and_twin_input(n, dtype, seed):
    """(what goes up, the f32 rows the index then holds): for float16 the widened rounding of binary16-range rows"""
    if dtype == np.float16:
        return f16_rows(n, DIM, seed=seed)
    X = float_rows(n, seed)
    return X, X


# ---- 1. the builder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [(1 << 16) + 1, 100_003])
def test_shadow_equals_the_twin(six, n, dtype):
    X, W = rows_and_twin_input(n, dtype, seed=n)
    idx = make(X, dtype)
    try:
        assert idx.prune_stats()["eligible"] and idx.prune_stats()["shadow"] == "none"
        c, s, a = hook_shadow6(idx)
        tc, ts, ta = shadow6(W)
        assert np.array_equal(c, tc), np.argwhere(c != tc)[:4]
        assert np.array_equal(s.view(np.uint32), ts.view(np.uint32))
        inf = np.isinf(ta)
        assert np.array_equal(np.isinf(a), inf) and inf.sum() >= 26
        # a6's double sums are taken in the device's order: the band of the int8 and the 6-bit shadow's tests
        assert np.all(np.abs(f64(a[~inf]) - f64(ta[~inf])) <= 2.0 ** -20 * f64(ta[~inf]))
        st = idx.prune_stats()
        padded_rows = (n + 15) // 16 * 16
        assert st["shadow"] == "current" and st["shadow_bytes"] == padded_rows * 584 == shadow_bytes(n), st
    finally:
        idx.close()


# ---- 2. the lane map --------------------------------------------------------------------------------------------------
def int_rows(n, seed):
    """rows that ARE their codes: integers in [-31, 31] (exact in binary16 too), every row with a 31 (s6 = 1)"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-31, 32, (n, DIM)).astype(np.float32)
    X[np.arange(n), np.arange(n) % DIM] = 31.0
    return X


def chunk_queries(seed=5):
    """16 queries, all different in direction and by orders of magnitude in norm"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((16, DIM)) * np.exp2(rng.integers(-12, 13, 16))[:, None]
    Q[3] = edge_queries(rng, DIM)[3]  # rint ties and clamped lo codes
    return np.ascontiguousarray(Q, dtype=np.float32)


def check_query_state(got_codes, got_Qet2, t):
    assert np.array_equal(got_codes[0], t["d_hi"]) and np.array_equal(got_codes[1], t["d_lo"])
    got = np.array(got_Qet2, np.float32)
    want = np.array([t["Q"], t["e"], t["t2"]], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_map_on_exact_integers(six, dtype):
    """every I of both scans equals the numpy integer dot; Q, e, t2 and both code planes equal the twin bit for bit.  That
    these rows and queries tell a wrong lane map apart is checked on the twin's packed bytes
    (tests/test_prune768_cpu.py, test_integer_rows_expose_a_wrong_placement)."""
    (G, W), (Gm, Wm) = shapes()
    rng = np.random.default_rng(5)
    qs = [rng.integers(-3, 4, DIM).astype(np.float32), edge_queries(rng, DIM)[3], rng.standard_normal(DIM).astype(np.float32)]
    single_twins = [quantise_query(q) for q in qs]
    Qall = chunk_queries()
    twins = [quantise_query(q) for q in Qall]
    assert not any(t["bad"] for t in single_twins + twins)
    # |I| <= 768 * 124 * (256 * 127 + 127) < 2^32: the float64 product is the exact integer dot
    D = np.stack([256.0 * t["d_hi"].astype(np.float64) + t["d_lo"].astype(np.float64) for t in twins])
    for n in sorted({1, 17, G + 1, W * G + 1, Gm + 1, Wm * Gm + 1, 50_003}):
        X = int_rows(n, seed=n)
        idx = make(X, dtype)
        try:
            c, s, _ = hook_shadow6(idx)
            assert np.array_equal(c, X.astype(np.int8)) and np.all(s == 1)
            for q, t in zip(qs, single_twins):
                out = hook_bounds6(idx, q)
                assert not out["bad"]
                check_query_state(out["codes"], [out["Q"], out["e"], out["t2"]], t)
                I = integer_sums(c, t)
                assert np.array_equal(out["I"], I), (n, np.argwhere(out["I"] != I)[:4])
            want = ((4.0 * c.astype(np.float64)) @ D.T).T.astype(np.int64)  # [16, n], once for every width
            assert np.array_equal(want[5, :64], integer_sums(c[:64], twins[5]))
            for w in (1, 5, 16):
                sel = slice(16 - w, 16)  # another query in slot 0 every time
                out = hook_bounds6_mq(idx, Qall[sel])
                assert not out["bad"].any()
                for j, t in enumerate(twins[sel]):
                    check_query_state(out["codes"][j], [out["Q"][j], out["e"][j], out["t2"][j]], t)
                assert np.array_equal(out["I"], want[sel]), (n, w, np.argwhere(out["I"] != want[sel])[:4])
            st = stats(idx)
            assert st[0] == 1 and st[5] == shadow_bytes(n), st  # the hooks built the 6-bit shadow and no other
        finally:
            idx.close()


# ---- 3. the certificate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_certificate_row_by_row(six, dtype):
    (G, W), _ = shapes()
    Q = edge_queries(np.random.default_rng(11), DIM)
    assert len(Q) == 8
    twins = [quantise_query(q) for q in Q]
    for n in (17, G - 1, W * G + 1, 50_003):
        X, _ = rows_and_twin_input(n, dtype, seed=n)
        idx = make(X, dtype)
        try:
            S = unpruned(six, lambda: [idx.scores(q) for q in Q])  # the device's full scan
            _, s, a = hook_shadow6(idx, codes=False)
            fin = np.isfinite(a)
            rows = np.nonzero(fin)[0]
            assert fin.any() and (n < 50 or not fin.all())  # bounded rows, and from 49 rows on unbounded ones too
            for q, t, Sq in zip(Q, twins, S):
                out = hook_bounds6(idx, q, sums=False)
                assert not t["bad"] and not out["bad"]
                assert np.all(out["lb"][~fin] == -np.inf), n
                w = width6(s, a, t)[fin]  # with the dim-768 code norm
                l, sv = f64(out["lb"])[fin], f64(Sq)[fin]
                assert np.all(np.isfinite(l)) and np.all(np.isfinite(sv)), n
                assert np.all(l < sv), (n, rows[~(l < sv)][:8])
                slack = 2 * w * (1 + 2.0 ** -19) + np.abs(l) * 2.0 ** -19 + 2.0 ** -98
                wide = ~(sv - l <= slack)
                assert not wide.any(), (n, rows[wide][:8], float(((sv - l) / slack).max()))
        finally:
            idx.close()


# ---- 4. the ends of the loop ------------------------------------------------------------------------------------------
def gaussian_rows(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal((n, DIM)).astype(np.float32) / np.float32(np.sqrt(DIM)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_loop_ends_pruned_equals_full(six, dtype):
    """with the three-launch top-k of small indexes switched off (ssw_tune_topk(2)): it never prunes.  Where k images are
    to be had the call must have been certified: a silent full scan would pass the comparison vacuously."""
    from seesaw_amd import _lib
    (G, W), _ = shapes()
    counts = sorted({1, 15, 16, 17, G - 1, G, G + 1, W * G - 1, W * G, W * G + 1, 2 * W * G + 5})
    try:
        _lib.call("ssw_tune_topk", 2)
        for n in counts:
            idx = make(gaussian_rows(n, seed=n), dtype)
            try:
                q = query(n, DIM)
                for tiles in (1, 3):  # rows an image: without and with a row-to-image map
                    n_images = n
                    if tiles != 1:
                        idx.set_row2image((np.arange(n, dtype=np.int64) // tiles).astype(np.int32))
                        n_images = (n + tiles - 1) // tiles
                    for ex in (None, np.arange(0, n_images, 7)):  # a seventh of the images excluded
                        avail = n_images - (0 if ex is None else ex.shape[0])
                        for k in (1, 10):
                            before = stats(idx)
                            full, got, st = both6(six, idx, lambda: idx.topk(q, k, excluded=ex))
                            same(full, got)
                            assert len(got[0]) == min(k, avail)
                            assert st[0] == 1 and st[3] == before[3] + 1, (n, tiles, k, st)  # on the current shadow
                            if avail >= k:
                                assert st[2] >= 0 and st[4] == before[4], (n, tiles, k, before, st)
            finally:
                idx.close()
    finally:
        _lib.call("ssw_tune_topk", 3)


# ---- 5. the pruned batch ----------------------------------------------------------------------------------------------
def unit_queries(seed, nq):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, DIM)).astype(np.float32)
    return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True))


def exclusions(nq, n_images, seed):
    """per query: None, an empty list, a few images, repeats"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(nq):
        kind = b % 4
        out.append(None if kind == 0 else [] if kind == 1 else rng.integers(0, n_images, 40).tolist() if kind == 2
                   else [3, 3, int(n_images - 1)])
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_equals_the_single_calls(six, dtype):
    from seesaw_amd.device_index import DeviceIndex
    n, k = 100_003, 10
    idx = DeviceIndex.synthetic(n, DIM, seed=21, dtype=dtype)
    try:
        for nq in (1, 5, 16, 17):  # 17 crosses a chunk
            Q = unit_queries(30 + nq, nq)
            ex = exclusions(nq, n, seed=nq)
            singles = [idx.topk(Q[b], k, excluded=ex[b]) for b in range(nq)]
            before = idx.prune_stats()
            got = idx.topk_batch(Q, k, ex, prune=True)
            now = idx.prune_stats()
            assert len(got) == nq
            for a, b in zip(singles, got):
                same(a, b)
            assert now["queries"] == before["queries"] + nq and now["fallbacks"] == before["fallbacks"], (before, now)
            assert now["last_survivors"] >= k
        st = idx.prune_stats()
        assert st["shadow"] == "current" and st["shadow_bytes"] == shadow_bytes(n), st  # one shadow serves both calls
    finally:
        idx.close()


def tiled_index(n, seed, dtype):
    """four tiles an image (the last image has n % 4), boxes and zoom levels for the second stage"""
    from seesaw_amd.device_index import DeviceIndex
    h = DeviceIndex.synthetic(n, DIM, seed=seed, dtype=dtype)
    h.set_row2image((np.arange(n, dtype=np.int64) // 4).astype(np.int32))
    boxes = np.array([[0, 0, 1, 1], [0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1]], np.float32)
    h.set_tile_meta(boxes[np.arange(n) % 4], np.array([0, 1, 1, 1], np.int32)[np.arange(n) % 4])
    return h


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_stage_batch_equals_the_unpruned_call(six, dtype):
    n, k, nq = 100_003, 10, 5
    idx = tiled_index(n, 22, dtype)
    try:
        Q = unit_queries(41, nq)
        ex = exclusions(nq, (n + 3) // 4, seed=9)
        want = unpruned(six, lambda: idx.topk_batch_avg(Q, k, "greater", excluded=ex))
        before = idx.prune_stats()
        got = idx.topk_batch_avg(Q, k, "greater", excluded=ex, prune=True)
        now = idx.prune_stats()
        for a, b in zip(want, got):
            same(a, b)
        assert now["queries"] == before["queries"] + nq and now["fallbacks"] == before["fallbacks"], (before, now)
        assert now["shadow"] == "current" and now["shadow_bytes"] == shadow_bytes(n)
    finally:
        idx.close()


# ---- 6. the chunk that never waits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_batch_block_equals_the_plain_call(six, dtype):
    import torch
    from seesaw_amd.device_index import DeviceIndex
    n, k, nq = 50_003, 10, 5
    dev = torch.device("cuda", 0)
    Q = unit_queries(90, nq)
    excluded = [None, [1, 2], None, [7], [3, 3, 900]]
    blocks = []
    for prune in (False, True):
        h = DeviceIndex.synthetic(n, DIM, seed=91, dtype=dtype)
        try:
            block = torch.full((8, 2 * 16 + 1), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()  # the handle works on its own stream
            h.set_exchange_target_batch(block.data_ptr(), 8, 16, True)
            h.topk_batch_dev(Q, k, excluded=excluded, prune=prune)
            h.sync()
            blocks.append(block.cpu().numpy())
            surv, why = h.prune_batch_dev_counts()
            st = h.prune_stats()
            if prune:
                assert surv.shape[0] == nq and not why.any(), (surv, why)
                assert np.all(surv >= k) and np.all(surv <= SURV_CAP)
                assert st["queries"] == nq and st["shadow"] == "current" and st["shadow_bytes"] == shadow_bytes(n), st
            else:
                assert surv.shape[0] == 0 and st["queries"] == 0 and st["shadow"] == "none", st
        finally:
            h.close()
    assert np.array_equal(blocks[0], blocks[1]) and (blocks[0][:nq, -1] == k).all()  # count k, no flag in the last word


# ---- 7. the fallbacks -------------------------------------------------------------------------------------------------
def test_more_survivors_than_the_cap(six):
    n = SURV_CAP + 4096
    rng = np.random.default_rng(2)
    row = rng.standard_normal(DIM).astype(np.float32) / np.float32(np.sqrt(DIM))
    X = np.tile(row, (n, 1))  # identical rows: every one reaches the threshold
    X[::1000] *= np.float32(1.5)
    idx = make(X, np.float32)
    try:
        q = query(1, DIM)
        full, got, st = both6(six, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and st[2] == -1 and st[3] == 1 and st[4] == 1, st
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_queries_that_cannot_be_bounded(six, dtype):
    """the zero query, and a NaN or inf query, which reaches the pre-scan only through the device entry (ssw_index_topk
    refuses it on the host): flagged, the full scan's bits, and `fallbacks` counts each"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    n = 100_000
    idx = DeviceIndex.synthetic(n, DIM, seed=4, dtype=dtype)
    try:
        before = stats(idx)
        z = np.zeros(DIM, np.float32)
        full, got, st = both6(six, idx, lambda: idx.topk(z, 10))
        same(full, got)
        assert st[3] == before[3] + 1 and st[4] == before[4] + 1 and st[2] == -1, (before, st)
        for v in (np.nan, np.inf, -np.inf):
            q = query(3, DIM)
            q[17] = v
            with pytest.raises(Exception, match="non-finite"):
                idx.topk(q, 10)
            assert hook_bounds6(idx, q, sums=False)["bad"]
            qd = torch.from_numpy(q).cuda()
            torch.cuda.synchronize()

            def dev_topk():
                idx.topk_dev(qd.data_ptr(), 10)
                return idx.topk_fetch(10)
            before = stats(idx)
            full, got, st = both6(six, idx, dev_topk)
            same(full, got)
            assert st[3] == before[3] + 1 and st[4] == before[4] + 1 and st[2] == -1, (v, before, st)
        # and a query that can be bounded is certified on the same handle
        before = stats(idx)
        q = query(5, DIM)
        full, got, st = both6(six, idx, lambda: idx.topk(q, 10))
        same(full, got)
        assert st[4] == before[4] and 10 <= st[2] <= SURV_CAP, (before, st)
    finally:
        idx.close()


@pytest.mark.parametrize("dim", [DIM, 256])
def test_the_6bit_shadow_refused_for_memory(lab_build, dim):
    """no shadow fits beside the reserve: the call is the full scan, nothing is built, and the refusal holds until the
    rows change, at the dim without an int8 shadow and at one that has it.  The first two words of the report are the
    product's own at this state: at dim 768 the 6-bit shadow's refusal on an eligible index, at dim 256 the untouched
    int8 shadow's "none", on an index of too few rows for it.  The three-launch top-k of small indexes is switched off
    (ssw_tune_topk(2)): it never reaches the pre-scan."""
    import ctypes
    from seesaw_amd import _lib
    n = 16 * 40 + 5  # more than one block of tiles, the last tile ragged
    X = np.random.default_rng(dim).standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    q = query(1, dim)
    refused = [3, 1] if dim == DIM else [0, 0]
    idx = make(X, np.float32)
    try:
        _lib.call("ssw_tune_topk", 2)
        full = unpruned(lab_build, lambda: idx.topk(q, 10))
        mode6(True, 1)
        mode(lab_build, True, reserve=1 << 60)
        same(full, idx.topk(q, 10))
        st = stats(idx)
        assert list(st[:2]) == refused and st[3] == 0 and st[5] == 0, st
        mode(lab_build, True)  # the reserve is the product's again, the refusal stands
        same(full, idx.topk(q, 10))
        st = stats(idx)
        assert list(st[:2]) == refused and st[3] == 0 and st[5] == 0, st
        _lib.call("ssw_index_upload", idx._h, ctypes.c_void_p(X.ctypes.data), 0, n)  # the same rows, changed
        same(full, idx.topk(q, 10))
        st = stats(idx)
        assert list(st[:2]) == [1, 1] and st[3] == 1 and st[5] == shadow_bytes(n, dim), st
    finally:
        mode6(True, -1)
        mode(lab_build, True)
        _lib.call("ssw_tune_topk", 3)
        idx.close()


# ---- 8. the product's thresholds, without the lab switches ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_product_threshold(lab_build, dtype):
    """an index of MIN_ROWS (6-bit single call, dim 768, f32; float16: f16) rows filled on the device is pruned on the 6-bit shadow, single
    query and batch (the batch's constants are the same), and answers with the full scan's keys; one row fewer is not
    eligible: its single query is the full scan and, with no int8 fallback, its pruned batch is the plain batch"""
    from seesaw_amd.device_index import DeviceIndex
    n = MIN_ROWS_768[dtype]
    assert n <= 1 << 24 and BATCH_MIN_ROWS_768[dtype] == n  # else: the upper case by ssw_index_prune_stats alone
    mode(lab_build, True)
    mode6(True, -1)
    batch6(-1)
    q, Q = query(300, DIM), unit_queries(50, 2)
    below = DeviceIndex.synthetic(n - 1, DIM, seed=7, dtype=dtype)
    try:
        assert not below.prune_stats()["eligible"]
        below.topk(q, 100)
        plain = below.topk_batch(Q, 10)
        pruned = below.topk_batch(Q, 10, prune=True)
        for a, b in zip(plain, pruned):
            same(a, b)
        st = below.prune_stats()
        assert st["shadow"] == "none" and st["shadow_bytes"] == 0 and st["queries"] == 0, st
    finally:
        below.close()
    idx = DeviceIndex.synthetic(n, DIM, seed=7, dtype=dtype)
    try:
        assert idx.prune_stats()["eligible"] and idx.prune_stats()["shadow"] == "none"
        full, got, st = both6(lab_build, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[0] == 1 and 100 <= st[2] <= SURV_CAP and st[3] == 1 and st[4] == 0, st
        assert st[5] == n * 584 == shadow_bytes(n), st
        assert idx.prune_stats()["shadow"] == "current" and idx.prune_stats()["shadow_bytes"] == n * 584
        print(f"dim 768, {np.dtype(dtype).name}, {n} rows: {st[2]} survivors")
        plain = idx.topk_batch(Q, 10)
        pruned = idx.topk_batch(Q, 10, prune=True)
        for a, b in zip(plain, pruned):
            same(a, b)
        after = idx.prune_stats()
        assert after["queries"] == 3 and after["fallbacks"] == 0 and after["shadow_bytes"] == n * 584, after
    finally:
        mode(lab_build, True)
        idx.close()


# ---- 9. the int8 side ------------------------------------------------------------------------------------------------
def test_the_int8_shadow_never_serves_dim_768(lab_build):
    """ssw_tune_prune's min_rows is the int8 shadow's: at one row, with the 6-bit defaults, a small dim-768 index stays
    unpruned; with the 6-bit path off nothing prunes it at any setting; the int8 hooks refuse it"""
    from seesaw_amd.device_index import DeviceIndex
    n = 3000
    idx = DeviceIndex.synthetic(n, DIM, seed=12)
    try:
        q = query(8, DIM)
        mode(lab_build, True, 1)
        mode6(True, -1)
        batch6(-1)
        assert not idx.prune_stats()["eligible"]
        mode6(False, 1)
        assert not idx.prune_stats()["eligible"]
        want = idx.topk(q, 10)
        st = idx.prune_stats()
        assert st["queries"] == 0 and st["shadow"] == "none" and st["shadow_bytes"] == 0, st
        with pytest.raises(Exception, match="not pruned"):
            hook_shadow(idx)
        with pytest.raises(Exception, match="not pruned"):
            hook_bounds(idx, q)
        # the 6-bit switches alone make it eligible, and the result is the same
        mode(lab_build, True)
        mode6(True, 1)
        assert idx.prune_stats()["eligible"]
        same(want, idx.topk(q, 10))
    finally:
        batch6(-1)
        mode6(True, -1)
        mode(lab_build, True)
        idx.close()
