"""GPU: the packed 6-bit shadow of single queries on an f16 index (csrc/prune.hip, k_q6_build_h16; DESIGN.md section 4,
"6-bit shadow"), on the lab build.  The shadow of an f16 index is built from the lane-interleaved binary16 rows;
everything here is compared with the widened rounding W = X.astype(float16).astype(float32) of the f32 rows X that went
into `DeviceIndex.from_numpy(X, dtype=np.float16)`:

  1. the shadow the device built equals the numpy twin `shadow6(W)` (codes and s6 bit for bit, a6 within the band of the
     f32 and int8 builder tests: its double sums are taken in the device's order), and only the 6-bit shadow exists;
  2. it equals the shadow of an f32 index of W: a swapped chunk or lane order in the wave's LDS line changes codes;
  3. every bounded row's lower bound contains the score of the f16 index's own full scan, within the width;
  4. pruned top-k = full top-k = the top-k of an f32 index of W, byte for byte, at the scan loop's ends;
  5. the handle's state, the fallbacks, a stale shadow and the first pruned batch;
  6. the product's constants leave an f16 index of 2^22 rows on the int8 shadow.

Rows: tests/_prune6_f16_helpers.py."""
import ctypes

import numpy as np
import pytest

from _prune6_f16_helpers import f16_rows
from _prune6_helpers import hook_bounds6, hook_shadow6, launch_shape6, mode6, quantise_query, shadow6, width6
from _prune_batch_helpers import edge_queries
from _prune_f16_helpers import unbounded_rows
from _prune_helpers import mode, query, same, stats

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
SURV_CAP = 1 << 18
F16 = np.float16


def f64(a):
    return np.asarray(a, dtype=np.float64)


def bytes6(n, dim):
    """device memory of the 6-bit shadow: whole 16-row tiles of 3 dim / 4 code bytes and two floats a row"""
    return (n + 15) // 16 * 16 * (dim * 3 // 4 + 8)


@pytest.fixture()
def six(lab_build):
    """every index takes the 6-bit path from one row on; the defaults again afterwards"""
    mode(lab_build, True)
    mode6(True, 1)
    try:
        yield lab_build
    finally:
        mode6(True, -1)
        mode(lab_build, True)


def shape(dim):
    """(G rows of one request of a wave, W waves of a full launch) of k_q6_bounds over an f16 index"""
    from seesaw_amd.device_index import DeviceIndex
    probe = DeviceIndex(1 << 20, dim, dtype=F16)
    try:
        blocks, tiles = launch_shape6(probe)
    finally:
        probe.close()
    return 16 * tiles, 4 * blocks


def f16_index(X, row2image=None):
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex.from_numpy(X, row2image=row2image, dtype=F16)


@pytest.mark.parametrize("n,dim", [((1 << 16) + 1, 256), (100_003, 512), ((1 << 16) + 1, 1024),
                                   (1, 512), (15, 512), (16, 512), (17, 512)])
def test_shadow_equals_the_twin_on_the_widened_rows(six, n, dim):
    """1.  A single row is either bounded or not: n = 1 runs with an unbounded first row and with a bounded one."""
    unbounded = 0
    for lead in ((0, 1) if n == 1 else (0,)):
        X, W = f16_rows(n, dim, lead=lead)
        idx = f16_index(X)
        try:
            c, s, a = hook_shadow6(idx)
            tc, ts, ta = shadow6(W)
            assert np.array_equal(c, tc), (lead, np.argwhere(c != tc)[:4])
            assert np.array_equal(s.view(np.uint32), ts.view(np.uint32)), lead
            unb = unbounded_rows(W)
            assert np.array_equal(np.isinf(ta), unb)  # the twin agrees with the statement on the rows themselves
            assert not np.isnan(a).any() and np.array_equal(np.isinf(a), unb), (lead, np.nonzero(np.isinf(a) != unb)[0][:8])
            unbounded += int(unb.sum())
            fin = ~unb
            assert np.all(np.abs(f64(a[fin]) - f64(ta[fin])) <= 2.0 ** -20 * f64(ta[fin])), (dim, n, lead)
            st = stats(idx)
            assert st[0] == 1 and st[5] == bytes6(n, dim), st  # the 6-bit shadow only, no int8 shadow
        finally:
            idx.close()
    assert unbounded >= 1


@pytest.mark.parametrize("n,dim", [(50_003, 512), (17, 256), (17, 512), (17, 1024)])
def test_same_shadow_as_an_f32_index_of_the_widened_rows(six, n, dim):
    """2. codes and s6 bits of the f16 index's shadow equal those k_q6_build gives on an f32 index of W"""
    from seesaw_amd.device_index import DeviceIndex
    X, W = f16_rows(n, dim)
    half, wide = f16_index(X), DeviceIndex.from_numpy(W)
    try:
        assert np.array_equal(half.download().view(np.uint32), W.view(np.uint32))  # the index holds W
        ch, sh, ah = hook_shadow6(half)
        cw, sw, aw = hook_shadow6(wide)
        assert np.array_equal(ch, cw), np.argwhere(ch != cw)[:4]
        assert ch.any() and np.array_equal(sh.view(np.uint32), sw.view(np.uint32))
        assert np.array_equal(np.isinf(ah), np.isinf(aw))
    finally:
        half.close()
        wide.close()


@pytest.mark.parametrize("dim", DIMS)
def test_certificate_row_by_row(six, dim):
    """3. the queries, the width and the slack of tests/test_prune6_gpu.py, test_certificate_row_by_row"""
    G, Wv = shape(dim)
    rng = np.random.default_rng(11)
    Q = edge_queries(rng, dim) + [query(40 + i, dim) * np.float32(2.0 ** (7 * i - 10)) for i in range(4)]
    for n in (17, G - 1, Wv * G + 1, 100_003):
        X, W = f16_rows(n, dim)
        idx = f16_index(X)
        try:
            mode(six, False)
            S = [idx.scores(q) for q in Q]  # the f16 index's own full scan
            mode(six, True)
            _, s, a = hook_shadow6(idx, codes=False)
            fin = np.isfinite(a)
            assert np.array_equal(~fin, unbounded_rows(W)) and fin.any() and not fin.all(), (dim, n)
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


def three(lib, idx, ref, fn):
    """fn(index) on the f16 index with pruning off, then on the 6-bit path, then on the f32 index of the widened rows with
    pruning off: (full, pruned, f32, the f16 index's stats after its pruned call)"""
    mode(lib, False)
    full = fn(idx)
    mode(lib, True)
    got = fn(idx)
    st = stats(idx)
    mode(lib, False)
    wide = fn(ref)
    mode(lib, True)
    return full, got, wide, st


@pytest.mark.parametrize("dim", DIMS)
def test_loop_ends_pruned_equals_full_equals_f32(six, dim):
    """4. with the three-launch top-k of small indexes switched off (ssw_tune_topk(2)): it never prunes"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    G, Wv = shape(dim)
    counts = sorted({1, 15, 16, 17, G - 1, G + 1, Wv * G - 1, Wv * G + 1, 2 * Wv * G + 5})
    really_pruned = 0
    try:
        _lib.call("ssw_tune_topk", 2)
        for n in counts:
            X, W = f16_rows(n, dim, lead=1)  # an index of one row holds a bounded row
            idx, ref = f16_index(X), DeviceIndex.from_numpy(W)
            try:
                q = query(n, dim)
                for calls, k in enumerate((1, 100), 1):
                    full, got, wide, st = three(six, idx, ref, lambda i: i.topk(q, k))
                    same(full, got)
                    same(wide, got)
                    assert st[0] == 1 and st[3] == calls, (dim, n, k, st)  # the shadow is current, the call was pruned
                    really_pruned += int(st[2] >= 0)
                if n >= 3:  # multi-row images, a seventh of them excluded
                    r2i = (np.arange(n, dtype=np.int64) // 3).astype(np.int32)
                    idx.set_row2image(r2i)
                    ref.set_row2image(r2i)
                    ex = np.arange(0, (n + 2) // 3, 7)
                    for calls, k in enumerate((1, 100), 3):
                        full, got, wide, st = three(six, idx, ref, lambda i: i.topk(q, k, excluded=ex))
                        same(full, got)
                        same(wide, got)
                        assert st[0] == 1 and st[3] == calls, (dim, n, k, st)
                        really_pruned += int(st[2] >= 0)
            finally:
                idx.close()
                ref.close()
    finally:
        _lib.call("ssw_tune_topk", 3)
    assert really_pruned > 0  # not every call fell back to the full scan


def test_state_and_fallbacks(six):
    """5. after a pruned call on an f16 index: survivors within the cap, no fallback, only the 6-bit shadow's bytes; every
    reader of the score buffer sees the full scan's bits; the zero query falls back; an upload makes the shadow stale and
    the next call rebuilds it; the first pruned batch adds the int8 shadow"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    dim, n = 512, 200_000
    idx = DeviceIndex.synthetic(n, dim, seed=9, dtype=F16)
    try:
        q = query(2, dim)
        mode(six, False)
        want_scores, want_top, want_50 = idx.scores(q), idx.topk(q, 100), idx.topk(None, 50)
        mode(six, True)
        same(idx.topk(q, 100), want_top)
        st = stats(idx)
        assert st[0] == 1 and 100 <= st[2] <= SURV_CAP and st[4] == 0, st
        assert st[5] == bytes6(n, dim)  # 6-bit bytes and no int8 shadow
        ps = idx.prune_stats()
        assert ps["shadow"] == "current" and ps["eligible"] and ps["fallbacks"] == 0, ps
        assert 100 <= ps["last_survivors"] <= SURV_CAP and ps["shadow_bytes"] == bytes6(n, dim), ps
        # the buffer after a pruned call: every reader sees the full scan's
        same(idx.topk(None, 50), want_50)
        idx.topk(q, 100)
        got_scores = idx.gather_scores(np.arange(n, dtype=np.int64))
        assert np.array_equal(got_scores.view(np.uint32), want_scores.view(np.uint32))
        # the zero query cannot be bounded: the full scan, counted as a fallback
        z = np.zeros(dim, np.float32)
        mode(six, False)
        full = idx.topk(z, 10)
        mode(six, True)
        before = stats(idx)[4]
        same(idx.topk(z, 10), full)
        assert stats(idx)[4] == before + 1
        # rows uploaded as from_numpy uploads a chunk of f32 rows: the shadow goes stale, the next call rebuilds it
        first = 100_000 - 3  # across a tile boundary
        block = np.repeat((q * np.float32(3.0))[None, :], 7, axis=0)
        assert stats(idx)[0] == 1
        _lib.call("ssw_index_upload", idx._h, block.ctypes.data_as(ctypes.c_void_p), first, block.shape[0])
        assert stats(idx)[0] == 2 and idx.prune_stats()["shadow"] == "stale"
        mode(six, False)
        full = idx.topk(q, 100)
        mode(six, True)
        got = idx.topk(q, 100)
        same(full, got)
        st = stats(idx)
        assert got[2][0] == first and st[0] == 1 and st[2] >= 100 and st[5] == bytes6(n, dim), st
        c, _, _ = hook_shadow6(idx, first - 1, 9)
        assert np.array_equal(c[1], c[7]) and not np.array_equal(c[0], c[1]) and not np.array_equal(c[8], c[1])
        # the first pruned batch builds the int8 shadow; its results equal the plain batch's
        mode(six, True, 1)
        Q = np.stack([query(20 + i, dim) for i in range(4)])
        plain = idx.topk_batch(Q, 20)
        pruned = idx.topk_batch(Q, 20, prune=True)
        for a, b in zip(plain, pruned):
            same(a, b)
        assert stats(idx)[5] == bytes6(n, dim) + n * (dim + 8)
    finally:
        idx.close()


def test_default_constants_leave_small_indexes_alone(lab_build):
    """6. the product's constants: single queries on an f16 index of 2^22 rows scan the int8 shadow"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim = 1 << 22, 512
    mode(lab_build, True)
    mode6(True, -1)
    idx = DeviceIndex.synthetic(n, dim, seed=7, dtype=F16)
    try:
        idx.topk(query(300), 100)
        st = stats(idx)
        assert st[0] == 1 and st[3] == 1 and st[5] == n * (dim + 8), st
        assert idx.prune_stats()["shadow_bytes"] == n * (dim + 8)
    finally:
        mode(lab_build, True)
        idx.close()
