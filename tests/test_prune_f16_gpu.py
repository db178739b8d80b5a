"""GPU: the certified int8 pre-scan (csrc/prune.hip) on an f16 index.  The shadow of an f16 index
is built by k_q8_build_h16 from the lane-interleaved binary16 rows; everything here is compared with the widened
rounding W = round_vectors(X, np.float16) of the f32 rows X that went into `DeviceIndex.from_numpy(X, dtype=np.float16)`:

  1. eligibility: an f16 index is pruned once it has the threshold's rows, and DeviceIndex.prune_stats() says so;
  2. the shadow the device built equals the numpy twin `shadow(W)` row by row (codes and s_r bit for bit, a_r within the
     limits of tests/test_prune_certificate_gpu.py: the double sums are taken in another order than the f32 builder's);
  3. every row's lower bound contains the score of the f16 index's own full scan;
  4. pruned top-k = full top-k = the top-k of an f32 index of W, byte for byte;
  5. every reader of the score buffer sees the full scan afterwards, both uploads make the shadow stale;
  6. a session-level query.

Rows: Gaussian rows with the 56 binary16-specific rows of tests/_prune_f16_helpers.py over the first rows, across a
k_q8_bounds group boundary (4096 is one at every dim) and, reversed, over the last rows.  Shapes: dims 256 / 512 / 1024
(the f16 layout differs per dim), 2^16 + 1 and 100 003 rows (above the 65 536-row latency variant of the scan, no
multiple of a group or a wave), and once 2^22 + 5 rows: launch_q8_build caps its grid at 2^20 blocks of 4 rows, so
only past 2^22 rows does a wave take a second row."""
import ctypes
import functools

import numpy as np
import pytest

from _prune_f16_helpers import N_ROWS, N_UNBOUNDED, f16_adversarial_rows, unbounded_rows
from _prune_helpers import SAFETY, both, gamma, hook_bounds, hook_shadow, mode, queries, same, shadow, stats

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
ROWS = ((1 << 16) + 1, 100003)
CHUNK = 1 << 14


def f64(a):
    return np.asarray(a, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def gaussian(dim):
    """100 003 Gaussian rows of norm about 1, generated once per dim and never written to (dropped after the module)"""
    return np.random.default_rng(dim).standard_normal((ROWS[-1], dim), dtype=np.float32) / np.float32(np.sqrt(dim))


@pytest.fixture(scope="module", autouse=True)
def _drop_rows():
    yield
    gaussian.cache_clear()


def widen(X):
    from seesaw_amd.device_index import round_vectors
    with np.errstate(over="ignore"):
        return round_vectors(X, np.float16)


def adversarial_case(dim, n):
    """(X f32 [n, dim], W = its widened rounding, ((position, block), ...))"""
    X = gaussian(dim)[:n].copy()
    A = f16_adversarial_rows(np.random.default_rng(0), dim)
    blocks = ((0, A), (4076, A), (n - N_ROWS, np.ascontiguousarray(A[::-1])))
    for p, B in blocks:
        X[p:p + N_ROWS] = B
    return X, widen(X), blocks


def f16_index(X, row2image=None):
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex.from_numpy(X, row2image=row2image, dtype=np.float16)


def check_shadow(W, c, s, a, dim, where):
    """the device's shadow (c, s, a) of the widened rows W against the numpy twin and the float64 statement of a_r"""
    tc, ts, _ = shadow(W)
    assert int(c.min()) >= -127, where
    assert np.array_equal(s.view(np.uint32), ts.view(np.uint32)), (where, np.nonzero(s != ts)[0][:8])
    assert np.array_equal(c, tc), (where, np.nonzero((c != tc).any(axis=1))[0][:8])
    unb = unbounded_rows(W)
    assert not np.isnan(a).any()
    assert np.array_equal(np.isinf(a), unb), (where, np.nonzero(np.isinf(a) != unb)[0][:8])
    assert np.all(a[unb] == np.inf) and np.all(s[unb] == 0) and not c[unb].any()
    ok = ~unb
    Wd, cd, sd = f64(W[ok]), f64(c[ok]), f64(s[ok])
    e = Wd - sd[:, None] * cd
    a_star = np.sqrt((e * e).sum(1)) + gamma(dim) * (np.sqrt((Wd * Wd).sum(1)) + sd * np.sqrt((cd * cd).sum(1)))
    a_ok = f64(a[ok])
    low = SAFETY * a_star * (1 - 2.0 ** -40)  # the factor is there and the rounding to f32 goes up
    assert np.all(low <= a_ok), (where, float((low / np.maximum(a_ok, 1e-300)).max()))
    lim = a_star * (1 + 2.0 ** -9) + f64(np.spacing(a[ok]))
    assert np.all(a_ok <= lim), (where, float((a_ok / np.maximum(a_star, 1e-300)).max()))
    return int(unb.sum())


def test_an_f16_index_is_pruned(lab_build):
    """1. with the threshold lowered an f16 index is eligible, a top-k with a query builds the shadow and counts as a
    pruned call, and DeviceIndex.prune_stats() reports what ssw_index_prune_stats does; min_rows < 0 restores a
    threshold far above these 65 537 rows"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim = ROWS[0], 512
    idx = DeviceIndex.synthetic(n, dim, seed=5, dtype=np.float16)
    try:
        mode(lab_build, True, min_rows=1)
        st = stats(idx)
        assert st[1] == 1 and st[0] == 0, st
        assert idx.prune_stats() == {"shadow": "none", "eligible": True, "last_survivors": 0, "queries": 0,
                                     "fallbacks": 0, "shadow_bytes": 0}
        q = np.random.default_rng(3).standard_normal(dim).astype(np.float32)
        got = idx.topk(q, 100)
        st2 = stats(idx)
        assert st2[3] == st[3] + 1 and st2[0] == 1, st2
        assert st2[2] >= 100 and st2[4] == 0, st2
        assert idx.prune_stats() == {"shadow": "current", "eligible": True, "last_survivors": int(st2[2]), "queries": 1,
                                     "fallbacks": 0, "shadow_bytes": n * (dim + 8)}
        mode(lab_build, False)
        same(idx.topk(q, 100), got)
        assert idx.prune_stats()["eligible"] is False and stats(idx)[3] == st2[3]
        mode(lab_build, True, min_rows=-1)
        assert stats(idx)[1] == 0
    finally:
        mode(lab_build, True)
        idx.close()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_shadow_row_by_row(lab_build, dim, n):
    """2. the index holds W (download), and the shadow of every row is the twin's: check_shadow"""
    X, W, blocks = adversarial_case(dim, n)
    idx = f16_index(X)
    try:
        mode(lab_build, True, min_rows=1)
        seen = 0
        for r0 in range(0, n, CHUNK):
            m = min(CHUNK, n - r0)
            got = idx.download(r0, m)
            assert np.array_equal(got.view(np.uint32), W[r0:r0 + m].view(np.uint32)), r0
            c, s, a = hook_shadow(idx, r0, m)
            seen += check_shadow(W[r0:r0 + m], c, s, a, dim, (dim, n, r0))
        assert seen == N_UNBOUNDED * len(blocks)
        for p, B in blocks:  # the binary16-specific rows by name: bounded subnormal row, zero rows, the pinned step
            _, s, a = hook_shadow(idx, p, N_ROWS, codes=False)
            at = (lambda i: N_ROWS - 1 - i) if p == n - N_ROWS else (lambda i: i)  # the last block is reversed
            assert np.isinf(a[at(50)]) and np.isfinite(a[at(49)]) and s[at(49)] == np.float32(65504) / np.float32(127)
            assert np.isfinite(a[at(52)]) and s[at(52)] > 0
            assert s[at(53)] == 0 and a[at(53)] == 0 and s[at(24)] == 0 and a[at(24)] == 0
            assert s[at(55)] == np.float32(2.0 ** -7)
    finally:
        mode(lab_build, True)
        idx.close()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_every_row_is_contained(lab_build, dim, n):
    """3. for every query of queries() and every row with finite a_r: lb_r < S_r and
    S_r - lb_r <= 2 a_r Q (1 + 2^-19) + |lb_r| 2^-19 + 2^-98, S = the f16 index's own full scan.  The zero query and a
    query of norm above 2^40 report "cannot be bounded"; so does, through the top-k, a non-finite device query"""
    X, W, blocks = adversarial_case(dim, n)
    idx = f16_index(X)
    try:
        mode(lab_build, True, min_rows=1)
        _, _, a = hook_shadow(idx, codes=False)
        fin = np.isfinite(a)
        assert int((~fin).sum()) == N_UNBOUNDED * len(blocks)
        rng = np.random.default_rng(1)
        for i, q in enumerate(queries(rng, W)):
            mode(lab_build, False)
            S = idx.scores(q)
            mode(lab_build, True, min_rows=1)
            lb, Q, bad = hook_bounds(idx, q)
            same([S], [idx.scores(q)])  # the buffer of bounds is completed for its readers
            norm = float(np.sqrt(np.sum(f64(q) ** 2)))
            assert norm <= float(Q) <= norm * (1 + 2.0 ** -20), (i, norm, float(Q))
            assert bad == (1 if norm == 0 else 0), (i, bad)
            Sd, lbd, ad = f64(S[fin]), f64(lb[fin]), f64(a[fin])
            assert np.all(np.isfinite(Sd)) and np.all(np.isfinite(lbd)), i
            assert np.all(lbd < Sd), (i, np.nonzero(fin)[0][~(lbd < Sd)][:8])
            slack = 2 * ad * float(Q) * (1 + 2.0 ** -19) + np.abs(lbd) * 2.0 ** -19 + 2.0 ** -98
            wide = ~(Sd - lbd <= slack)
            assert not wide.any(), (i, np.nonzero(fin)[0][wide][:8], float(((Sd - lbd) / slack).max()))
            if norm == 0:
                assert np.all(np.isnan(lb[~fin])), i
            else:
                assert np.all(lb[~fin] == -np.inf), i
        big = (rng.standard_normal(dim) * 2.0 ** 41).astype(np.float32)
        assert hook_bounds(idx, big)[2] == 1
        # a non-finite query never passes the host entries; on the device it is refused by k_q8_query: the call falls back
        import torch
        for v in (np.inf, np.nan):
            q = rng.standard_normal(dim).astype(np.float32)
            q[dim // 2] = v
            qd = torch.from_numpy(q).cuda()
            torch.cuda.synchronize()
            mode(lab_build, False)
            idx.topk_dev(qd.data_ptr(), 10)
            full = idx.topk_fetch(10)
            mode(lab_build, True, min_rows=1)
            before = stats(idx)
            idx.topk_dev(qd.data_ptr(), 10)
            got = idx.topk_fetch(10)
            st = stats(idx)
            same(full, got)
            assert st[3] == before[3] + 1 and st[4] == before[4] + 1 and st[2] == -1, (v, st)
    finally:
        mode(lab_build, True)
        idx.close()


def variants(n):
    """(row2image or None, name): single-row images, and 4 rows an image"""
    return ((None, "rows"), ((np.arange(n, dtype=np.int64) // 4).astype(np.int32), "4 rows an image"))


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_pruned_topk_is_the_full_topk_on_gaussian_rows(lab_build, dim, n):
    """4. Gaussian rows: every call is really pruned (survivors >= k, no fallback: the cap of 2^18 survivors cannot
    trigger below 2^18 rows and these rows have no mass ties), and returns the bytes of the full scan and of an f32
    index of the widened rows"""
    from seesaw_amd.device_index import DeviceIndex
    X = gaussian(dim)[:n]
    idx, ref = f16_index(X), DeviceIndex.from_numpy(widen(X))
    try:
        rng = np.random.default_rng(7)
        for r2i, name in variants(n):
            idx.set_row2image(r2i)
            ref.set_row2image(r2i)
            for j in range(2):
                q = rng.standard_normal(dim).astype(np.float32)
                mode(lab_build, False)
                ex = idx.topk(q, 40)[0][::2]
                for excluded in (None, ex):
                    for k in (1, 100):
                        fallbacks = stats(idx)[4]
                        full, got, st = both(lab_build, idx, lambda: idx.topk(q, k, excluded=excluded), min_rows=1)
                        msg = (name, j, excluded is not None, k, st)
                        same(full, got)
                        assert len(got[0]) == k, msg
                        assert st[0] == 1 and st[2] >= k and st[4] == fallbacks, msg
                        mode(lab_build, False)
                        same(ref.topk(q, k, excluded=excluded), got)
    finally:
        mode(lab_build, True)
        idx.close()
        ref.close()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_pruned_topk_is_the_full_topk_on_adversarial_rows(lab_build, dim, n):
    """4. the binary16-specific rows in the index, every query of queries(): a call may fall back (the zero query does),
    the bytes are those of the full scan and of the f32 index of the widened rows all the same"""
    from seesaw_amd.device_index import DeviceIndex
    X, W, blocks = adversarial_case(dim, n)
    idx, ref = f16_index(X), DeviceIndex.from_numpy(W)
    try:
        adv_rows = np.concatenate([np.arange(p, p + N_ROWS) for p, _ in blocks])
        pruned = 0
        for r2i, name in variants(n):
            idx.set_row2image(r2i)
            ref.set_row2image(r2i)
            adv_images = adv_rows if r2i is None else np.unique(r2i[adv_rows])
            for i, q in enumerate(queries(np.random.default_rng(1), W)):
                for excluded in (None, adv_images):
                    for k in (1, 100):
                        full, got, st = both(lab_build, idx, lambda: idx.topk(q, k, excluded=excluded), min_rows=1)
                        msg = (name, i, excluded is not None, k, st)
                        same(full, got)
                        assert len(got[0]) == k and st[0] == 1, msg
                        assert st[2] == -1 or st[2] >= k, msg
                        pruned += int(st[2] >= k)
                        mode(lab_build, False)
                        same(ref.topk(q, k, excluded=excluded), got)
        assert pruned > 0  # not every call fell back: the case is not vacuous
    finally:
        mode(lab_build, True)
        idx.close()
        ref.close()


def test_state_after_a_pruned_topk(lab_build):
    """5. after a pruned top-k on an f16 index gather_scores, scores(q) and rescore_avg return the full scan's bits;
    ssw_index_upload and ssw_index_upload_f16 make the shadow stale and the next top-k sees the new rows; topk_batch
    with two queries and a call with the pruning off leave the counters alone; device_ptrs ends the eligibility"""
    from seesaw_amd import _lib
    n, dim = ROWS[0], 512
    r2i = (np.arange(n, dtype=np.int64) // 4).astype(np.int32)
    idx = f16_index(gaussian(dim)[:n], row2image=r2i)
    try:
        boxes = np.tile(np.array([[0, 0, 1, 1], [0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1]], np.float32), (n // 4 + 1, 1))
        idx.set_tile_meta(boxes[:n], np.tile(np.array([0, 1, 1, 1], np.int32), n // 4 + 1)[:n])
        rng = np.random.default_rng(11)
        q = rng.standard_normal(dim).astype(np.float32)
        q /= np.linalg.norm(q)
        rows = rng.choice(n, 3000, replace=False)
        pos = rng.choice(idx.n_images, 200, replace=False)
        mode(lab_build, False)
        ref_scores = idx.scores(q)
        ref_top = idx.topk(q, 64)
        ref_avg = idx.rescore_avg(pos, "greater")
        mode(lab_build, True, min_rows=1)

        def pruned_topk():
            before = stats(idx)
            same(ref_top, idx.topk(q, 64))
            st = stats(idx)
            assert st[3] == before[3] + 1 and st[2] >= 64 and st[4] == before[4], st

        pruned_topk()
        same(ref_top, idx.topk(None, 64))
        pruned_topk()
        same([ref_scores[rows]], [idx.gather_scores(rows)])
        pruned_topk()
        same([ref_scores], [idx.scores(q)])
        pruned_topk()
        same(ref_avg, idx.rescore_avg(pos, "greater"))
        # a batch of two never touches the shadow or the counters
        pruned_topk()
        before = stats(idx)
        q2 = rng.standard_normal(dim).astype(np.float32)
        pair = idx.topk_batch(np.stack([q2, q]), 64)
        same(ref_top, pair[1])
        assert np.array_equal(stats(idx), before)
        # both upload entries: f32 rows (rounded on the device), binary16 rows
        hit32 = np.repeat((q * 3.0).astype(np.float32)[None, :], 3, axis=0)
        hit16 = np.repeat((q * 5.0).astype(np.float16)[None, :], 3, axis=0)
        for entry, block, first in (("ssw_index_upload", hit32, 1001), ("ssw_index_upload_f16", hit16, n - 3)):
            assert stats(idx)[0] == 1
            _lib.call(entry, idx._h, block.ctypes.data_as(ctypes.c_void_p), first, block.shape[0])
            assert stats(idx)[0] == 2, entry
            full, got, st = both(lab_build, idx, lambda: idx.topk(q, 64), min_rows=1)
            same(full, got)
            assert got[0][0] == r2i[first] and got[2][0] == first and st[0] == 1 and st[2] >= 64, (entry, st)
            mode(lab_build, True, min_rows=1)
        # with the pruning off nothing is pruned
        before = stats(idx)
        mode(lab_build, False)
        idx.topk(q, 64)
        after = stats(idx)
        assert after[1] == 0 and after[3] == before[3]
        mode(lab_build, True, min_rows=1)
        assert stats(idx)[1] == 1
        idx.device_ptrs()
        assert stats(idx)[1] == 0 and stats(idx)[0] == 0
    finally:
        mode(lab_build, True)
        idx.close()


def test_past_the_build_grid(lab_build):
    """2, 4. at 2^22 + 5 rows (dim 256, filled on the device) the waves of the first blocks build a second row: the
    first 8 rows, 8 rows around row 2^22 and the last 8 against the twin of the downloaded rows; then one pruned top-k"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim = (1 << 22) + 5, 256
    idx = DeviceIndex.synthetic(n, dim, seed=9, dtype=np.float16)
    try:
        mode(lab_build, True, min_rows=1)
        for r0 in (0, (1 << 22) - 4, n - 8):
            W = idx.download(r0, 8)
            assert np.array_equal(W, widen(W))
            c, s, a = hook_shadow(idx, r0, 8)
            assert check_shadow(W, c, s, a, dim, r0) == 0 and np.all(s > 0)
        q = np.random.default_rng(100).standard_normal(dim).astype(np.float32)
        q = (q / np.linalg.norm(q)).astype(np.float32)
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100), min_rows=1)
        same(full, got)
        assert len(got[0]) == 100
        assert st[0] == 1 and 100 <= st[2] < (1 << 18) and st[4] == 0, st
    finally:
        mode(lab_build, True)
        idx.close()


def test_vector_index_query(lab_build):
    """6. a VectorIndex with vector_dtype="float16": query() returns what it returns with the pruning off, and is pruned"""
    from seesaw_amd.vector_index import VectorIndex
    vi = VectorIndex(vectors=gaussian(512)[:ROWS[0]], vector_dtype="float16")
    try:
        q = np.random.default_rng(21).standard_normal(512).astype(np.float32)
        mode(lab_build, False)
        full = vi.query(q, 100)
        mode(lab_build, True, min_rows=1)
        got = vi.query(q, 100)
        same(full, got)
        st = stats(vi._dev)
        assert st[3] == 1 and st[2] >= 100 and st[4] == 0, st
    finally:
        mode(lab_build, True)
        vi._dev.close()
