"""GPU: the certificate of the int8 pre-scan (csrc/prune.hip) checked row by row on what the
device wrote.  tests/test_prune_gpu.py compares only the final top-k, where ~400 survivors for k = 100 hide almost any
error in the bounds; here the lab build's hooks (ssw_debug_prune_shadow / _bounds / _survivors: the product's kernels
through the product's launch functions) return the shadow, every row's lower bound, Q and the survivor list, and each is
compared with a float64 / numpy statement of what DESIGN.md claims:

  a. the shadow equals the numpy twin of k_q8_build bit for bit, and a_r is valid and no wider than its formula;
  b. the f32 scan equals oracle.scores_kernel_order bit for bit on the adversarial rows (subnormals, non-finite);
  c. lb_r < S_r and S_r - lb_r within the doubled slack of the ub formula, for every row; Q brackets ||q||;
  d. k_survivors keeps every row that must be kept, no row that is proven below the threshold, and never a cut list;
  e. pruned and full top-k agree at dim 256 / 1024, ragged row counts, multi-row images, exclusions, edge queries.

Every index is synthetic rows generated on the device with the 49 adversarial rows of tests/_prune_helpers.py uploaded
over its first rows, its last rows (in reverse order; the clamped tail loads of k_q8_bounds cover them) and rows that
straddle a group boundary (8, 16 or 32 rows a group at dim 1024 / 512 / 256).  The row counts are no multiple of a group nor of a wave:
2^18 + 37, the prime 100 003, and 2^16 + 1 = one row past a group boundary at every dim."""
import ctypes

import numpy as np
import pytest

from _prune_helpers import (SAFETY, adversarial_rows, both, gamma, hook_bounds, hook_shadow, hook_survivors, mode, queries,
                            same, shadow)

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
ROWS = ((1 << 18) + 37, 100003, (1 << 16) + 1)
MIN_ROWS = 1 << 15  # the pruning threshold of these cases (the product's is 2^22)
SURV_CAP = 1 << 18
CHUNK = 1 << 14


def f64(a):
    return np.asarray(a, dtype=np.float64)


def make_index(dim, n, seed=1):
    """(index, adversarial rows [49, dim], ((position, block), ...)): synthetic rows with the adversarial rows over the
    first rows, over rows across the group boundaries 4080 ... 4120 (4096 is one at every dim) and, in reverse order,
    over the last rows, so that the index ends in bounded rows with different codes.  The caller closes the index."""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(n, dim, seed=seed)
    A = adversarial_rows(np.random.default_rng(0), dim)
    blocks = ((0, A), (4076, A), (n - A.shape[0], np.ascontiguousarray(A[::-1])))
    for p, B in blocks:
        _lib.call("ssw_index_upload", idx._h, B.ctypes.data_as(ctypes.c_void_p), int(p), B.shape[0])
    return idx, A, blocks


def edge_queries(A):
    """the helper's six (random, ones, a multiple of a row, zero, one component 1e6, norm ~1e-30) and a finite query of
    norm above 2^40: (name, q, bounded).  k_q8_query refuses to bound the last one and the zero query."""
    rng = np.random.default_rng(1)
    dim = A.shape[1]
    names = ("random", "ones", "row multiple", "zero", "one component 1e6", "norm 1e-30")
    out = [(nm, q, nm != "zero") for nm, q in zip(names, queries(rng, A))]  # Q = 0 counts as not bounded
    out.append(("norm above 2^40", (rng.standard_normal(dim) * 2.0 ** 41).astype(np.float32), False))
    return out


def ub_doubled(lb, a, Q):
    """DESIGN.md's ub formula with each slack term doubled, in float64 (NaN where a = +inf)"""
    lb, a = f64(lb), f64(a)
    with np.errstate(invalid="ignore", over="ignore"):
        return lb + 2 * a * float(Q) * (1 + 2.0 ** -19) + np.abs(lb) * 2.0 ** -19 + 2.0 ** -98


def unbounded_rows(X):
    """rows k_q8_build must refuse, from the rows themselves: a non-finite element or max|x| outside [2^-60, 2^60]"""
    fin = np.all(np.isfinite(X), axis=1)
    m = np.max(np.abs(np.where(np.isfinite(X), X, 0)), axis=1)
    return ~fin | ((m > 0) & ((m < np.float32(2.0 ** -60)) | (m > np.float32(2.0 ** 60))))


def key_order_topk(S, r2i, excluded, k):
    """what the selection does with a score vector that may hold NaN (select): an image's value is
    the maximum over its rows by `s > best` from -inf, so a NaN row never wins and the lowest row attaining the maximum
    is the best row; images order by the composite key (ord(value) << 32) | ~image, in which a NaN with the sign bit clear
    lies above +inf and one with the sign bit set below -inf.  -> (images, score bits, best rows) of the k largest keys"""
    S = np.asarray(S, dtype=np.float32)
    if r2i is None:
        val, best = S, np.arange(S.shape[0], dtype=np.int64)
    else:
        start = np.concatenate(([0], np.nonzero(np.diff(r2i))[0] + 1)).astype(np.int64)
        clean = np.where(np.isnan(S), -np.inf, S).astype(np.float32)
        val = np.maximum.reduceat(clean, start)
        hit = np.nonzero(clean == val[r2i])[0]  # rows attaining their image's maximum, ascending
        first = np.unique(r2i[hit], return_index=True)[1]
        best = hit[first].astype(np.int64)
        assert best.shape == val.shape
    u = val.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    img = np.arange(val.shape[0], dtype=np.uint64)
    key = (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - img)
    keep = np.ones(val.shape[0], dtype=bool)
    if excluded is not None and len(excluded):
        keep[np.asarray(excluded, dtype=np.int64)] = False
    cand = np.nonzero(keep)[0]
    top = cand[np.argsort(key[cand])[::-1][:k]]
    return top.astype(np.int64), val[top].view(np.uint32), best[top]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_shadow_the_device_built(lab_build, dim, n):
    """a. every row: |c| <= 127; s and the codes are the numpy twin's bits (both divide and round in IEEE f32); the rows
    that cannot be bounded, and no others, have c = 0, s = 0, a = +inf; for the rest a_r >= a* = ||x - s c|| +
    gamma (||x|| + s ||c||) evaluated in float64 from the device's c and s without the safety factor, and
    a_r <= a* (1 + 2^-9) + one f32 ulp (the kernel's factor is 1 + 2^-10; the doubled margin is for the float64
    summation order); and a_r >= (1 + 2^-10) a* (1 - 2^-40): the factor is there and the rounding to f32 goes up"""
    idx, A, pos = make_index(dim, n)
    try:
        mode(lab_build, True, MIN_ROWS)
        g = gamma(dim)
        seen_unbounded = 0
        for r0 in range(0, n, CHUNK):
            m = min(CHUNK, n - r0)
            X = idx.download(r0, m)
            c, s, a = hook_shadow(idx, r0, m)
            tc, ts, _ = shadow(X)
            assert int(c.min()) >= -127, (r0, int(c.min()))
            assert np.array_equal(s.view(np.uint32), ts.view(np.uint32)), (r0, np.nonzero(s != ts)[0][:8])
            assert np.array_equal(c, tc), (r0, np.nonzero((c != tc).any(axis=1))[0][:8])
            unb = unbounded_rows(X)
            seen_unbounded += int(unb.sum())
            assert not np.isnan(a).any()
            assert np.array_equal(np.isinf(a), unb), (r0, np.nonzero(np.isinf(a) != unb)[0][:8])
            assert np.all(a[unb] == np.inf) and np.all(s[unb] == 0) and not c[unb].any()
            ok = ~unb
            Xd, cd, sd = f64(X[ok]), f64(c[ok]), f64(s[ok])
            e = Xd - sd[:, None] * cd
            a_star = np.sqrt((e * e).sum(1)) + g * (np.sqrt((Xd * Xd).sum(1)) + sd * np.sqrt((cd * cd).sum(1)))
            a_ok = a[ok]
            assert np.all(a_star <= f64(a_ok)), (r0, float((a_star / f64(a_ok)).max()))
            # the kernel rounds SAFETY * a* UP to f32, so a_r is never below that double value; its double sums and
            # these differ by summation order only: (dim - 1) 2^-53 <= 2^-43 a sum of non-negative terms, 2^-40 in all
            low = SAFETY * a_star * (1 - 2.0 ** -40)
            assert np.all(low <= f64(a_ok)), (r0, float((low / np.maximum(f64(a_ok), 1e-300)).max()))
            lim = a_star * (1 + 2.0 ** -9) + f64(np.spacing(a_ok))
            assert np.all(f64(a_ok) <= lim), (r0, float((f64(a_ok) / np.maximum(a_star, 1e-300)).max()))
        assert seen_unbounded == 13 * len(pos)  # the synthetic rows are all bounded, the blocks hold 13 each
        # the blocks themselves once more against the twin of the rows that went up
        for p, B in pos:
            _, ts, ta = shadow(B)
            _, s, a = hook_shadow(idx, p, B.shape[0], codes=False)
            assert np.array_equal(s.view(np.uint32), ts.view(np.uint32))
            assert np.array_equal(np.isinf(a), np.isinf(ta))
    finally:
        mode(lab_build, True)
        idx.close()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_scan_bits_on_the_adversarial_rows(lab_build, oracle, dim, n):
    """b. with pruning off the f32 scan of the adversarial rows, wherever they lie, is oracle.scores_kernel_order bit
    for bit for every query, subnormal elements and non-finite rows included (a NaN equals a NaN)"""
    idx, A, pos = make_index(dim, n)
    try:
        mode(lab_build, False)
        for name, q, _ in edge_queries(A):
            S = idx.scores(q)
            for p, B in pos:
                with np.errstate(invalid="ignore", over="ignore"):
                    ref = oracle.scores_kernel_order(B, q)
                got = S[p:p + B.shape[0]]
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(got), nan), (name, p)
                assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32)), \
                    (name, p, np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0][:8])
    finally:
        mode(lab_build, True)
        idx.close()


WIDTH = {}  # dim -> the largest (S - lb) / (a Q) seen by test_every_row_is_contained (rows with a Q > 2^-80)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_every_row_is_contained(lab_build, dim, n):
    """c. for every query of norm up to 2^40 and every row with finite a_r (S_r = the device's full scan, float64):
    lb_r < S_r strictly; S_r - lb_r <= 2 a_r Q (1 + 2^-19) + |lb_r| 2^-19 + 2^-98 (DESIGN.md's ub with each slack term
    doubled: it implies ub_r > S_r and fails on uselessly low bounds); ||q|| <= Q <= ||q|| (1 + 2^-20).  A row with
    a_r = +inf has lb = -inf, except for the zero query: there Q = 0 and inf * 0 makes lb NaN.  The query of norm above
    2^40 sets the state's "cannot be bounded" word, and so does the zero query (a NaN bound among the k largest would be
    a threshold that keeps every row); the zero query's bounds are written and checked all the same.  After the hooks
    the buffer is marked partial with the query kept: topk without a query and scores() return the full scan."""
    idx, A, pos = make_index(dim, n)
    try:
        mode(lab_build, True, MIN_ROWS)
        _, _, a = hook_shadow(idx, codes=False)
        fin = np.isfinite(a)
        assert int((~fin).sum()) == 13 * len(pos)
        worst = WIDTH.get(dim, 0.0)
        for name, q, bounded in edge_queries(A):
            mode(lab_build, False)
            S = idx.scores(q)
            top = idx.topk(q, 64)
            mode(lab_build, True, MIN_ROWS)
            lb, Q, bad = hook_bounds(idx, q)
            same(top, idx.topk(None, 64))  # a reader of the partial buffer sees the full scan
            lb2, _, _ = hook_bounds(idx, q)
            same([lb], [lb2])
            same([S], [idx.scores(q)])
            norm = float(np.sqrt(np.sum(f64(q) ** 2)))
            assert norm <= float(Q) <= norm * (1 + 2.0 ** -20), (name, norm, float(Q))
            assert bad == (0 if bounded else 1), (name, bad)
            if norm > 2.0 ** 40:
                continue
            Sd, lbd, ad = f64(S[fin]), f64(lb[fin]), f64(a[fin])
            assert np.all(np.isfinite(Sd)) and np.all(np.isfinite(lbd)), name
            aq = ad * float(Q)
            wide_enough = aq > 2.0 ** -80  # below that the absolute pad 2^-100 is the width, not a Q (the 1e-30 query)
            ratio = (Sd - lbd)[wide_enough] / aq[wide_enough]
            if ratio.size:
                worst = max(worst, float(ratio.max()))
                WIDTH[dim] = worst
            msg = f"query '{name}', dim {dim}, n {n}: largest (S - lb) / (a Q) so far {worst:.6f}"
            assert np.all(lbd < Sd), (msg, np.nonzero(fin)[0][~(lbd < Sd)][:8])
            slack = 2 * aq * (1 + 2.0 ** -19) + np.abs(lbd) * 2.0 ** -19 + 2.0 ** -98
            wide = ~(Sd - lbd <= slack)
            assert not wide.any(), (msg, np.nonzero(fin)[0][wide][:8], float(((Sd - lbd) / slack).max()))
            if norm == 0:
                assert float(Q) == 0 and np.all(np.isnan(lb[~fin])), msg
            else:
                assert np.all(lb[~fin] == -np.inf), msg
        print(f"\nprune certificate: dim {dim} n {n}: largest (S - lb) / (a Q) = {worst:.6f}")
    finally:
        mode(lab_build, True)
        idx.close()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_survivors_against_a_chosen_threshold(lab_build, dim, n):
    """d. k_survivors + k_prune_publish over the device's bounds for thresholds the test chooses: the list has no
    duplicate and no row >= n, holds every row with S_r >= T, every NaN score and every row with a_r = +inf, and only rows
    whose doubled-slack upper bound reaches T (or is NaN); more qualifying rows than the capacity publish -1, never a
    cut list; a selection count below k, a raised overflow word and an unboundable query publish -1 and collect nothing"""
    idx, A, pos = make_index(dim, n)
    try:
        mode(lab_build, True, MIN_ROWS)
        _, _, a = hook_shadow(idx, codes=False)
        qs = edge_queries(A)
        for name, q, _ in (qs[0], qs[1]):
            mode(lab_build, False)
            S = idx.scores(q)
            top = idx.topk(q, 64)
            mode(lab_build, True, MIN_ROWS)
            lb, Q, bad = hook_bounds(idx, q)
            assert bad == 0
            ub2 = ub_doubled(lb, a, Q)
            ranked = np.sort(S[~np.isnan(S)])[::-1]  # one row an image here: the k-th image score is the k-th row's
            finite = S[np.isfinite(S)]
            Ts = [ranked[0], ranked[99], ranked[1023], finite.max(), np.float32(2) * np.abs(finite).max() + np.float32(1),
                  lb[np.isfinite(lb)].min()]
            for T, cap in [(t, SURV_CAP) for t in Ts] + [(ranked[1023], 512), (ranked[99], 99)]:
                T = np.float32(T)
                must = (S >= T) | np.isnan(S) | np.isinf(a)
                may = (ub2 >= float(T)) | np.isnan(ub2)
                assert not (must & ~may).any()  # the reference's own consistency
                pub, got, rows = hook_survivors(idx, T, 100, cap=cap)
                msg = (name, float(T), cap, pub, got, int(must.sum()), int(may.sum()))
                assert int(must.sum()) <= got <= int(may.sum()), msg
                assert pub == (-1 if got > cap else got), msg
                if int(must.sum()) > cap:
                    assert pub == -1, msg
                if pub >= 0:
                    assert rows.shape[0] == pub and np.unique(rows).shape[0] == pub, msg
                    assert rows.min(initial=0) >= 0 and rows.max(initial=0) < n, msg
                    inlist = np.zeros(n, dtype=bool)
                    inlist[rows] = True
                    assert not (must & ~inlist).any(), (msg, np.nonzero(must & ~inlist)[0][:8])
                    assert not (inlist & ~may).any(), (msg, np.nonzero(inlist & ~may)[0][:8])
            if n > SURV_CAP:  # every row qualifies against the lowest bound: more than the product's capacity
                assert hook_survivors(idx, Ts[-1], 100)[0] == -1
            # the threshold selection failed: fewer than k keys, or its overflow word
            assert hook_survivors(idx, ranked[99], 100, sel_count=99)[:2] == (-1, 0)
            assert hook_survivors(idx, ranked[99], 100, sel_overflow=1)[:2] == (-1, 0)
            assert hook_survivors(idx, ranked[99], 100)[0] >= 100
            # the buffer is still partial: its readers complete it
            same(top, idx.topk(None, 64))
            same([S], [idx.scores(q)])
        name, q, _ = qs[-1]
        _, _, bad = hook_bounds(idx, q)
        assert bad == 1
        assert hook_survivors(idx, np.float32(0), 100)[:2] == (-1, 0)
        mode(lab_build, False)
        top = idx.topk(q, 64)
        mode(lab_build, True, MIN_ROWS)
        hook_bounds(idx, q)
        same(top, idx.topk(None, 64))
    finally:
        mode(lab_build, True)
        idx.close()


def ragged_images(n, rng):
    """row2image with 1 .. 5 rows an image"""
    sizes = rng.integers(1, 6, n)
    r2i = np.repeat(np.arange(n, dtype=np.int64), sizes)[:n]
    return r2i.astype(np.int32)


@pytest.mark.parametrize("multi_row", [False, True])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", (256, 1024))
def test_topk_end_to_end_at_the_new_shapes(lab_build, dim, n, multi_row):
    """e. pruned and full top-k return the same bits at dim 256 and 1024 and ragged row counts with the adversarial rows
    in the index, for k in (1, 100, 1024) and every edge query, single-row and ragged multi-row images, with and
    without exclusions that remove the adversarial images.  The zero query and the query of norm above 2^40 (neither is
    bounded) report a fallback, every other call is pruned.  NaN scores: the
    full scan's own top-k is key_order_topk of the device's scores (a NaN with the sign bit clear leads the single-row
    top-k, a NaN row never represents a multi-row image), and the pruned call returns the same."""
    idx, A, pos = make_index(dim, n)
    try:
        r2i = None
        if multi_row:
            r2i = ragged_images(n, np.random.default_rng(4))
            idx.set_row2image(r2i)
        adv_rows = np.concatenate([np.arange(p, p + B.shape[0]) for p, B in pos])
        adv_images = adv_rows if r2i is None else np.unique(r2i[adv_rows])
        nan_led = False
        for name, q, bounded in edge_queries(A):
            mode(lab_build, False)
            S = idx.scores(q)
            for ex in (None, adv_images):
                for k in (1, 100, 1024):
                    full, got, st = both(lab_build, idx, lambda: idx.topk(q, k, excluded=ex), min_rows=MIN_ROWS)
                    msg = (name, k, ex is not None, st)
                    same(full, got)
                    assert len(got[0]) == k, msg
                    assert st[0] == 1, msg
                    if not bounded:
                        assert st[2] == -1, msg
                    else:
                        assert k <= st[2] <= SURV_CAP, msg
                    e_img, e_bits, e_rows = key_order_topk(S, r2i, ex, k)
                    assert np.array_equal(full[0], e_img), msg
                    assert np.array_equal(full[1].view(np.uint32), e_bits), msg
                    assert np.array_equal(full[2], e_rows), msg
                    nan_led = nan_led or bool(np.isnan(full[1][0]))
        if r2i is None:
            assert nan_led  # a NaN score did lead a top-k here: the case is not vacuous
    finally:
        mode(lab_build, True)
        idx.close()


@pytest.mark.parametrize("dim", (256, 1024))
def test_product_threshold_at_dim_256_and_1024(lab_build, dim):
    """e. once at the product's own threshold (no tuning): 2^22 + 37 synthetic rows are pruned at dim 256 and 1024"""
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic((1 << 22) + 37, dim, seed=7)
    try:
        q = np.random.default_rng(100).standard_normal(dim).astype(np.float32)
        q = (q / np.linalg.norm(q)).astype(np.float32)
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert len(got[0]) == 100
        assert st[0] == 1 and 100 <= st[2] < (1 << 18), st
    finally:
        mode(lab_build, True)
        idx.close()
