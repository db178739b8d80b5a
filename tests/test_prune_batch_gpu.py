"""GPU: the pruned batch (ssw_index_topk_batch_pruned; csrc/prune.hip k_q8_query_mq, k_q8_bounds_mq, k_survivors_mq,
k_prune_publish_mq) on the lab build.

1. The matrix core's lane map on exact integers: the kernel's int32 sums equal codes @ d for rows and queries that all
   differ, at every row count where the kernel's loop changes shape; the query codes, Q, e, t2 equal the numpy twin.
2. The certificate row by row against the device's full scan.
3. The survivors of one slot against chosen thresholds.
4. Results equal single full-scan top-k calls of a fresh handle, bit for bit.
5. The handle's state after the call.
6. One case at the product's default threshold (2^22 f16 rows).
7. A bad argument is refused with the plain batch's error before a shadow is built.

A non-finite query is SSW_ERR_NUMERIC for this entry point as for ssw_index_topk and ssw_index_topk_batch (there is no
single-call result it could equal); that the kernel flags one is checked through the hook."""
import numpy as np
import pytest

from _prune_batch_helpers import (edge_queries, flagged_queries, hook_bounds_mq, hook_survivors_mq, launch_shape,
                                  quantise_query, thresholds, upper_bound, width)
from _prune_helpers import adversarial_rows, hook_shadow, mode, same, stats

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
NQS = (1, 2, 15, 16)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def row_counts(dim):
    """the loop's shapes: one request of a wave is G = 16 x tiles rows, a full launch has W = 4 x blocks waves"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    probe = DeviceIndex(1 << 20, dim)  # large enough for an unclamped grid
    try:
        blocks, tiles = launch_shape(probe)
    finally:
        probe.close()
    assert blocks == torch.cuda.get_device_properties(0).multi_processor_count
    G, W = 16 * tiles, 4 * blocks
    counts = {1, 15, 16, 17, 63, 64, 65, G - 1, G + 1, W * G - 1, W * G + 1, 100_003, (1 << 16) + 1}
    return sorted(counts), G


def int_rows(n, dim, seed):
    """f32 rows that ARE their codes: integers in [-127, 127], every row with a 127 (s = 1), all patterns different"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-127, 128, (n, dim)).astype(np.float32)
    X[np.arange(n), np.arange(n) % dim] = 127.0
    return X


def the_queries(dim, seed=5):
    """16 queries, all different in direction and by orders of magnitude in norm"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((16, dim)) * np.exp2(rng.integers(-12, 13, 16))[:, None]
    Q[3] = edge_queries(rng, dim)[3]  # rint ties and clamped lo codes
    return np.ascontiguousarray(Q, dtype=np.float32)


def check_query_state(out, Q):
    """codes, Q, e, t2 and the flag of every slot against the twin, bit for bit -> the twins"""
    twins = [quantise_query(q) for q in Q]
    for j, t in enumerate(twins):
        assert bool(out["bad"][j]) == t["bad"], j
        assert np.array_equal(out["codes"][j, 0], t["d_hi"]) and np.array_equal(out["codes"][j, 1], t["d_lo"]), j
        if not t["bad"]:
            got = np.array([out["Q"][j], out["e"][j], out["t2"][j]], np.float32)
            want = np.array([t["Q"], t["e"], t["t2"]], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (j, got, want)
    return twins


@pytest.mark.parametrize("dim", DIMS)
def test_lane_map_on_exact_integers(lab_build, dim):
    from seesaw_amd.device_index import DeviceIndex
    counts, _ = row_counts(dim)
    Qall = the_queries(dim)
    try:
        for n in counts:
            X = int_rows(n, dim, seed=n)
            idx = DeviceIndex.from_numpy(X)
            try:
                mode(lab_build, True, 1)
                c, s, _ = hook_shadow(idx)
                assert np.array_equal(c, X.astype(np.int8)) and np.all(s == 1)
                cf = c.astype(np.float32)  # |sums| <= 1024 * 127^2 < 2^24: exact in f32
                for nq in NQS:
                    Q = Qall[16 - nq:]  # another query in slot 0 every time
                    out = hook_bounds_mq(idx, Q)
                    check_query_state(out, Q)
                    for name, plane in (("I_hi", 0), ("I_lo", 1)):
                        want = (cf @ out["codes"][:, plane].astype(np.float32).T).T.astype(np.int64)
                        got = out[name].astype(np.int64)
                        assert np.array_equal(got, want), (dim, n, nq, name, np.argwhere(got != want)[:4])
            finally:
                idx.close()
    finally:
        mode(lab_build, True)


def float_rows(n, dim, G, seed):
    """Gaussian rows of mixed scale with the adversarial rows over the first rows, a request boundary and the last rows"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    adv = adversarial_rows(rng, dim)
    m = adv.shape[0]
    X[:min(m, n)] = adv[:min(m, n)]
    if n >= 4 * m + 2 * G:
        at = ((n // 2) // G) * G - m // 2  # straddles a boundary between two requests
        X[at:at + m] = adv
    if n >= 2 * m:
        X[n - m:] = adv[::-1]
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("dim", DIMS)
def test_certificate_row_by_row(lab_build, dim):
    from seesaw_amd.device_index import DeviceIndex
    counts, G = row_counts(dim)
    rng = np.random.default_rng(11)
    Qall = np.stack(edge_queries(rng, dim) + [q for q in the_queries(dim, 9)[:8]])
    try:
        for n in counts:
            X = float_rows(n, dim, G, seed=n)
            idx = DeviceIndex.from_numpy(X)
            try:
                mode(lab_build, False)
                S = np.stack([idx.scores(q) for q in Qall])  # the device's full scan
                mode(lab_build, True, 1)
                _, s, a = hook_shadow(idx, codes=False)
                fin = np.isfinite(a)
                for nq in NQS:
                    sel = np.arange(16 - nq, 16)
                    out = hook_bounds_mq(idx, Qall[sel], sums=False)
                    twins = check_query_state(out, Qall[sel])
                    for j, t in enumerate(twins):
                        assert not t["bad"]
                        lb, Sd = f64(out["lb"][j]), f64(S[sel[j]])
                        assert np.all(out["lb"][j][~fin] == -np.inf), (dim, n, nq, j)
                        w = width(s, a, t, dim)[fin]
                        l, sv = lb[fin], Sd[fin]
                        rows = np.nonzero(fin)[0]
                        assert np.all(np.isfinite(l)) and np.all(np.isfinite(sv)), (dim, n, nq, j)
                        assert np.all(l < sv), (dim, n, nq, j, rows[~(l < sv)][:8])
                        slack = 2 * w * (1 + 2.0 ** -19) + np.abs(l) * 2.0 ** -19 + 2.0 ** -98
                        wide = ~(sv - l <= slack)
                        assert not wide.any(), (dim, n, nq, j, rows[wide][:8], float(((sv - l) / slack).max()))
            finally:
                idx.close()
    finally:
        mode(lab_build, True)


@pytest.mark.parametrize("dim", DIMS)
def test_survivors_of_one_slot(lab_build, dim):
    from seesaw_amd.device_index import DeviceIndex
    n = 4099
    X = float_rows(n, dim, 32, seed=3)
    idx = DeviceIndex.from_numpy(X)
    try:
        rng = np.random.default_rng(2)
        Q = np.stack([rng.standard_normal(dim) * 40.0, np.zeros(dim), rng.standard_normal(dim) * 0.01,
                      flagged_queries(dim)[1], rng.standard_normal(dim)]).astype(np.float32)
        nq = Q.shape[0]
        mode(lab_build, False)
        S = {j: f64(idx.scores(Q[j])) for j in (0, 2, 4)}
        mode(lab_build, True, 1)
        _, s, a = hook_shadow(idx, codes=False)
        out = hook_bounds_mq(idx, Q, sums=False)
        twins = check_query_state(out, Q)
        assert [t["bad"] for t in twins] == [False, True, False, True, False]
        for j in (0, 2, 4):
            ub = upper_bound(out["lb"][j], width(s, a, twins[j], dim))
            for T in thresholds(ub):
                expect = np.nonzero(~(ub < float(T)))[0]
                pub, got, rows = hook_survivors_mq(idx, nq, j, T, 1)
                msg = (dim, j, float(T), pub, got, expect.shape[0])
                assert pub == got == expect.shape[0], msg
                assert np.array_equal(np.sort(rows), expect), msg
                with np.errstate(invalid="ignore"):
                    must = (S[j] >= float(T)) | np.isnan(S[j]) | np.isinf(a)
                assert np.all(np.isin(np.nonzero(must)[0], rows)), msg
            T = thresholds(ub)[-1]  # keeps all n rows
            assert hook_survivors_mq(idx, nq, j, T, 1, cap=n - 1)[:2] == (-1, n)  # more than the list holds
            assert hook_survivors_mq(idx, nq, j, T, 5, sel_count=4)[:2] == (-1, 0)  # fewer than k keys
            assert hook_survivors_mq(idx, nq, j, T, 5, sel_overflow=1)[:2] == (-1, 0)  # the selection overflowed
            assert hook_survivors_mq(idx, nq, j, T, 5)[:2] == (n, n)  # and the failure mark does not stick
        for j in (1, 3):  # a flagged query collects nothing and publishes -1
            assert hook_survivors_mq(idx, nq, j, np.float32(-1e30), 1)[:2] == (-1, 0)
    finally:
        idx.close()
        mode(lab_build, True)


N_RESULT = (1 << 17) + 37


def reference(ref, Q, k, ex):
    return [ref.topk(Q[b], k, excluded=None if ex is None else ex[b]) for b in range(Q.shape[0])]


def batch_queries(nq, dim=512, seed=0):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True) * np.exp2(rng.integers(-3, 4, nq))[:, None],
                                dtype=np.float32)


@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_results_equal_single_full_scans(lab_build, dtype, with_map):
    from seesaw_amd.device_index import DeviceIndex
    n = N_RESULT
    idx = DeviceIndex.synthetic(n, 512, seed=21, dtype=dtype)
    ref = DeviceIndex.synthetic(n, 512, seed=21, dtype=dtype)
    try:
        if with_map:
            r2i = (np.arange(n, dtype=np.int64) // 3).astype(np.int32)
            idx.set_row2image(r2i)
            ref.set_row2image(r2i)
        n_img = idx.n_images
        rng = np.random.default_rng(4)
        for nq in (1, 2, 15, 16, 17, 33):
            Q = batch_queries(nq, seed=nq)
            ex = [None if b % 3 == 0 else rng.choice(n_img, 5 + 40 * b, replace=False) for b in range(nq)]
            for k, e in ((1, None), (100, ex)):
                mode(lab_build, False)
                want = reference(ref, Q, k, e)
                mode(lab_build, True, 1)
                before = stats(idx)
                got = idx.topk_batch(Q, k, excluded=e, prune=True)
                st = stats(idx)
                for b in range(nq):
                    same(want[b], got[b])
                    assert len(got[b][0]) == k
                assert st[3] - before[3] == nq and st[4] == before[4] and st[2] >= k, (nq, k, before, st)
        # queries that cannot be bounded among ordinary ones: they alone take the full scan
        Q = batch_queries(7, seed=99)
        Q[1] = 0.0
        Q[4] = flagged_queries(512)[3]
        Q[6] = flagged_queries(512)[4]
        mode(lab_build, False)
        want = reference(ref, Q, 100, None)
        mode(lab_build, True, 1)
        before = stats(idx)
        got = idx.topk_batch(Q, 100, prune=True)
        st = stats(idx)
        for b in range(7):
            same(want[b], got[b])
        assert st[3] - before[3] == 7 and st[4] - before[4] == 3 and st[2] == -1, (before, st)
        # fewer images left than k for one query only: its threshold selection returns fewer than k keys
        Q = batch_queries(5, seed=98)
        keep = rng.choice(n_img, 40, replace=False)
        ex = [None, None, np.setdiff1d(np.arange(n_img), keep), rng.choice(n_img, 9, replace=False), None]
        mode(lab_build, False)
        want = reference(ref, Q, 100, ex)
        mode(lab_build, True, 1)
        before = stats(idx)
        got = idx.topk_batch(Q, 100, excluded=ex, prune=True)
        st = stats(idx)
        for b in range(5):
            same(want[b], got[b])
        assert len(got[2][0]) == 40 and st[4] - before[4] == 1 and st[3] - before[3] == 5, (before, st)
        # a non-finite query is refused before anything runs, as by the plain batch and the single call
        Q[3, 7] = np.nan
        for call in (lambda: idx.topk_batch(Q, 10, prune=True), lambda: idx.topk_batch(Q, 10), lambda: idx.topk(Q[3], 10)):
            with pytest.raises(Exception, match="non-finite"):
                call()
        assert np.array_equal(stats(idx)[3:5], st[3:5])
    finally:
        idx.close()
        ref.close()
        mode(lab_build, True)


def test_state_after_the_call(lab_build):
    from seesaw_amd.device_index import DeviceIndex
    n, k = N_RESULT, 50
    idx = DeviceIndex.synthetic(n, 512, seed=31)
    ref = DeviceIndex.synthetic(n, 512, seed=31)
    try:
        Q = batch_queries(19, seed=7)
        ex = [np.arange(b, 3 * b + 1) for b in range(19)]
        rows = np.random.default_rng(0).choice(n, 2000, replace=False)
        mode(lab_build, False)
        last = ref.topk(Q[-1], k, excluded=ex[-1])
        again = ref.topk(None, k)
        gathered = ref.gather_scores(rows)
        plain = ref.topk_batch(Q[:5], k)
        single = ref.topk(Q[2], k)
        mode(lab_build, True, 1)
        got = idx.topk_batch(Q, k, excluded=ex, prune=True)
        same(last, got[-1])
        st = idx.prune_stats()
        assert st["last_survivors"] >= k and st["queries"] == 19 and st["fallbacks"] == 0, st
        same(again, idx.topk(None, k))  # the last query's resident scores, completed, and its exclusions
        same([gathered], [idx.gather_scores(rows)])
        idx.topk_batch(Q, k, excluded=ex, prune=True)
        for a, b in zip(plain, idx.topk_batch(Q[:5], k)):  # a plain batch after it: unaffected, counters alone
            same(a, b)
        assert idx.prune_stats()["queries"] == 38
        idx.topk_batch(Q, k, excluded=ex, prune=True)
        same(single, idx.topk(Q[2], k))  # a pruned single call after it
        assert idx.prune_stats()["queries"] == 58 and idx.prune_stats()["last_survivors"] >= k
        # an index that is not pruned takes the plain batch and leaves the counters alone
        mode(lab_build, True, n + 1)
        before = stats(idx)
        for a, b in zip(plain, idx.topk_batch(Q[:5], k, prune=True)):
            same(a, b)
        assert np.array_equal(stats(idx)[2:5], before[2:5]) and stats(idx)[1] == 0
    finally:
        idx.close()
        ref.close()
        mode(lab_build, True)


def test_default_threshold_f16(lab_build):
    """the product's own threshold: 2^22 binary16 rows filled on the device, 16 queries, no fallback"""
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(1 << 22, 512, seed=7, dtype=np.float16)
    try:
        mode(lab_build, True)
        Q = batch_queries(16, seed=3)
        plain = idx.topk_batch(Q, 100)
        assert stats(idx)[3] == 0
        got = idx.topk_batch(Q, 100, prune=True)
        for a, b in zip(plain, got):
            same(a, b)
        st = stats(idx)
        assert st[0] == 1 and st[3] == 16 and st[4] == 0 and 100 <= st[2] < (1 << 18), st
    finally:
        idx.close()


def test_invalid_arguments_are_refused_before_the_shadow(lab_build):
    """a pruned batch with a bad argument returns the plain batch's error and allocates and launches nothing: no shadow
    is built for it and no query is counted; the valid call after it builds the shadow and equals the single calls"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex, _ptr
    n, dim, k, nq = 1000, 256, 10, 3
    rows = np.random.default_rng(11).standard_normal((n, dim)).astype(np.float32)
    r2i = (np.arange(n) // 4).astype(np.int32)
    mode(lab_build, True, 1)
    idx = DeviceIndex.from_numpy(rows, row2image=r2i)
    try:
        Q = batch_queries(nq, dim=dim, seed=2)
        bad_q = Q.copy()
        bad_q[1, 5] = np.nan
        ids = np.arange(6, dtype=np.int64)
        down = np.array([0, 4, 2, 6], dtype=np.int64)
        out = [np.empty((nq, k), np.int64), np.empty((nq, k), np.float32), np.empty((nq, k), np.int64), np.zeros(nq, np.int32)]

        def raw(name):  # decreasing offsets: DeviceIndex.topk_batch cannot express them
            _lib.call(name, idx._h, _ptr(Q), nq, _ptr(ids), _ptr(down), k, *[_ptr(a) for a in out])

        cases = [(_lib.SSW_ERR_NUMERIC, "query 1 of the batch has a non-finite component at 5",
                  lambda prune: idx.topk_batch(bad_q, k, prune=prune)),
                 (_lib.SSW_ERR_INVALID, "excluded_offsets decrease at query 1",
                  lambda prune: raw("ssw_index_topk_batch_pruned" if prune else "ssw_index_topk_batch")),
                 (_lib.SSW_ERR_INVALID, r"excluded image 250 outside \[0, 250\)",
                  lambda prune: idx.topk_batch(Q, k, excluded=[None, [3], [7, idx.n_images]], prune=prune))]
        for status, message, call in cases:
            with pytest.raises(_lib.SeesawHipError, match=message) as plain:
                call(False)
            with pytest.raises(_lib.SeesawHipError, match=message) as pruned:
                call(True)
            assert pruned.value.status == plain.value.status == status
            assert str(pruned.value) == str(plain.value)
            st = idx.prune_stats()
            assert st["shadow"] == "none" and st["queries"] == 0, (message, st)
        ex = [None, [3], [7, 9]]
        got = idx.topk_batch(Q, k, excluded=ex, prune=True)
        st = idx.prune_stats()
        assert st["shadow"] == "current" and st["queries"] == nq, st
        for b in range(nq):
            same(idx.topk(Q[b], k, excluded=ex[b]), got[b])
    finally:
        idx.close()
        mode(lab_build, True)
