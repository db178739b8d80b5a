"""GPU: the pruned batch on the packed 6-bit shadow (csrc/prune.hip: k_q6_query_mq, k_q6_bounds_mq, k_survivors_mq with the
6-bit code norm; csrc/index_prune.hip: prune_batch_shadow) on the lab build.

1. The matrix core's lane map on exact integers: the hook's I of every slot equals the numpy integer dot for rows and
   queries that all differ, at every row count where the kernel's loop changes shape; codes, Q, e, t2 and the flag of
   every slot equal the numpy twin bit for bit.
2. The certificate row by row against the device's full scan.
3. The survivors of one slot against chosen thresholds.
4. Results: topk_batch / topk_batch_avg / topk_batch_dev with prune=True equal the same call with pruning off on a fresh
   handle, byte for byte.
5. The shadow that was used: the 6-bit one alone, no int8 shadow beside it.
6. Fallbacks.
7. The product's own thresholds: the 6-bit shadow from 25 M rows, the int8 shadow below.

Every case switches every index onto the pruned path from one row on, for the int8 and for the 6-bit shadow
(ssw_tune_prune(1, 1, -1), ssw_tune_prune6(1, 1)), lowers the batch's own 6-bit threshold to one row as well
(ssw_tune_prune6_batch(1): ssw_tune_prune6 moves the single call's constant alone) and restores all three."""
import ctypes

import numpy as np
import pytest

from _prune6_helpers import hook_shadow6, integer_sums, mode6, quantise_query, width6
from _prune_batch_helpers import edge_queries, flagged_queries, thresholds, upper_bound
from _prune_helpers import adversarial_rows, mode, same, stats

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
NQS = (1, 2, 15, 16)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def bytes6(n, dim):
    """device memory of the 6-bit shadow: whole 16-row tiles of 3 dim / 4 code bytes and two floats a row"""
    return (n + 15) // 16 * 16 * (dim * 3 // 4 + 8)


def batch6(min_rows):
    """the batch's own 6-bit threshold (ssw_tune_prune6_batch); < 0: the product's constants"""
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune6_batch", int(min_rows))


@pytest.fixture()
def six(lab_build):
    """every index is pruned from one row on, single queries and batches on the 6-bit shadow; the defaults afterwards"""
    mode(lab_build, True, 1)
    mode6(True, 1)
    batch6(1)
    try:
        yield lab_build
    finally:
        batch6(-1)
        mode6(True, -1)
        mode(lab_build, True)


def unpruned(six, fn):
    """fn() with the pruning off, then the fixture's switches again"""
    mode(six, False)
    try:
        return fn()
    finally:
        mode(six, True, 1)
        mode6(True, 1)


# ---- the lab hooks of the 6-bit chunk (include/seesaw_hip_debug.h) ---------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def launch_shape6_mq(idx):
    """(four-wave blocks, 16-row tiles of one request) of the next k_q6_bounds_mq launch over idx"""
    from seesaw_amd import _lib
    b, t = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune6_scan_mq_shape", idx._h, ctypes.byref(b), ctypes.byref(t))
    return int(b.value), int(t.value)


def hook_bounds6_mq(idx, Q, sums=True):
    """k_q6_query_mq + k_q6_bounds_mq: dict(I int64 [nq, n] (or None), lb f32 [nq, n], Q, e, t2 f32 [nq], bad bool [nq],
    codes int8 [nq, 2, dim])"""
    from seesaw_amd import _lib
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq, n = Q.shape[0], idx.n_rows
    I = np.empty((nq, n), np.int64) if sums else None
    lb, qe = np.empty((nq, n), np.float32), np.empty((nq, 4), np.float32)
    codes = np.empty((nq, 2, idx.dim), np.int8)
    _lib.call("ssw_debug_prune6_bounds_mq", idx._h, _p(Q), nq, _p(I), _p(lb), _p(qe), _p(codes))
    return dict(I=I, lb=lb, Q=qe[:, 0].copy(), e=qe[:, 1].copy(), t2=qe[:, 2].copy(), bad=qe[:, 3] != 0, codes=codes)


def hook_survivors6_mq(idx, nq, slot, threshold, k, sel_count=None, sel_overflow=0, cap=1 << 18):
    """k_survivors_mq of one slot of the 6-bit chunk + k_prune_publish_mq: (published, collected, rows int64)"""
    from seesaw_amd import _lib
    rows = np.full(max(int(cap), 1), -1, dtype=np.int64)
    pub, got = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.call("ssw_debug_prune6_survivors_mq", idx._h, int(nq), int(slot), ctypes.c_float(float(threshold)), int(k),
              int(k if sel_count is None else sel_count), int(sel_overflow), int(cap), ctypes.byref(pub),
              ctypes.byref(got), _p(rows))
    return int(pub.value), int(got.value), rows[:max(int(pub.value), 0)]


def row_counts(dim):
    """the loop's shapes: one request of a wave is G = 16 x tiles rows, a full launch has W = 4 x blocks waves"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    probe = DeviceIndex(1 << 20, dim)  # large enough for an unclamped grid
    try:
        blocks, tiles = launch_shape6_mq(probe)
    finally:
        probe.close()
    assert blocks == torch.cuda.get_device_properties(0).multi_processor_count and tiles * dim <= 1024
    G, W = 16 * tiles, 4 * blocks
    return sorted({1, 15, 16, 17, G - 1, G + 1, W * G - 1, W * G + 1, 100_003, (1 << 16) + 1}), G


def int_rows(n, dim, seed):
    """f32 rows that ARE their codes: integers in [-31, 31], every row with a 31 (s6 = 1), all patterns different"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-31, 32, (n, dim)).astype(np.float32)
    X[np.arange(n), np.arange(n) % dim] = 31.0
    return X


def the_queries(dim, seed=5):
    """16 queries, all different in direction and by orders of magnitude in norm"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((16, dim)) * np.exp2(rng.integers(-12, 13, 16))[:, None]
    Q[3] = edge_queries(rng, dim)[3]  # rint ties and clamped lo codes
    return np.ascontiguousarray(Q, dtype=np.float32)


def check_query_state(out, twins):
    """codes, Q, e, t2 and the flag of every slot against the twin, bit for bit"""
    for j, t in enumerate(twins):
        assert bool(out["bad"][j]) == t["bad"], j
        assert np.array_equal(out["codes"][j, 0], t["d_hi"]) and np.array_equal(out["codes"][j, 1], t["d_lo"]), j
        if not t["bad"]:
            got = np.array([out["Q"][j], out["e"][j], out["t2"][j]], np.float32)
            want = np.array([t["Q"], t["e"], t["t2"]], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (j, got, want)


@pytest.mark.parametrize("dim", DIMS)
def test_lane_map_on_exact_integers(six, dim):
    from seesaw_amd.device_index import DeviceIndex
    counts, _ = row_counts(dim)
    Qall = the_queries(dim)
    twins = [quantise_query(q) for q in Qall]
    # |I| <= 1024 * 124 * (256 * 127 + 127) < 2^33: the float64 product is the exact integer dot
    D = np.stack([256.0 * t["d_hi"].astype(np.float64) + t["d_lo"].astype(np.float64) for t in twins])
    for n in counts:
        X = int_rows(n, dim, seed=n)
        idx = DeviceIndex.from_numpy(X)
        try:
            c, s, _ = hook_shadow6(idx)
            assert np.array_equal(c, X.astype(np.int8)) and np.all(s == 1)
            want = ((4.0 * c.astype(np.float64)) @ D.T).T.astype(np.int64)  # [16, n], once for every nq
            assert np.array_equal(want[5, :64], integer_sums(c[:64], twins[5]))
            for nq in NQS:
                sel = slice(16 - nq, 16)  # another query in slot 0 every time
                out = hook_bounds6_mq(idx, Qall[sel])
                check_query_state(out, twins[sel])
                assert np.array_equal(out["I"], want[sel]), (dim, n, nq, np.argwhere(out["I"] != want[sel])[:4])
            st = stats(idx)
            assert st[0] == 1 and st[5] == bytes6(n, dim), st  # the hook built the 6-bit shadow and no other
        finally:
            idx.close()


def float_rows(n, dim, G, seed):
    """Gaussian rows of mixed scale with the adversarial rows over the first rows, a tile boundary and the last rows"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    adv = adversarial_rows(rng, dim)
    m = adv.shape[0]
    X[:min(m, n)] = adv[:min(m, n)]
    if n >= 4 * m + 2 * G:
        at = ((n // 2) // G) * G - m // 2  # straddles a boundary between two requests (and two tiles)
        X[at:at + m] = adv
    if n >= 2 * m:
        X[n - m:] = adv[::-1]
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("dim", DIMS)
def test_certificate_row_by_row(six, dim):
    from seesaw_amd.device_index import DeviceIndex
    counts, G = row_counts(dim)
    rng = np.random.default_rng(11)
    Qall = np.stack(edge_queries(rng, dim) + [q for q in the_queries(dim, 9)[:8]])
    twins = [quantise_query(q) for q in Qall]
    assert not any(t["bad"] for t in twins)
    for n in counts:
        X = float_rows(n, dim, G, seed=n)
        idx = DeviceIndex.from_numpy(X)
        try:
            S = unpruned(six, lambda: np.stack([idx.scores(q) for q in Qall]))  # the device's full scan, once
            _, s, a = hook_shadow6(idx, codes=False)
            fin = np.isfinite(a)
            rows = np.nonzero(fin)[0]
            for nq in NQS:
                sel = np.arange(16 - nq, 16)
                out = hook_bounds6_mq(idx, Qall[sel], sums=False)
                check_query_state(out, [twins[i] for i in sel])
                for j, qi in enumerate(sel):
                    lb, Sd = f64(out["lb"][j]), f64(S[qi])
                    assert np.all(out["lb"][j][~fin] == -np.inf), (dim, n, nq, j)
                    w = width6(s, a, twins[qi], dim)[fin]
                    l, sv = lb[fin], Sd[fin]
                    assert np.all(np.isfinite(l)) and np.all(np.isfinite(sv)), (dim, n, nq, j)
                    assert np.all(l < sv), (dim, n, nq, j, rows[~(l < sv)][:8])
                    slack = 2 * w * (1 + 2.0 ** -19) + np.abs(l) * 2.0 ** -19 + 2.0 ** -98
                    wide = ~(sv - l <= slack)
                    assert not wide.any(), (dim, n, nq, j, rows[wide][:8], float(((sv - l) / slack).max()))
        finally:
            idx.close()


@pytest.mark.parametrize("dim", DIMS)
def test_survivors_of_one_slot(six, dim):
    from seesaw_amd.device_index import DeviceIndex
    n = 4099
    X = float_rows(n, dim, 32, seed=3)
    idx = DeviceIndex.from_numpy(X)
    try:
        rng = np.random.default_rng(2)
        Q = np.stack([rng.standard_normal(dim) * 40.0, np.zeros(dim), rng.standard_normal(dim) * 0.01,
                      flagged_queries(dim)[1], rng.standard_normal(dim)]).astype(np.float32)
        nq = Q.shape[0]
        S = unpruned(six, lambda: {j: f64(idx.scores(Q[j])) for j in (0, 2, 4)})
        _, s, a = hook_shadow6(idx, codes=False)
        out = hook_bounds6_mq(idx, Q, sums=False)
        twins = [quantise_query(q) for q in Q]
        check_query_state(out, twins)
        assert [t["bad"] for t in twins] == [False, True, False, True, False]
        for j in (0, 2, 4):
            ub = upper_bound(out["lb"][j], width6(s, a, twins[j], dim))
            for T in thresholds(ub):
                expect = np.nonzero(~(ub < float(T)))[0]
                pub, got, rows = hook_survivors6_mq(idx, nq, j, T, 1)
                msg = (dim, j, float(T), pub, got, expect.shape[0])
                assert pub == got == expect.shape[0], msg
                assert np.array_equal(np.sort(rows), expect), msg
                with np.errstate(invalid="ignore"):
                    must = (S[j] >= float(T)) | np.isnan(S[j]) | np.isinf(a)
                assert np.all(np.isin(np.nonzero(must)[0], rows)), msg  # every row it must keep
            T = thresholds(ub)[-1]  # keeps all n rows
            assert hook_survivors6_mq(idx, nq, j, T, 1, cap=n - 1)[:2] == (-1, n)  # more than the list holds
            assert hook_survivors6_mq(idx, nq, j, T, 5, sel_count=4)[:2] == (-1, 0)  # fewer than k keys
            assert hook_survivors6_mq(idx, nq, j, T, 5, sel_overflow=1)[:2] == (-1, 0)  # the selection overflowed
            assert hook_survivors6_mq(idx, nq, j, T, 5)[:2] == (n, n)  # and the failure mark does not stick
        for j in (1, 3):  # a flagged query collects nothing and publishes -1
            assert hook_survivors6_mq(idx, nq, j, np.float32(-1e30), 1)[:2] == (-1, 0)
    finally:
        idx.close()


# ---- results ---------------------------------------------------------------------------------------------------------
N_RESULT = (1 << 17) + 37
NQ_RESULT = (1, 3, 16, 19)  # 19: a second, ragged chunk


def batch_queries(nq, dim=512, seed=0):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True) * np.exp2(rng.integers(-3, 4, nq))[:, None],
                                dtype=np.float32)


def exclusions(ref, Q):
    """per query every other image of its exact top-100: part of the exact top-k is gone (query 1 excludes nothing)"""
    top = ref.topk_batch(Q, 100)
    return [None if b == 1 else np.sort(top[b][0][::2]) for b in range(Q.shape[0])]


@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_results_equal_the_plain_batch_of_a_fresh_handle(six, dtype, with_map):
    from seesaw_amd.device_index import DeviceIndex
    n = N_RESULT
    idx = DeviceIndex.synthetic(n, 512, seed=21, dtype=dtype)
    ref = DeviceIndex.synthetic(n, 512, seed=21, dtype=dtype)
    try:
        if with_map:
            r2i = (np.arange(n, dtype=np.int64) // 3).astype(np.int32)
            idx.set_row2image(r2i)
            ref.set_row2image(r2i)
        first = True
        for nq in NQ_RESULT:
            Q = batch_queries(nq, seed=nq)
            ex = unpruned(six, lambda: exclusions(ref, Q))
            for k in (1, 100):
                want = unpruned(six, lambda: ref.topk_batch(Q, k, excluded=ex))
                before = stats(idx)
                got = idx.topk_batch(Q, k, excluded=ex, prune=True)
                st = stats(idx)
                for b in range(nq):
                    same(want[b], got[b])
                    assert len(got[b][0]) == k
                assert st[3] - before[3] == nq and st[4] == before[4] and st[2] >= k, (nq, k, before, st)
                if first:  # case 5 on the first call of all: the 6-bit shadow bounded it, and nothing else was built
                    ps = idx.prune_stats()
                    assert ps["shadow"] == "current" and ps["queries"] == nq and ps["fallbacks"] == 0, ps
                    assert ps["shadow_bytes"] == bytes6(n, 512), ps
                    first = False
        assert stats(idx)[5] == bytes6(n, 512)
    finally:
        idx.close()
        ref.close()


def tiled_index(n, dtype=np.float32, seed=4):
    """four tiles an image: a full-image tile at zoom 0 and three quadrants at zoom 1"""
    from seesaw_amd.device_index import DeviceIndex
    assert n % 4 == 0
    h = DeviceIndex.synthetic(n, 512, seed=seed, dtype=dtype)
    h.set_row2image((np.arange(n, dtype=np.int64) // 4).astype(np.int32))
    boxes = np.tile(np.array([[0, 0, 1, 1], [0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1]], np.float32), (n // 4, 1))
    h.set_tile_meta(boxes, np.tile(np.array([0, 1, 1, 1], np.int32), n // 4))
    return h


def test_two_stage_results_equal_the_plain_batch(six):
    n, k = (1 << 16) + 36, 100
    idx, ref = tiled_index(n), tiled_index(n)
    try:
        for nq in NQ_RESULT:
            Q = batch_queries(nq, seed=40 + nq)
            ex = unpruned(six, lambda: exclusions(ref, Q))
            for kk, aug in ((1, "all"), (k, "greater")):
                want = unpruned(six, lambda: ref.topk_batch_avg(Q, kk, aug, excluded=ex))
                before = idx.prune_stats(completions=True)
                got = idx.topk_batch_avg(Q, kk, aug, excluded=ex, prune=True)
                now = idx.prune_stats(completions=True)
                for w, g in zip(want, got):
                    same(w, g)
                assert now["queries"] - before["queries"] == nq and now["fallbacks"] == before["fallbacks"], (before, now)
                assert now["completions"] == before["completions"], (before, now)
        assert idx.prune_stats()["shadow_bytes"] == bytes6(n, 512)
    finally:
        idx.close()
        ref.close()


def test_device_batch_messages_equal_the_plain_call(six):
    import torch
    from seesaw_amd.device_index import DeviceIndex
    n, k_max, slots = N_RESULT, 128, 24
    dev = torch.device("cuda", 0)
    idx = DeviceIndex.synthetic(n, 512, seed=23)
    ref = DeviceIndex.synthetic(n, 512, seed=23)
    plain_block = torch.full((slots, 2 * k_max + 1), -1, dtype=torch.int64, device=dev)
    block = torch.full((slots, 2 * k_max + 1), -1, dtype=torch.int64, device=dev)
    try:
        for h, blk in ((idx, block), (ref, plain_block)):
            h.set_row2image((np.arange(n, dtype=np.int64) // 3).astype(np.int32))
            h.set_exchange_target_batch(blk.data_ptr(), slots, k_max, True, 1000, 5000)
        for nq in NQ_RESULT:
            Q = batch_queries(nq, seed=60 + nq)
            ex = unpruned(six, lambda: exclusions(ref, Q))
            for k in (1, 100):
                def plain():
                    plain_block.fill_(-1)
                    ref.topk_batch_dev(Q, k, excluded=ex, first_slot=2)
                    ref.sync()
                    return plain_block.cpu().numpy(), ref.topk(None, k, excluded=ex[-1])
                want, want_last = unpruned(six, plain)
                block.fill_(-1)
                before = stats(idx)
                idx.topk_batch_dev(Q, k, excluded=ex, first_slot=2, prune=True)
                idx.sync()
                got = block.cpu().numpy()
                assert np.array_equal(got, want), (nq, k, np.argwhere(got != want)[:4])
                assert ((got[2:2 + nq, -1] >> 32) == 0).all() and (got[2:2 + nq, -1] == k).all()
                surv, why = idx.prune_batch_dev_counts()
                assert surv.shape[0] == (nq - 1) % 16 + 1 and not why.any() and (surv >= k).all(), (nq, k, surv, why)
                assert stats(idx)[3] - before[3] == nq
                same(want_last, idx.topk(None, k, excluded=ex[-1]))  # the handle: the last query's, completed
        assert stats(idx)[5] == bytes6(n, 512)
    finally:
        idx.close()
        ref.close()


def upload(idx, first, X):
    from seesaw_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float32)
    _lib.call("ssw_index_upload", idx._h, X.ctypes.data_as(ctypes.c_void_p), int(first), X.shape[0])


def test_the_shadow_that_was_used(six):
    """a six-eligible index runs its pruned batches on the 6-bit shadow and never allocates the int8 one; with the
    6-bit path switched off the same call holds the int8 shadow, as before; an upload makes the 6-bit shadow stale and
    the next pruned batch rebuilds it and returns the new rows"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim, k, nq = N_RESULT, 512, 100, 19
    Q = batch_queries(nq, seed=7)
    idx = DeviceIndex.synthetic(n, dim, seed=31)
    ref = DeviceIndex.synthetic(n, dim, seed=31)
    try:
        want = unpruned(six, lambda: ref.topk_batch(Q, k))
        got = idx.topk_batch(Q, k, prune=True)
        for w, g in zip(want, got):
            same(w, g)
        ps = idx.prune_stats()
        assert ps["shadow"] == "current" and ps["queries"] == nq and ps["fallbacks"] == 0 and ps["eligible"], ps
        assert ps["shadow_bytes"] == bytes6(n, dim), ps  # the 6-bit shadow alone
        idx.topk(Q[0], k)  # a single query shares it
        assert idx.prune_stats()["shadow_bytes"] == bytes6(n, dim) and idx.prune_stats()["queries"] == nq + 1
        # rows that win for query 4, across a tile boundary: stale, rebuilt, found
        first = 70_000 - 3
        new = np.repeat((Q[4] * np.float32(3.0))[None, :], 7, axis=0)
        for h in (idx, ref):
            upload(h, first, new)
        assert idx.prune_stats()["shadow"] == "stale"
        want = unpruned(six, lambda: ref.topk_batch(Q, k))
        got = idx.topk_batch(Q, k, prune=True)
        for w, g in zip(want, got):
            same(w, g)
        assert got[4][2][0] == first and set(range(first, first + 7)) <= set(got[4][0][:7].tolist())
        ps = idx.prune_stats()
        assert ps["shadow"] == "current" and ps["shadow_bytes"] == bytes6(n, dim) and ps["fallbacks"] == 0, ps
    finally:
        idx.close()
    # the 6-bit path off: the same call on a fresh handle builds and holds the int8 shadow
    other = DeviceIndex.synthetic(n, dim, seed=31)
    try:
        upload(other, first, new)
        want = unpruned(six, lambda: ref.topk_batch(Q, k))
        mode6(False)
        got = other.topk_batch(Q, k, prune=True)
        for w, g in zip(want, got):
            same(w, g)
        ps = other.prune_stats()
        assert ps["shadow"] == "current" and ps["queries"] == nq and ps["shadow_bytes"] == n * (dim + 8), ps
    finally:
        other.close()
        ref.close()


def test_fallbacks(six):
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    n, dim, k = N_RESULT, 512, 100
    idx = DeviceIndex.synthetic(n, dim, seed=33)
    ref = DeviceIndex.synthetic(n, dim, seed=33)
    try:
        r2i = (np.arange(n, dtype=np.int64) // 3).astype(np.int32)
        idx.set_row2image(r2i)
        ref.set_row2image(r2i)
        n_img = idx.n_images
        # a non-finite query: refused with the plain batch's error before any shadow is built
        Q = batch_queries(5, seed=98)
        bad = Q.copy()
        bad[3, 7] = np.nan
        for prune in (False, True):
            with pytest.raises(_lib.SeesawHipError, match="non-finite") as err:
                idx.topk_batch(bad, 10, prune=prune)
            assert err.value.status == _lib.SSW_ERR_NUMERIC
        ps = idx.prune_stats()
        assert ps["shadow"] == "none" and ps["queries"] == 0 and ps["shadow_bytes"] == 0, ps
        # a refused shadow (the reserve above the card's memory): the plain batch's bits, nothing counted
        want = unpruned(six, lambda: ref.topk_batch(Q, k))
        mode(six, True, 1, reserve=1 << 50)
        got = idx.topk_batch(Q, k, prune=True)
        for w, g in zip(want, got):
            same(w, g)
        ps = idx.prune_stats()
        assert ps["queries"] == 0 and ps["shadow_bytes"] == 0 and ps["shadow"] == "refused", ps
        mode(six, True, 1)
        upload(idx, 0, idx.download(0, 1))  # the same rows again: a refusal is retried once the rows change
        # fewer images left than k for one query only: its slot takes the full scan into its slab
        rng = np.random.default_rng(4)
        keep = rng.choice(n_img, 40, replace=False)
        ex = [None, None, np.setdiff1d(np.arange(n_img), keep), rng.choice(n_img, 9, replace=False), None]
        want = unpruned(six, lambda: ref.topk_batch(Q, k, excluded=ex))
        before = stats(idx)
        got = idx.topk_batch(Q, k, excluded=ex, prune=True)
        st = stats(idx)
        for w, g in zip(want, got):
            same(w, g)
        assert len(got[2][0]) == 40 and st[4] - before[4] == 1 and st[3] - before[3] == 5, (before, st)
        assert st[0] == 1 and st[5] == bytes6(n, dim), st
        # queries that cannot be bounded among ordinary ones: they alone take the full scan
        Qf = batch_queries(7, seed=99)
        Qf[1] = 0.0
        Qf[4] = flagged_queries(dim)[3]
        want = unpruned(six, lambda: ref.topk_batch(Qf, k))
        before = stats(idx)
        got = idx.topk_batch(Qf, k, prune=True)
        st = stats(idx)
        for w, g in zip(want, got):
            same(w, g)
        assert st[3] - before[3] == 7 and st[4] - before[4] == 2, (before, st)
        # the device path: the same slot is flagged with the value 2 in its message, the others are the plain call's
        k_max = 128
        dev = torch.device("cuda", 0)
        blocks = {}
        for name, h in (("plain", ref), ("pruned", idx)):
            blk = torch.full((8, 2 * k_max + 1), -1, dtype=torch.int64, device=dev)
            h.set_exchange_target_batch(blk.data_ptr(), 8, k_max, True)

            def run():
                h.topk_batch_dev(Q, k, excluded=ex, prune=name == "pruned")
                h.sync()
                return blk.cpu().numpy()
            blocks[name] = unpruned(six, run) if name == "plain" else run()
            if name == "pruned":
                surv, why = h.prune_batch_dev_counts()
                assert why.tolist() == [0, 0, 1, 0, 0], (surv, why)
            h.set_exchange_target_batch(0, 0, 0, False)
        flags = blocks["pruned"][:5, -1] >> 32
        assert flags.tolist() == [0, 0, 2, 0, 0] and (blocks["plain"][:5, -1] >> 32 == 0).all(), flags
        ok = [0, 1, 3, 4]
        assert np.array_equal(blocks["pruned"][ok], blocks["plain"][ok])
        assert stats(idx)[5] == bytes6(n, dim)
    finally:
        idx.close()
        ref.close()


def test_product_thresholds(lab_build):
    """the product's own constants on float16 rows filled on the device: at 25 M rows a pruned batch runs on the 6-bit
    shadow and builds no other; at 2^24 rows, where single queries already scan the 6-bit shadow, it still builds and
    scans the int8 one"""
    from seesaw_amd.device_index import DeviceIndex
    mode(lab_build, True)
    mode6(True, -1)
    Q = batch_queries(16, seed=3)
    for n, six_bytes in ((25_000_000, True), (1 << 24, False)):
        idx = DeviceIndex.synthetic(n, 512, seed=7, dtype=np.float16)
        try:
            plain = idx.topk_batch(Q, 100)
            assert stats(idx)[3] == 0
            got = idx.topk_batch(Q, 100, prune=True)
            for a, b in zip(plain, got):
                same(a, b)
            st = stats(idx)
            assert st[3] == 16 and st[4] == 0 and 100 <= st[2] < (1 << 18), st
            assert st[5] == (bytes6(n, 512) if six_bytes else n * (512 + 8)), (n, st)
            # word 0 is the state of the shadow SINGLE queries scan, the 6-bit one at both sizes: the batch at 2^24 rows
            # built the int8 shadow and left that one unbuilt
            assert st[0] == (1 if six_bytes else 0), (n, st)
        finally:
            idx.close()
