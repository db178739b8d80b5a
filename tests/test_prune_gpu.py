"""GPU: the pruned top-k (int8 shadow pre-scan + exact rescoring of the survivors, csrc/prune.hip) returns the bits of
the full f32 scan -- images, scores and best rows -- and leaves a score buffer that every consumer sees complete.
Every case runs the same calls with pruning forced off (ssw_tune_prune(0), what SSW_TOPK_FULL_SCAN does) and on."""
import ctypes

import numpy as np
import pytest

from _prune_helpers import both, mode, query, same, stats

pytestmark = pytest.mark.gpu

MIN_ROWS = 1 << 22


@pytest.mark.parametrize("log_rows", [22, 23, 25])
def test_synthetic_topk_is_the_full_scan(lab_build, log_rows):
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(1 << log_rows, 512, seed=7)
    try:
        for i, k in enumerate((1, 100, 1024)):
            q = query(100 + i)
            full, got, st = both(lab_build, idx, lambda: idx.topk(q, k))
            same(full, got)
            assert len(got[0]) == k
            assert st[0] == 1 and st[2] >= k, st  # the shadow is current and this call was pruned
            assert st[2] < (1 << 18)
    finally:
        idx.close()


def test_hundred_million_rows(lab_build):
    """the headline shape: every row of a 100 M-row shadow is built and bounded (a grid over all rows would pass 2^32
    threads)"""
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(100_000_000, 512, seed=2024)
    try:
        for i in (0, 24):
            q = np.random.default_rng(10_000 + i).standard_normal(512).astype(np.float32)
            q = (q / np.linalg.norm(q)).astype(np.float32)
            full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100))
            same(full, got)
            assert st[0] == 1 and 100 <= st[2] < (1 << 18), st
    finally:
        idx.close()


def test_multi_row_images_and_exclusions(lab_build):
    from seesaw_amd.device_index import DeviceIndex
    n = 1 << 22
    idx = DeviceIndex.synthetic(n, 512, seed=3)
    try:
        r2i = (np.arange(n, dtype=np.int64) // 3).astype(np.int32)
        idx.set_row2image(r2i)
        q = query(5)
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert st[2] >= 100
        # the best images excluded, then all but a few hundred
        ex = full[0][:50]
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100, excluded=ex))
        same(full, got)
        keep = np.random.default_rng(0).choice(idx.n_images, 300, replace=False)
        mostly = np.setdiff1d(np.arange(idx.n_images), keep)
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100, excluded=mostly))
        same(full, got)
        assert set(got[0].tolist()) <= set(keep.tolist())
        # fewer images left than k: the threshold selection returns fewer than k keys and the full scan runs
        few = np.setdiff1d(np.arange(idx.n_images), keep[:40])
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100, excluded=few))
        same(full, got)
        assert len(got[0]) == 40 and st[2] == -1
    finally:
        idx.close()


def test_duplicated_rows_and_a_rewritten_row(lab_build):
    """mass ties (one row copied many times: the threshold selection overflows and the call falls back), then a row
    rewritten by upload to become the top hit: the stale shadow must not be used"""
    from seesaw_amd.device_index import DeviceIndex
    n = 1 << 22
    idx = DeviceIndex.synthetic(n, 512, seed=11)
    try:
        q = query(9)
        mode(lab_build, True)
        idx.topk(q, 10)  # builds the shadow
        row = (q * 0.9).astype(np.float32)
        dup = np.repeat(row[None, :], 20000, axis=0)
        from seesaw_amd import _lib
        _lib.call("ssw_index_upload", idx._h, dup.ctypes.data_as(ctypes.c_void_p), 1000, dup.shape[0])
        assert stats(idx)[0] == 2  # stale
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert got[0][0] == 1000 and st[0] == 1
        one = (q * 1.5).astype(np.float32)[None, :]
        _lib.call("ssw_index_upload", idx._h, one.ctypes.data_as(ctypes.c_void_p), n - 5, 1)
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100))
        same(full, got)
        assert got[0][0] == n - 5
    finally:
        idx.close()


def test_loose_bound_overflows_the_survivor_cap(lab_build):
    """every row carries one element far above the rest in a coordinate the query ignores: the int8 step, and with it
    the bound, is wider than the spread of the scores, more rows than the cap survive and the call falls back"""
    from seesaw_amd.device_index import DeviceIndex
    n = 1 << 19
    X = np.random.default_rng(1).standard_normal((n, 512)).astype(np.float32) * np.float32(1 / np.sqrt(512))
    X[:, 0] = 10.0
    idx = DeviceIndex.from_numpy(X)
    del X
    try:
        q = query(2)
        q[0] = 0.0
        full, got, st = both(lab_build, idx, lambda: idx.topk(q, 100), min_rows=1 << 18)
        same(full, got)
        assert st[2] == -1 and st[4] >= 1
    finally:
        idx.close()


def test_consumers_see_the_complete_buffer(lab_build):
    """after a pruned top-k every reader of the score buffer sees the full scan of that query"""
    from seesaw_amd.device_index import DeviceIndex
    import torch
    n = 1 << 22
    idx = DeviceIndex.synthetic(n, 512, seed=21)
    try:
        q = query(31)
        mode(lab_build, False)
        ref_scores = idx.scores(q)
        ref_top = idx.topk(q, 64)
        rows = np.random.default_rng(3).choice(n, 5000, replace=False)
        mode(lab_build, True)
        # topk(None) after a pruned topk
        same(ref_top, idx.topk(q, 64))
        assert stats(idx)[2] >= 64
        same(ref_top, idx.topk(None, 64))
        # gather_scores
        idx.topk(q, 64)
        same([ref_scores[rows]], [idx.gather_scores(rows)])
        # select_deep_dev
        idx.topk(q, 64)
        idx.select_deep_dev(64)
        same(ref_top, idx.topk_fetch(64))
        # ssw_index_scan's copy-out runs its own full scan
        idx.topk(q, 64)
        same([ref_scores], [idx.scores(q)])
        # device_ptrs: the whole buffer (and the shadow ends: the rows escaped)
        idx.topk(q, 64)
        assert stats(idx)[2] >= 64
        _, s_ptr = idx.device_ptrs()
        from seesaw_amd.sharded import _DevArray
        buf = torch.as_tensor(_DevArray(s_ptr, (n,), "<f4"), device="cuda").cpu().numpy()
        same([ref_scores], [buf])
        assert stats(idx)[1] == 0
        same(ref_top, idx.topk(q, 64))
    finally:
        idx.close()


def test_rescore_avg_after_a_pruned_topk(lab_build):
    from seesaw_amd.device_index import DeviceIndex
    n = 1 << 22
    idx = DeviceIndex.synthetic(n, 512, seed=4)
    try:
        r2i = (np.arange(n, dtype=np.int64) // 4).astype(np.int32)
        idx.set_row2image(r2i)
        rng = np.random.default_rng(0)
        boxes = np.tile(np.array([[0, 0, 1, 1], [0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1]], np.float32), (n // 4, 1))
        zoom = np.tile(np.array([0, 1, 1, 1], np.int32), n // 4)
        idx.set_tile_meta(boxes, zoom)
        q = query(8)
        pos = rng.choice(idx.n_images, 200, replace=False)
        mode(lab_build, False)
        idx.topk(q, 100)
        ref = idx.rescore_avg(pos, "greater")
        mode(lab_build, True)
        idx.topk(q, 100)
        assert stats(idx)[2] >= 100
        same(ref, idx.rescore_avg(pos, "greater"))
    finally:
        idx.close()


def test_sharded_exchange_message_is_the_same(lab_build):
    import torch
    from seesaw_amd.sharded import ShardedSyntheticIndex
    n = 1 << 23
    x = ShardedSyntheticIndex(n, 512, 5, 0, 1, 0, k_max=128)
    try:
        qs = torch.from_numpy(np.stack([query(40 + i) for i in range(3)])).cuda()
        for i in range(3):
            msgs = []
            for on in (False, True):
                mode(lab_build, on)
                keys, count = x.topk_async(qs[i].data_ptr(), 100)
                torch.cuda.synchronize()
                msgs.append((keys[:int(count.item())].cpu().numpy().copy(), x.local_count.cpu().numpy().copy()))
            same([msgs[0][0], msgs[0][1]], [msgs[1][0], msgs[1][1]])
            assert stats(x.local)[2] >= 100
        x.xchg.assert_no_overflow_seen()
    finally:
        mode(lab_build, True)
        x.close()


def test_memory_reserve_refusal(lab_build):
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(1 << 22, 512, seed=2)
    try:
        q = query(1)
        mode(lab_build, False)
        full = idx.topk(q, 100)
        mode(lab_build, True, reserve=1 << 60)
        got = idx.topk(q, 100)
        st = stats(idx)
        same(full, got)
        assert st[0] == 3 and st[3] == 0 and st[5] == 0
    finally:
        mode(lab_build, True)
        idx.close()
