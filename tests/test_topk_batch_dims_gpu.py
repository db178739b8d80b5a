"""GPU: the multi-query scan kernel at dims 256, 768 and 1024 (csrc/scan.hip: batch_scores_kernel at C = 1, 3, 4 and the
width table beside SCAN_BATCH_MAX_F32 / F16).  A batch returns, query by query, the BITS of the single-query path --
scores against `scores` and the kernel-order oracle, selections against `topk` on a second handle -- in fewer scan
launches than queries, through every layer that chunks a batch: DeviceIndex, MultiscaleIndex.query_batch and the
sharded exchange.  Every comparison is exact."""
import numpy as np
import pandas as pd
import pytest

from _batch_dims_helpers import (F16, OneRank, bits, expected_launches, hard_rows, launches_of, queries, ragged, widen)
from _prune_helpers import same

pytestmark = pytest.mark.gpu

DIMS = (256, 768, 1024)
NQS = (2, 3, 5, 8, 9, 17, 19)
# 65 536: the first size served, where the grid is cut to the blocks the rows need; 200 037 ends inside a 64-row batch
# and gives a wave more than one batch at two blocks a CU (3 126 batches over 2 048 waves)
ROWS = (65536, 65537, 65536 + 63, 200_037)
WIDTHS = (2, 4, 8, 16)
DTYPES = pytest.mark.parametrize("dtype", [np.float32, F16], ids=["f32", "f16"])


@pytest.fixture(scope="module")
def DeviceIndex():
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex


@pytest.fixture(scope="module")
def big_rows(oracle):
    """the 200 037 hard rows of each dim, made once: the smaller row counts are their prefixes"""
    cache = {}

    def get(dim):
        if dim not in cache:
            cache[dim] = hard_rows(oracle, max(ROWS), dim, seed=dim)
            cache[dim].setflags(write=False)
        return cache[dim]
    return get


@DTYPES
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_scores_batch_is_scores_per_query_and_the_oracle(DeviceIndex, oracle, big_rows, dim, n, dtype):
    X = big_rows(dim)[:n]
    rows = widen(X) if dtype == F16 else X  # the rows the index holds, as f32
    idx = DeviceIndex.from_numpy(X, dtype=dtype)
    try:
        Q = queries(oracle, max(NQS), dim)
        single = np.stack([idx.scores(q) for q in Q])
        for b in (0, 18):
            assert np.array_equal(bits(single[b]), bits(oracle.scores_kernel_order(rows, Q[b]))), (n, dim, b)
        for nq in NQS:
            got = idx.scores_batch(Q[:nq])
            assert got.shape == (nq, n) and got.dtype == np.float32
            assert np.array_equal(bits(got), bits(single[:nq])), (n, dim, nq)
            # the resident scores are the last query's
            probe = np.unique(np.random.default_rng(nq).integers(0, n, 50))
            assert np.array_equal(bits(idx.gather_scores(probe)), bits(single[nq - 1][probe]))
    finally:
        idx.close()


@DTYPES
@pytest.mark.parametrize("dim", DIMS)
def test_nineteen_queries_are_chunks_of_the_products_width(DeviceIndex, oracle, big_rows, dim, dtype):
    """the product library: 19 queries are 19 // W chunks and one launch per set bit of 19 % W, W the product's width
    for the shape -- not 19 single scans"""
    idx = DeviceIndex.from_numpy(big_rows(dim)[:65536 + 63], dtype=dtype)
    try:
        _, launches = launches_of(idx, lambda: idx.scores_batch(queries(oracle, 19, dim)))
        assert launches in [expected_launches(19, w) for w in WIDTHS], launches
    finally:
        idx.close()


@DTYPES
@pytest.mark.parametrize("blocks_per_cu", [1, 2])
@pytest.mark.parametrize("dim", DIMS)
def test_every_compiled_width_writes_the_same_bits(lab_build, DeviceIndex, oracle, big_rows, dim, dtype, blocks_per_cu):
    """the lab build's widths 2, 4, 8 and 16 (ssw_tune_scan_batch), on which the width sweep rests, against the
    single-query scan; a width above the shape's widest instance is served by that instance, never refused"""
    from seesaw_amd import _lib
    X = big_rows(dim)
    idx = DeviceIndex.from_numpy(X, dtype=dtype)
    try:
        Q = queries(oracle, 19, dim)
        _lib.call("ssw_tune_scan_batch", 1, -1)
        single, launches = launches_of(idx, lambda: idx.scores_batch(Q))
        assert launches == 19
        rows = widen(X) if dtype == F16 else X
        assert np.array_equal(bits(single[7]), bits(oracle.scores_kernel_order(rows, Q[7])))
        _lib.call("ssw_tune_scan_batch", 16, blocks_per_cu)
        _, at16 = launches_of(idx, lambda: idx.scores_batch(Q))
        widest = [w for w in WIDTHS if expected_launches(19, w) == at16]  # (the four counts differ: 10, 7, 4, 3)
        assert len(widest) == 1, at16
        for width in WIDTHS:
            _lib.call("ssw_tune_scan_batch", width, blocks_per_cu)
            got, launches = launches_of(idx, lambda: idx.scores_batch(Q))
            assert np.array_equal(bits(got), bits(single)), width
            assert launches == expected_launches(19, min(width, widest[0])), (width, widest, launches)
    finally:
        _lib.call("ssw_tune_scan_batch", -1, -1)
        idx.close()


@DTYPES
@pytest.mark.parametrize("dim", [768, 1024])
def test_topk_batch_is_topk_per_query(DeviceIndex, oracle, dim, dtype):
    """~70 000 rows under a ragged image map; query 4 of 9 ties on 30 000 rows, so the deep selection runs in the middle
    of a chunk between fast ones; one exclusion list leaves 37 images"""
    n_images = 15500
    row2image = ragged(n_images, 1, 9, seed=3)
    n = row2image.shape[0]
    assert 65536 <= n < 75000
    X = hard_rows(oracle, n, dim, seed=21)
    base = oracle.synth_rows(1, 0, 1, dim)[0]
    X[20000:50000] = base[None, :] * np.float32(0.5)
    a = DeviceIndex.from_numpy(X, row2image=row2image, dtype=dtype)
    b = DeviceIndex.from_numpy(X, row2image=row2image, dtype=dtype)
    try:
        rng = np.random.default_rng(dim)
        Q = queries(oracle, 9, dim, first=9)
        Q[4] = base
        keep = rng.choice(n_images, 37, replace=False)
        pool = [[], None, [5, 5, 5, 9, 5, 9], rng.integers(0, n_images, 3000).tolist(),
                np.setdiff1d(np.arange(n_images), keep)]  # the last leaves 37 images: fewer than k = 100
        excluded = [pool[(i + 4) % len(pool)] for i in range(9)]  # query 0 gets the last list, query 4 excludes nobody
        for k in (1, 100):
            singles = [b.topk(Q[i], k, excluded=excluded[i]) for i in range(9)]
            assert len(singles[0][0]) == min(k, 37)
            got, launches = launches_of(a, lambda: a.topk_batch(Q, k, excluded=excluded))
            assert launches < 9
            assert len(got) == 9
            for g, r in zip(got, singles):
                same(r, g)
            # the state after the batch is the last query's
            same(singles[8], a.topk(None, k, excluded=excluded[8]))
            probe = np.arange(0, n, 97)
            assert np.array_equal(bits(a.gather_scores(probe)), bits(b.scores(Q[8])[probe]))
        for g, r in zip(a.topk_batch(Q[:5], 100), [b.topk(q, 100) for q in Q[:5]]):  # excluded=None
            same(r, g)
    finally:
        a.close()
        b.close()


def test_two_stage_query_batch_at_dim_768(oracle):
    """MultiscaleIndex.query_batch over 66 000 tiles of dim 768 (9 000 images of 3, 7 and 12 overlapping boxes on three
    zoom levels), avg_score on a shortlist of 50: entry by entry the loop of `query`, in fewer scan launches than
    queries"""
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    counts = np.tile([3, 7, 12], 3000)  # 9 000 images, 66 000 tiles
    n = int(counts.sum())
    assert n >= 65536
    image = np.repeat(np.arange(counts.shape[0]), counts)
    within = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
    x1 = (within * 13 % 50).astype(np.float32)
    y1 = (within * 7 % 40).astype(np.float32)
    meta = pd.DataFrame({"dbidx": image.astype(np.int64) * 3 + 1, "zoom_level": (1 << (within % 3)).astype(np.int16),
                         "x1": x1, "y1": y1, "x2": (x1 + 30 + (within % 4) * 10).astype(np.float32),
                         "y2": (y1 + 25 + (within % 5) * 8).astype(np.float32)})
    assert all(meta[c].dtype == np.float32 for c in ("x1", "y1", "x2", "y2"))  # the device second stage needs f32 boxes
    index = MultiscaleIndex(embedding=None, vectors=hard_rows(oracle, n, 768, seed=4), vector_meta=meta)
    try:
        ids = index._dbidx
        vectors = [q for q in queries(oracle, 7, 768)]
        excludes = [None, BitMap(ids[:100].tolist()), BitMap(), BitMap(ids[3:].tolist()), None, None,
                    BitMap(ids[::2].tolist())]  # entry 3 leaves 3 images
        kw = dict(topk=10, shortlist_size=50, agg_method="avg_score", aug_larger="greater", rescore_method=None)
        got, launches = launches_of(index._dev, lambda: index.query_batch(vectors=vectors, excludes=excludes, **kw))
        ref = AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw)
        assert launches < 7, launches
        assert len(got) == len(ref) == 7 and got[3]["dbidxs"].shape[0] == 3 and got[0]["dbidxs"].shape[0] == 10
        for g, r in zip(got, ref):
            assert np.array_equal(g["dbidxs"], r["dbidxs"]) and g["dbidxs"].dtype == r["dbidxs"].dtype
            ga, ra = np.asarray(g["activations"].records()), np.asarray(r["activations"].records())
            assert ga.shape == ra.shape and np.array_equal(ga.view(np.uint64), ra.view(np.uint64))
    finally:
        index._dev.close()


def test_sharded_batch_of_one_rank_at_dim_768(DeviceIndex):
    """ssw_index_topk_batch_dev into a batched exchange target, a world of one: the merged keys are `topk` per query on
    a reference handle, and the shard scanned its rows fewer times than there are queries"""
    from seesaw_amd.device_index import decode_keys
    n, tiles, k, k_max, nq = 66_000, 3, 10, 16, 11
    shard = DeviceIndex.synthetic(n, 768, seed=11, device=0)
    ref = DeviceIndex.synthetic(n, 768, seed=11, device=0)
    try:
        r2i = (np.arange(n) // tiles).astype(np.int32)
        shard.set_row2image(r2i)
        ref.set_row2image(r2i)
        rng = np.random.default_rng(6)
        Q = rng.standard_normal((nq, 768)).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        excluded = [None if b % 3 == 0 else ref.topk(Q[b], 5)[0].tolist() + rng.integers(0, n // tiles, 200).tolist()
                    for b in range(nq)]
        want = [ref.topk(Q[b], k, excluded=excluded[b]) for b in range(nq)]
        rank = OneRank(shard, nq, k_max)
        _, launches = launches_of(shard, lambda: shard.topk_batch_dev(Q, k, excluded=[e or [] for e in excluded],
                                                                      first_slot=0))
        keys, counts, flags = rank.merge(nq, k)
        assert launches < nq, launches
        assert counts.tolist() == [k] * nq and not flags.any()
        for b in range(nq):
            imgs, scores = decode_keys(keys[b][:k])
            assert np.array_equal(imgs, want[b][0]), b
            assert np.array_equal(bits(scores), bits(want[b][1])), b
    finally:
        shard.close()
        ref.close()
