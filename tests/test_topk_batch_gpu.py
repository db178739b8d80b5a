"""GPU: the batched scan and the batched exact top-k (ssw_index_scan_batch / ssw_index_topk_batch, csrc/scan.hip:
batch_scores_kernel) return, query by query, the BITS of the single-query path -- scores against `scores` and the
kernel-order oracle, selections against `topk` on a second handle over the same rows -- and leave the handle in the
state the last query's `topk` leaves.  Every comparison is exact."""
import numpy as np
import pytest

from _prune_helpers import mode, same, stats

pytestmark = pytest.mark.gpu

F16 = np.float16
NQS = (1, 2, 3, 5, 8, 9, 17)
SHAPES = [(1, 512), (63, 512), (64, 512), (65, 512), (14417, 512), (65535, 512), (65536, 512), ((1 << 20) + 17, 512),
          (70000, 256), (70000, 768), (70000, 1024)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def widen(X):
    return np.asarray(X).astype(np.float16).astype(np.float32)


def hard_rows(oracle, n, dim, seed):
    """as in tests/test_index_f16_gpu.py: unit rows scaled to general magnitudes, with elements in the f16 subnormal
    range and exact round-to-nearest-even ties"""
    rng = np.random.default_rng(seed)
    X = oracle.synth_rows(seed, 0, n, dim) * rng.uniform(0.25, 40.0, size=(n, 1)).astype(np.float32)
    m = rng.random(X.shape)
    X[m < 0.05] = (rng.standard_normal(int((m < 0.05).sum())) * 3e-6).astype(np.float32)  # subnormal in f16
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 2.0 ** -25, 3 * 2.0 ** -25,
                     -5 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, 0.5 + 2.0 ** -12], dtype=np.float32)
    sel = (m >= 0.05) & (m < 0.08)
    X[sel] = ties[rng.integers(0, ties.shape[0], int(sel.sum()))]
    return np.ascontiguousarray(X, dtype=np.float32)


def queries(oracle, nq, dim=512, first=0):
    return np.stack([oracle.synth_query(first + i, dim) * np.float32(1.0 + 0.1 * i) for i in range(nq)])


@pytest.fixture(scope="module")
def DeviceIndex():
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex


@pytest.mark.parametrize("dtype", [np.float32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n,dim", SHAPES)
def test_scores_batch_is_scores_per_query_and_the_oracle(DeviceIndex, oracle, n, dim, dtype):
    X = hard_rows(oracle, n, dim, seed=n % 1000 + dim)
    rows = widen(X) if dtype == F16 else X  # the rows the index holds, as f32
    idx = DeviceIndex.from_numpy(X, dtype=dtype)
    try:
        Q = queries(oracle, max(NQS), dim)
        single = np.stack([idx.scores(q) for q in Q])
        for b, q in enumerate(Q):
            assert np.array_equal(bits(single[b]), bits(oracle.scores_kernel_order(rows, q))), (n, dim, b)
        for nq in NQS:
            got = idx.scores_batch(Q[:nq])
            assert got.shape == (nq, n) and got.dtype == np.float32
            assert np.array_equal(bits(got), bits(single[:nq])), (n, dim, nq)
            # the resident scores are the last query's
            probe = np.unique(np.random.default_rng(nq).integers(0, n, 50))
            assert np.array_equal(bits(idx.gather_scores(probe)), bits(single[nq - 1][probe]))
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", [np.float32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("blocks_per_cu", [1, 2])
def test_every_kernel_width_writes_the_same_bits(lab_build, DeviceIndex, oracle, dtype, blocks_per_cu):
    """the lab build's widths 2, 4, 8 and 16 (ssw_tune_scan_batch), on which the width sweep rests, against the
    single-query scan and the oracle; a row count that ends inside a 64-row batch"""
    from seesaw_amd import _lib
    n = 200_000 + 37
    X = hard_rows(oracle, n, 512, seed=77)
    rows = widen(X) if dtype == F16 else X
    idx = DeviceIndex.from_numpy(X, dtype=dtype)
    try:
        Q = queries(oracle, 19)
        _lib.call("ssw_tune_scan_batch", 1, -1)
        single = idx.scores_batch(Q)
        for b in (0, 7, 18):
            assert np.array_equal(bits(single[b]), bits(oracle.scores_kernel_order(rows, Q[b])))
        for width in (2, 4, 8, 16):
            _lib.call("ssw_tune_scan_batch", width, blocks_per_cu)
            idx.profile(True)
            got = idx.scores_batch(Q)
            launches = idx.profile_read().shape[0]
            idx.profile(False)
            assert np.array_equal(bits(got), bits(single)), width
            # 19 queries: chunks of `width`, then the narrower forms, one event pair per launch
            assert launches == 19 // width + bin(19 % width).count("1"), (width, launches)
    finally:
        _lib.call("ssw_tune_scan_batch", -1, -1)
        idx.close()


def ragged(n_images, lo, hi, seed):
    counts = np.random.default_rng(seed).integers(lo, hi, size=n_images)
    return np.repeat(np.arange(n_images), counts).astype(np.int32)


def same_results(batch, singles):
    assert len(batch) == len(singles)
    for got, ref in zip(batch, singles):
        same(ref, got)


@pytest.mark.parametrize("dtype", [np.float32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("k", [1, 100, 4096])
def test_topk_batch_is_topk_per_query(DeviceIndex, oracle, dtype, k):
    n_images = 20000
    row2image = ragged(n_images, 1, 9, seed=3)  # ~90 000 rows: the multi-query kernel's range
    assert row2image.shape[0] >= 65536
    X = hard_rows(oracle, row2image.shape[0], 512, seed=21)
    a = DeviceIndex.from_numpy(X, row2image=row2image, dtype=dtype)
    b = DeviceIndex.from_numpy(X, row2image=row2image, dtype=dtype)
    try:
        rng = np.random.default_rng(k)
        for nq in (2, 5, 8, 11):
            Q = queries(oracle, nq, first=nq)
            keep = rng.choice(n_images, 37, replace=False)
            pool = [[], None, [5, 5, 5, 9, 5, 9], rng.integers(0, n_images, 3000).tolist(),
                    np.setdiff1d(np.arange(n_images), keep)]  # the last leaves 37 images: count < k for k >= 100
            excluded = [pool[(i + 4) % len(pool)] for i in range(nq)]  # query 0 gets the last list
            singles = [b.topk(Q[i], k, excluded=excluded[i]) for i in range(nq)]
            same_results(a.topk_batch(Q, k, excluded=excluded), singles)
            if k > 37:
                assert any(len(s[0]) == 37 for s in singles)
        same_results(a.topk_batch(Q, k), [b.topk(q, k) for q in Q])  # excluded=None
    finally:
        a.close()
        b.close()


def test_mass_ties_in_the_middle_of_a_batch(DeviceIndex, oracle):
    """30 000 copies of one row: the fast selection overflows for the query they tie on and the deep path runs, between
    queries that take the fast path"""
    n = 70000
    X = oracle.synth_rows(5, 0, n, 512)
    base = oracle.synth_rows(1, 0, 1, 512)[0]
    X[20000:50000] = base[None, :] * np.float32(0.5)
    pos = 20000 + np.arange(20) * 1000 + 7
    X[pos] = base[None, :] * np.linspace(0.6, 0.9, 20, dtype=np.float32)[:, None]
    a, b = DeviceIndex.from_numpy(X), DeviceIndex.from_numpy(X)
    try:
        Q = queries(oracle, 5)
        Q[2] = base
        for k in (10, 21, 100, 4096):
            singles = [b.topk(q, k) for q in Q]
            assert singles[2][0][:20].tolist() == pos[::-1][:min(k, 20)].tolist()
            same_results(a.topk_batch(Q, k), singles)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("nq", [3, 8, 9])
def test_state_after_the_batch_is_the_last_querys(DeviceIndex, oracle, nq):
    row2image = ragged(15000, 1, 12, seed=8)
    X = hard_rows(oracle, row2image.shape[0], 512, seed=5)
    a = DeviceIndex.from_numpy(X, row2image=row2image)
    b = DeviceIndex.from_numpy(X, row2image=row2image)
    try:
        Q = queries(oracle, nq)
        excluded = [list(range(i, 400, 7)) for i in range(nq)]
        res = a.topk_batch(Q, 50, excluded=excluded)
        last = b.topk(Q[-1], 50, excluded=excluded[-1])
        same(last, res[-1])
        same(last, a.topk(None, 50, excluded=excluded[-1]))
        same(b.topk(None, 200, excluded=[1, 2]), a.topk(None, 200, excluded=[1, 2]))
        probe = np.arange(0, X.shape[0], 97)
        assert np.array_equal(bits(a.gather_scores(probe)), bits(b.scores(Q[-1])[probe]))
    finally:
        a.close()
        b.close()


def test_batch_between_pruned_calls_leaves_the_prune_counters_alone(lab_build, DeviceIndex, oracle):
    n = 300_000
    idx = DeviceIndex.synthetic(n, 512, seed=13)
    try:
        idx.set_row2image((np.arange(n) // 3).astype(np.int32))
        Q = queries(oracle, 5)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        ex = [None, [0, 1, 2], None, list(range(50)), [7]]
        mode(lab_build, False)
        ref = [idx.topk(Q[i], 100, excluded=ex[i]) for i in range(5)]
        mode(lab_build, True, min_rows=1 << 16)
        assert stats(idx)[1] == 1  # the next top-k with a query is pruned
        same(ref[0], idx.topk(Q[0], 100, excluded=ex[0]))
        st = stats(idx)
        assert st[3] == 1 and st[2] >= 100, st  # pruned, and the score buffer is partial now
        same_results(idx.topk_batch(Q, 100, excluded=ex), ref)
        after = stats(idx)
        assert after[3] == st[3] and after[4] == st[4] and after[2] == st[2], (st, after)
        same(ref[4], idx.topk(None, 100, excluded=ex[4]))  # complete scores of the last query
        same(ref[1], idx.topk(Q[1], 100, excluded=ex[1]))
        assert stats(idx)[3] == st[3] + 1
        same_results(idx.topk_batch(Q[:2], 100, excluded=ex[:2]), ref[:2])  # on a partial buffer again
        assert stats(idx)[3] == st[3] + 1
        same_results(idx.topk_batch(Q[:1], 100, excluded=ex[:1]), ref[:1])  # nq == 1 is the single call: pruned
        assert stats(idx)[3] == st[3] + 2
    finally:
        mode(lab_build, True)
        idx.close()


def test_nan_in_one_query_names_it_and_touches_nothing(DeviceIndex, oracle):
    from seesaw_amd import _lib
    X = hard_rows(oracle, 70000, 512, seed=2)
    idx = DeviceIndex.from_numpy(X)
    try:
        Q = queries(oracle, 5)
        first = idx.topk(Q[0], 30, excluded=[3])
        Q[3, 17] = np.nan
        with pytest.raises(_lib.SeesawHipError) as e:
            idx.topk_batch(Q, 30)
        assert e.value.status == _lib.SSW_ERR_NUMERIC
        assert "query 3" in str(e.value) and "17" in str(e.value)
        with pytest.raises(_lib.SeesawHipError, match="query 3"):
            idx.scores_batch(Q)
        same(first, idx.topk(None, 30, excluded=[3]))
        with pytest.raises(_lib.SeesawHipError):  # an excluded id out of range, also before anything runs
            idx.topk_batch(Q[:2], 30, excluded=[[1], [70000]])
        same(first, idx.topk(None, 30, excluded=[3]))
    finally:
        idx.close()


@pytest.mark.parametrize("vector_dtype", ["float32", "float16"])
def test_index_layers_equal_loops_of_query(oracle, vector_dtype):
    import pandas as pd
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.coarse.coarse_index import CoarseIndex
    from seesaw_amd.vector_index import VectorIndex
    n = 70000
    X = hard_rows(oracle, n, 512, seed=31)
    Q = queries(oracle, 6)
    vi = VectorIndex(vectors=X, vector_dtype=vector_dtype)
    got = vi.query_batch(Q, 25)
    for (ids, sc), q in zip(got, Q):
        r_ids, r_sc = vi.query(q, 25)
        assert np.array_equal(ids, r_ids) and np.array_equal(bits(sc), bits(r_sc))
    dbidx = np.sort(np.random.default_rng(0).choice(10 * n, n, replace=False)).astype(np.int64)
    ci = CoarseIndex(embedding=None, vectors=X, vector_meta=pd.DataFrame({"dbidx": dbidx}), vector_dtype=vector_dtype)
    excludes = [None, BitMap(dbidx[:100].tolist()), BitMap(), BitMap(dbidx[5::2].tolist()), None,
                BitMap(dbidx[:-3].tolist())]  # the last leaves 3 images
    vectors = [q for q in Q]
    got = ci.query_batch(topk=40, vectors=vectors + [None], excludes=excludes + [None])
    assert len(got) == 7 and got[6]["dbidxs"].shape[0] == 40  # the random-order entry went through query
    for g, q, e in zip(got, vectors, excludes):
        r = ci.query(topk=40, vector=q, exclude=e)
        assert np.array_equal(g["dbidxs"], r["dbidxs"]) and g["nextstartk"] == r["nextstartk"]
        assert g["activations"].records() == r["activations"].records()
    assert got[5]["dbidxs"].shape[0] == 3


def test_eight_queries_over_twelve_million_rows(DeviceIndex, oracle):
    idx = DeviceIndex.synthetic(12_500_000, 512, seed=77)
    try:
        Q = queries(oracle, 8, first=40)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        batch = idx.topk_batch(Q, 100)
        singles = [idx.topk(q, 100) for q in Q]
        same_results(batch, singles)
        assert all(len(s[0]) == 100 for s in singles)
    finally:
        idx.close()
