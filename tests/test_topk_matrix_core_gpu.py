"""GPU: `DeviceIndex.topk_batch(matrix_core=True)` (ssw_index_topk_batch_mc, index_mc.hip) returns, bit for bit, the
loop of `topk` -- images, score bits and rows -- and its certificate, not its fallback, carries ordinary data."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(oracle, n, dim, dtype, seed=3, row2image=None):
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex.from_numpy(oracle.synth_rows(seed, 0, n, dim), row2image=row2image, dtype=dtype)


def _queries(nq, dim, seed=11):
    return np.random.default_rng(seed).standard_normal((nq, dim)).astype(np.float32)


def _same_as_loop(dev, Q, k, excluded=None):
    got = dev.topk_batch(Q, k, excluded=excluded, matrix_core=True)
    assert len(got) == Q.shape[0]
    for b, (im, sc, rw) in enumerate(got):
        r_im, r_sc, r_rw = dev.topk(Q[b], k, None if excluded is None else excluded[b])
        assert np.array_equal(im, r_im), b
        assert np.array_equal(bits(sc), bits(r_sc)), b
        assert np.array_equal(rw, r_rw), b
    return got


def _sharp(stats, nq):
    """the candidate pass carried the call: (almost) nobody needed the plain batch"""
    assert stats["overflowed"] == 0 and stats["uncertified"] <= max(1, nq // 16), stats
    assert stats["proven"] + stats["uncertified"] == stats["queries"] == nq


@pytest.mark.parametrize("dtype,dim,n,nq,k", [
    (np.float32, 512, 1, 1, 1),
    (np.float16, 256, 63, 17, 10),
    (np.float32, 768, 129, 17, 128),
    (np.float16, 1024, 129, 1, 10),
    (np.float32, 512, 4097, 130, 10),
    (np.float16, 512, 4097, 17, 128),
    (np.float32, 256, 4097, 17, 1),
    (np.float16, 768, 4097, 130, 10),
    (np.float32, 1024, 4097, 17, 10),
    (np.float32, 512, 4224, 17, 10),   # MC_CAP = 4096 rows in the first level + one strip of 128 rows
    (np.float16, 1024, 4160, 17, 10),  # ... + one strip of 64 rows (dims 768 and 1024)
    (np.float16, 256, 4224, 1, 1),
])
def test_shapes(oracle, dtype, dim, n, nq, k):
    dev = _index(oracle, n, dim, dtype)
    _same_as_loop(dev, _queries(nq, dim), k)
    st = dev.matrix_core_stats()
    assert st["calls"] == 1 and st["queries"] == nq and st["diverted_calls"] == 0
    # every row of the first level is appended: 4096 rows, less where the index's short last strip is one of its strips
    assert st["strips"] == -(-n // (128 if dim <= 512 else 64)) and st["appended"] >= min(n, 4096 - 128) * nq
    if n == 4097:
        _sharp(st, nq)
    dev.close()


def test_k_above_128_is_the_plain_batch(oracle):
    dev = _index(oracle, 4097, 512, np.float32)
    _same_as_loop(dev, _queries(17, 512), 129)
    st = dev.matrix_core_stats()
    assert st["diverted_calls"] == 1 and st["calls"] == 1 and st["queries"] == 17 and st["strips"] == 0
    dev.close()


def test_three_levels_against_the_oracle(oracle):
    n, nq, k = 200_000, 130, 10
    X = oracle.synth_rows(5, 0, n, 512)
    from seesaw_amd.device_index import DeviceIndex
    dev = DeviceIndex.from_numpy(X)
    Q = _queries(nq, 512, seed=5)
    got = dev.topk_batch(Q, k, matrix_core=True)
    _sharp(dev.matrix_core_stats(), nq)
    dev.close()
    ids = np.arange(n)
    for b, (im, sc, rw) in enumerate(got):
        s = oracle.scores_kernel_order(X, Q[b])
        order = np.lexsort((ids, -s.astype(np.float64)))[:k]
        assert np.array_equal(im, order) and np.array_equal(rw, order), b
        assert np.array_equal(bits(sc), bits(s[order])), b


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_image_map_and_exclusions(oracle, dtype):
    n, nq, k = 5000, 17, 10
    dev = _index(oracle, n, 512, dtype, row2image=np.arange(n) // 13)
    Q = _queries(nq, 512)
    first = _same_as_loop(dev, Q, k)
    rng = np.random.default_rng(2)
    excluded = [np.concatenate([im[:5], rng.choice(dev.n_images, 20, replace=False)]) for im, _, _ in first]
    excluded[0], excluded[1] = None, []
    got = _same_as_loop(dev, Q, k, excluded)
    assert not set(got[2][0].tolist()) & set(excluded[2].tolist())
    dev.close()


def test_ties_and_clusters(oracle):
    from seesaw_amd.device_index import DeviceIndex
    X = np.load(os.path.join(GOLDEN, "labelprop.npz"))["X"].copy()  # clustered unit rows
    X[100:150] = X[7]  # 51 identical rows: exact score ties, ordered by row
    X = np.concatenate([X, X, X])
    dev = DeviceIndex.from_numpy(X)
    _same_as_loop(dev, X[np.arange(40) * 37], 10)  # fallbacks expected here: any number of them
    dev.close()


def test_refusals_and_state(oracle):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex, _ptr
    n, k = 4097, 10
    dev = _index(oracle, n, 512, np.float32)
    Q = _queries(17, 512)
    view = dev.view(np.arange(100))
    with pytest.raises(_lib.SeesawHipError, match="view") as e:
        view.topk_batch(Q, k, matrix_core=True)
    assert e.value.status == -4
    view.close()
    d384 = _index(oracle, 64, 384, np.float32)
    with pytest.raises(_lib.SeesawHipError, match="384") as e:
        d384.topk_batch(_queries(2, 384), k, matrix_core=True)
    assert e.value.status == -4
    d384.close()
    with pytest.raises(ValueError):
        dev.topk_batch(Q, k, prune=True, matrix_core=True)
    bad = Q.copy()
    bad[3, 5] = np.nan
    with pytest.raises(_lib.SeesawHipError) as e:
        dev.topk_batch(bad, k, matrix_core=True)
    assert e.value.status == -5
    # the handle afterwards: the last query is the resident one
    dev.topk_batch(Q, k, matrix_core=True)
    kept, last = dev.topk(None, k), dev.topk(Q[-1], k)
    assert all(np.array_equal(a, b) for a, b in zip(kept, last))
    # new rows: the cached row statistics go stale with them (these rows are 1000 x larger)
    X2 = np.ascontiguousarray(oracle.synth_rows(9, 0, n, 512) * np.float32(1000.0))
    _lib.call("ssw_index_upload", dev._h, _ptr(X2), 0, n)
    before = dev.matrix_core_stats()
    got = _same_as_loop(dev, Q, k)
    s = oracle.scores_kernel_order(X2, Q[0])
    assert np.array_equal(got[0][0], np.lexsort((np.arange(n), -s.astype(np.float64)))[:k])
    after = dev.matrix_core_stats()  # with the old rows' scale every product would overflow fp16 and nobody be proven
    assert after["proven"] - before["proven"] >= 16 and after["overflowed"] == 0
    dev.close()
