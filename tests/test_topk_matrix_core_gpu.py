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


# ---- end-to-end edges: groups, forced fallbacks, small indexes, the workspace, stale row statistics ----------------------
# (the overflow branch needs the strip order and lives in tests/test_topk_mc_certificate_gpu.py)
import _mc_helpers as mc  # noqa: E402


def _oracle_topk(oracle, Xs, q, k, r2i=None, excluded=None):
    """lexsort((rows, -scan scores)) in the device's total order of f32, then the first row of each image, exclusions"""
    s = oracle.scores_kernel_order(Xs, q)
    u = s.view(np.uint32)
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.int64)
    order = np.lexsort((np.arange(s.shape[0]), -o))
    img = order if r2i is None else np.asarray(r2i)[order]
    first = np.sort(np.unique(img, return_index=True)[1])
    rows, imgs = order[first], img[first]
    if excluded is not None and len(excluded):
        keep = ~np.isin(imgs, np.asarray(excluded))
        rows, imgs = rows[keep], imgs[keep]
    return imgs[:k], s[rows[:k]], rows[:k]


def _same_as_loop_and_oracle(dev, oracle, Xs, Q, k, r2i=None, excluded=None):
    got = _same_as_loop(dev, Q, k, excluded)
    for b, (im, sc, rw) in enumerate(got):
        o_im, o_sc, o_rw = _oracle_topk(oracle, Xs, Q[b], k, r2i, None if excluded is None else excluded[b])
        assert np.array_equal(im, o_im) and np.array_equal(rw, o_rw) and np.array_equal(bits(sc), bits(o_sc)), b
    return got


@pytest.mark.parametrize("nq", [1024, 1025, 1300])
def test_groups(oracle, nq):
    """a second group of queries (q0 = 1024): its exclusion offsets re-based, its results and its fallbacks at q0 + b.
    One query of each group with more than one query is 2^-30 of the group's largest: E >= 1.6e-5 maxnorm maxabs_q is
    then above any score it can have, |s| <= maxnorm |q|, and b is such a score (300 rows > M), so it is not proven"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim, k = 300, 256, 10
    rng = np.random.default_rng(nq)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    tiny = [7] + ([1100] if nq > 1025 else [])
    for t in tiny:
        Q[t] *= np.float32(2.0 ** -30)
    excluded = [rng.choice(n, size=int(rng.integers(0, 9)), replace=False) for _ in range(nq)]
    excluded[0], excluded[1], excluded[2] = None, [], np.arange(40)
    if nq > 1024:
        excluded[1024] = np.arange(5, 60)
        if nq > 1026:
            excluded[1025], excluded[1026] = None, []
    dev = DeviceIndex.from_numpy(X)
    _same_as_loop_and_oracle(dev, oracle, X, Q, k, None, excluded)
    st = dev.matrix_core_stats()
    groups = -(-nq // 1024)
    assert st["queries"] == nq and st["strips"] == groups * 3 and st["diverted_calls"] == 0
    assert st["proven"] + st["uncertified"] + st["overflowed"] == nq and st["overflowed"] == 0
    assert st["uncertified"] >= len(tiny) and st["proven"] >= nq - nq // 16
    dev.close()


def test_must_fall_back(oracle):
    """four cases in which no list of M = 64 candidates can prove a top 10, so `uncertified` counts every query"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim, k, nq = 2000, 256, 10, 17
    rng = np.random.default_rng(8)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = _queries(nq, dim)

    def all_uncertified(dev, Xs, Qs, r2i=None, excluded=None):
        got = _same_as_loop_and_oracle(dev, oracle, Xs, Qs, k, r2i, excluded)
        st = dev.matrix_core_stats()
        assert st["uncertified"] == Qs.shape[0] and st["proven"] == 0 and st["overflowed"] == 0, st
        dev.close()
        return got

    # more than M identical best rows, 20 rows apart (16 strips), each in an image of its own: s_k == b
    best = (X[0] * np.float32(3)).copy()
    Xd = X.copy()
    Xd[10::20] = best
    Qd = (best + np.float32(0.02) * Q).astype(np.float32)
    r2i = np.arange(n) // 2
    got = all_uncertified(DeviceIndex.from_numpy(Xd, row2image=r2i), Xd, Qd, r2i)
    assert all(np.array_equal(rw, 10 + 20 * np.arange(k)) for _, _, rw in got)  # the lowest of the tied rows
    # exclusions that remove the best M rows (the fp16 path's M hold at most a few others)
    dev = DeviceIndex.from_numpy(X)
    excluded = [dev.topk(q, 64)[0] for q in Q]
    all_uncertified(dev, X, Q, None, excluded)
    # an image map of 8 images: the M candidates, and the index, hold fewer than k images
    r2i = np.arange(n) // 250
    got = all_uncertified(DeviceIndex.from_numpy(X, row2image=r2i), X, Q, r2i)
    assert all(im.shape[0] == 8 for im, _, _ in got)


@pytest.mark.parametrize("which,low", [("rows", True), ("rows", False), ("queries", True), ("queries", False)])
def test_magnitudes_outside_the_bound_divert(oracle, which, low):
    """the largest |element| of the rows or of the queries one f32 step outside [2^-40, 2^40]: no bound, the plain batch
    answers every query and `uncertified` counts them; exactly 2^-40 and 2^40 are bounded (the certificate tests)"""
    from seesaw_amd.device_index import DeviceIndex
    n, nq, dim, k = 129, 17, 256, 10
    X, Q = mc.outside(which, low, n, nq, dim, np.random.default_rng(1))
    dev = DeviceIndex.from_numpy(X)
    _same_as_loop_and_oracle(dev, oracle, X, Q, k)
    st = dev.matrix_core_stats()
    assert st["uncertified"] == nq and st["proven"] == 0 and st["strips"] == 0 and st["diverted_calls"] == 0, st
    dev.close()


@pytest.mark.parametrize("family", mc.FAMILIES, ids=lambda f: f.__name__)
def test_families_end_to_end(oracle, family):
    """the input families of the certificate tests through the product call: whatever is proven and whatever falls back,
    the answer is `topk`'s"""
    from seesaw_amd.device_index import DeviceIndex
    n, nq, dim, k = 3968, 129, 256, 10
    for dtype in (np.float32, np.float16):
        if family in mc.F32_ONLY and dtype == np.float16:
            continue
        X, Xs, Q = mc.make(family, n, nq, dim, dtype)
        dev = DeviceIndex.from_numpy(X, dtype=dtype)
        _same_as_loop_and_oracle(dev, oracle, Xs, Q, k)
        st = dev.matrix_core_stats()
        assert st["proven"] + st["uncertified"] == nq and st["overflowed"] == 0, st
        dev.close()


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65])
def test_small_indexes(oracle, n):
    """n < k, n < M, n == M, n == M + 1 (k = 16: M = 64), with and without an image map; counts below k are topk's"""
    from seesaw_amd.device_index import DeviceIndex
    dim, nq = 256, 17
    X = oracle.synth_rows(n, 0, n, dim)
    Q = _queries(nq, dim, seed=n)
    for r2i in (None, np.arange(n) // 3):
        for dtype in (np.float32, np.float16):
            dev = DeviceIndex.from_numpy(X, row2image=r2i, dtype=dtype)
            for k in (1, 16, 100, 128):
                got = _same_as_loop_and_oracle(dev, oracle, mc.stored(X, dtype), Q, k, r2i)
                assert all(im.shape[0] == min(k, dev.n_images) for im, _, _ in got)
            st = dev.matrix_core_stats()
            assert st["proven"] + st["uncertified"] == st["queries"] == 4 * nq and st["overflowed"] == 0
            if n < 64:  # fewer rows than the smallest M: no threshold is ever raised, the list holds the index
                assert st["proven"] == 4 * nq
            dev.close()


def test_workspace_regrows(oracle):
    """one handle through calls whose group, k and exclusion block grow and shrink: (nq, k) = (17, 10), (300, 10),
    (17, 128), (1025, 128), (1, 1); the upload block passes 64 KiB at the second"""
    from seesaw_amd.device_index import DeviceIndex
    n, dim = 4097, 256
    X = oracle.synth_rows(2, 0, n, dim)
    dev = DeviceIndex.from_numpy(X)
    rng = np.random.default_rng(6)
    total = 0
    for nq, k in ((17, 10), (300, 10), (17, 128), (1025, 128), (1, 1)):
        Q = _queries(nq, dim, seed=nq + k)
        excluded = [rng.choice(n, size=30, replace=False) for _ in range(nq)]
        _same_as_loop_and_oracle(dev, oracle, X, Q, k, None, excluded)
        total += nq
        st = dev.matrix_core_stats()
        assert st["queries"] == total == st["proven"] + st["uncertified"] and st["overflowed"] == 0
    dev.close()


def _proves_new_rows(dev, oracle, Xs, Q, k, before):
    """after the rows changed to Xs (1000 x the old scale): results on the new rows, and proven with the new scale -- with
    the old one every product would overflow fp16 and nobody be proven"""
    _same_as_loop_and_oracle(dev, oracle, Xs, Q, k)
    after = dev.matrix_core_stats()
    assert after["proven"] - before["proven"] >= Q.shape[0] - 1 and after["overflowed"] == 0, (before, after)


def test_stale_row_statistics_after_every_mutator(oracle):
    import ctypes
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex, _ptr
    from seesaw_amd.sharded import _DevArray
    n, dim, k = 1000, 256, 10
    Q = _queries(17, dim)
    small = np.ascontiguousarray(oracle.synth_rows(9, 0, n, dim) * np.float32(1e-3))

    def primed(dtype=np.float32, rows=n):
        dev = DeviceIndex.from_numpy(small[:rows], dtype=dtype)
        dev.topk_batch(Q, k, matrix_core=True)  # the statistics of the small rows are cached now
        return dev, dev.matrix_core_stats()

    # ssw_index_upload_f16
    dev, before = primed(np.float16)
    X2 = (small * np.float32(1e3)).astype(np.float16)
    _lib.call("ssw_index_upload_f16", dev._h, _ptr(X2), 0, n)
    _proves_new_rows(dev, oracle, X2.astype(np.float32), Q, k, before)
    dev.close()
    # ssw_index_fill_random: unit rows
    dev, before = primed()
    _lib.call("ssw_index_fill_random", dev._h, ctypes.c_uint64(4), 0)
    _proves_new_rows(dev, oracle, oracle.synth_rows(4, 0, n, dim), Q, k, before)
    dev.close()
    # ssw_index_coarse_mean as destination: unit rows, one per image of the source
    src = DeviceIndex.from_numpy(oracle.synth_rows(5, 0, 4 * 250, dim), row2image=np.arange(4 * 250) // 4)
    dev, before = primed(rows=250)
    keep, pos = np.ones(4 * 250, dtype=np.uint8), np.arange(250, dtype=np.int64)
    _lib.call("ssw_index_coarse_mean", src._h, _ptr(keep), _ptr(pos), 250, dev._h)
    _proves_new_rows(dev, oracle, dev.download(), Q, k, before)
    dev.close()
    src.close()
    # ssw_index_device_ptrs: the rows escaped, overwritten behind the library's back
    dev, before = primed()
    vec_ptr, _ = dev.device_ptrs()
    X3 = np.ascontiguousarray(oracle.synth_rows(6, 0, n, dim))
    Xd = torch.as_tensor(_DevArray(vec_ptr, (n, dim), "<f4"), device=torch.device("cuda", 0))
    Xd.copy_(torch.from_numpy(X3))
    torch.cuda.synchronize()
    del Xd
    _proves_new_rows(dev, oracle, X3, Q, k, before)
    dev.close()
    # a partial upload: one row that raises maxabs a thousandfold
    dev, before = primed()
    X4 = small.copy()
    X4[n // 2] = oracle.synth_rows(7, 0, 1, dim)[0]
    _lib.call("ssw_index_upload", dev._h, _ptr(np.ascontiguousarray(X4[n // 2:n // 2 + 1])), n // 2, 1)
    _same_as_loop_and_oracle(dev, oracle, X4, Q, k)
    assert dev.matrix_core_stats()["overflowed"] == 0
    dev.close()
