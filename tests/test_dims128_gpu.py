"""GPU: index dims that are multiples of 128 -- 384, 640, 896, 1152 (whole 256-element chunks and a HALF one) and 1280
(five whole chunks) -- through the scan family ("Dims that are multiples of 128").

The yardstick of dims 384 / 640 / 896 is the scan that existed before: the scores are, bit for bit, those of today's
dim 512 / 768 / 1024 scan over the rows and the query zero-padded to whole chunks.  Dims 1152 and 1280 have nothing to
pad to and are held to the float64 dot product within the bound of the kernel's own roundings.  Every other path
(batched, view, listed rows) must give `scores`' bits, and the selection is the oracle's over the device's scores."""
import numpy as np
import pytest

from seesaw_amd._lib import SeesawHipError
from seesaw_amd.device_index import DeviceIndex

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
PADDED_DIMS, WIDE_DIMS = (384, 640, 896), (1152, 1280)
SMALL_N, STREAM_N = 4097, 70000  # one n on each side of the small kernels' 65 536 rows
U = 2.0 ** -24                   # unit roundoff of f32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pad(A):  # zero-padded to whole 256-element chunks
    return np.pad(A, [(0, 0)] * (A.ndim - 1) + [(0, -A.shape[-1] % 256)])


def rows_of(n, dim, seed=5):
    """unit Gaussian rows, one of all zeros and one with a negative-zero element (in the half chunk)"""
    X = np.random.default_rng(seed + dim).standard_normal((n, dim)).astype(np.float32)
    X[n // 2] = 0.0
    X[(n - 1) // 3, dim - 3] = -0.0
    return X


def queries_of(nq, dim):
    return np.random.default_rng(dim).standard_normal((nq, dim)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 65, 4097, 65535, 65536, 65537])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", PADDED_DIMS)
def test_scores_are_the_padded_scan_s_bits(dim, dtype, n):
    X, q = rows_of(n, dim), queries_of(1, dim)[0]  # the zero row and the negative zero lie inside every n
    idx, ref = DeviceIndex.from_numpy(X, dtype=dtype), DeviceIndex.from_numpy(pad(X), dtype=dtype)
    try:
        assert np.array_equal(bits(idx.scores(q)), bits(ref.scores(pad(q))))
    finally:
        idx.close()
        ref.close()


@pytest.mark.parametrize("n", [SMALL_N, STREAM_N])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", WIDE_DIMS)
def test_new_widths_within_the_rounding_bound(dim, dtype, n):
    """|score - float64 dot| <= gamma_k sum |x_i q_i| with k = 2 C + 7: the 2 C fmas of a chain, a0 + a1 and the six
    butterfly adds an element's path crosses; C = 5.  For f16 rows the reference takes the rounded rows."""
    X, q = rows_of(n, dim), queries_of(1, dim)[0]
    idx = DeviceIndex.from_numpy(X, dtype=dtype)
    try:
        got = idx.scores(q).astype(np.float64)
    finally:
        idx.close()
    Xr, q64 = X.astype(dtype).astype(np.float64), q.astype(np.float64)
    k = 2 * 5 + 7
    bound = k * U / (1 - k * U) * (np.abs(Xr) @ np.abs(q64))
    err = np.abs(got - Xr @ q64)
    print("dim %d %s n %d: max err / bound = %.3f" % (dim, np.dtype(dtype).name, n, np.max(err[bound > 0] / bound[bound > 0])))
    assert np.all(err <= bound)


@pytest.mark.parametrize("n", [SMALL_N, STREAM_N])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", PADDED_DIMS + WIDE_DIMS)
def test_every_path_gives_one_set_of_bits_and_the_oracle_s_selection(oracle, dim, dtype, n):
    X, Q = rows_of(n, dim), queries_of(17, dim)
    r2i = np.repeat(np.arange(n), 1 + np.arange(n) % 4)[:n].astype(np.int32)  # 1-4 rows an image
    n_images = int(r2i[-1]) + 1
    idx = DeviceIndex.from_numpy(X, row2image=r2i, dtype=dtype)
    # members: every third image (a small view at either n), and all but one image in 32 (a streaming view at STREAM_N)
    views = [idx.view(np.arange(0, n_images, 3)), idx.view(np.flatnonzero(np.arange(n_images) % 32 != 7))]
    try:
        S = np.stack([idx.scores(q) for q in Q])
        for nq in (1, 3, 16, 17):
            assert np.array_equal(bits(idx.scores_batch(Q[:nq])), bits(S[:nq])), nq
        listed = np.random.default_rng(1).integers(0, n, 100)
        assert np.array_equal(bits(idx.score_rows(Q[0], listed)), bits(S[0, listed]))
        idx.scores(Q[1])  # gather_scores reads the resident scores of the last scan
        assert np.array_equal(bits(idx.gather_scores(listed)), bits(S[1, listed]))
        excluded = [0, 5, n_images - 1]
        imgs, scs, best = idx.topk(Q[0], 50, excluded)
        o_imgs, o_scs, o_best = oracle.topk_images_tiebreak(S[0], r2i, n_images, excluded, 50)
        assert np.array_equal(imgs, o_imgs) and np.array_equal(bits(scs), bits(o_scs)) and np.array_equal(best, o_best)
        lists = [[b, 2 * b + 1] for b in range(5)]
        for got, b in zip(idx.topk_batch(Q[:5], 50, lists), range(5)):
            assert all(np.array_equal(g, w) for g, w in zip(got, idx.topk(Q[b], 50, lists[b]))), b
        for v in views:
            assert np.array_equal(bits(v.scores(Q[0])), bits(S[0, v.parent_rows]))
            for nq in (1, 3, 16, 17):
                assert np.array_equal(bits(v.view_scores_batch(Q[:nq])), bits(S[:nq, v.parent_rows])), nq
            for got, b in zip(v.view_topk_batch(Q[:5], 50, lists), range(5)):
                assert all(np.array_equal(g, w) for g, w in zip(got, v.topk(Q[b], 50, lists[b]))), b
    finally:
        for v in views:
            v.close()
        idx.close()


@pytest.mark.parametrize("dim", PADDED_DIMS + WIDE_DIMS)
def test_f16_round_trip_and_gather_rows(dim):
    X = rows_of(300, dim)
    want = X.astype(np.float16).astype(np.float32)
    idx, idx32 = DeviceIndex.from_numpy(X, dtype=F16), DeviceIndex.from_numpy(X)
    try:
        listed = np.array([299, 0, 150, 100, 7])
        assert np.array_equal(bits(idx.download()), bits(want))
        assert np.array_equal(bits(idx.gather_rows(listed)), bits(want[listed]))
        assert np.array_equal(bits(idx32.download()), bits(X)) and np.array_equal(bits(idx32.gather_rows(listed)), bits(X[listed]))
        up = DeviceIndex.from_numpy(X.astype(np.float16), dtype=F16)  # binary16 input goes up as it is
        assert np.array_equal(bits(up.download()), bits(want))
        up.close()
    finally:
        idx.close()
        idx32.close()


@pytest.mark.parametrize("dim", [320, 128, 1408])
def test_other_dims_stay_refused(dim):
    with pytest.raises(SeesawHipError, match=r"status -4: .*dim=%d" % dim):
        DeviceIndex(10, dim)


def views_topk_of(idx, Q, avg=False):
    v = idx.view(np.arange(10))
    try:
        DeviceIndex.views_topk_batch_avg([v], Q[:1], 5, "all") if avg else DeviceIndex.views_topk_batch([v], Q[:1], 5)
    finally:
        v.close()


REFUSED = {  # each raises SSW_ERR_UNSUPPORTED (status -4) with the dim in its text
    "knn": lambda idx, Q: idx.knn(3),
    "synthetic": lambda idx, Q: DeviceIndex.synthetic(100, idx.dim),
    "views_topk_batch": lambda idx, Q: views_topk_of(idx, Q),
    "views_topk_batch_avg": lambda idx, Q: views_topk_of(idx, Q, avg=True),
    "stage2_pair": lambda idx, Q: idx.stage2_pair(Q[:1], Q[1:2], np.zeros((1, 4), np.int64), np.array([4]), "plain_score"),
    "topk_dev": lambda idx, Q: idx.topk_dev(0, 5),
    "topk_batch_dev": lambda idx, Q: idx.topk_batch_dev(Q, 5),
    "topk_batch_dev_pruned": lambda idx, Q: idx.topk_batch_dev(Q, 5, prune=True),
    "stage2_avg_batch_dev": lambda idx, Q: idx.stage2_avg_batch_dev(Q, 0, 0, 8, 5, "all", 0),
    "coarse_mean": lambda idx, Q: idx.coarse_mean(np.ones(idx.n_rows)),
}


@pytest.mark.parametrize("entry", sorted(REFUSED))
def test_entries_outside_the_scan_family_refuse(entry):
    dim = 384
    idx = DeviceIndex.from_numpy(rows_of(200, dim), row2image=np.arange(200) // 2)
    try:
        with pytest.raises(SeesawHipError, match=r"status -4: .*384"):
            REFUSED[entry](idx, queries_of(2, dim))
    finally:
        idx.close()


def test_a_384_dim_index_is_unpruned():
    Q = queries_of(3, 384)
    idx = DeviceIndex.from_numpy(rows_of(200, 384))
    try:
        st = idx.prune_stats()
        assert st["shadow"] == "none" and not st["eligible"] and st["shadow_bytes"] == 0
        for got, want in zip(idx.topk_batch(Q, 10, prune=True), idx.topk_batch(Q, 10)):
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert idx.prune_stats()["queries"] == 0
    finally:
        idx.close()
