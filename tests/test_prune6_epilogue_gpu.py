"""GPU: the bound of k_q6_bounds (csrc/prune.hip, "6-bit shadow") row by row, on the lab build.  A tile's 16 rows leave
the matrix core spread over the lanes of a wave (lane l holds rows 4 (l >> 4) .. + 3 for column l & 15), and the epilogue
pairs each row's two sums with that row's two constants and its place in the output.  What a change of that lane map can
get wrong and the tests of tests/test_prune6_gpu.py cannot see: a row's bound taken from another row of its tile (so
every row goes through every lane position), a bound that depends on the launch shape, and the I of rows at every count
of groups around a full launch.  Every comparison is bit for bit.

docs/EXPERIMENTS.md, "The 6-bit scan's loads were not non-temporal", lists the six mutations of a one-row-a-lane form of
the epilogue that these tests were run against once (none committed) and which test caught each."""
import numpy as np
import pytest

from _prune6_helpers import hook_bounds6, hook_shadow6, integer_sums, quantise_query
from _prune_batch_helpers import edge_queries
from _prune_helpers import query
from test_prune6_gpu import DIMS, edge_rows, int_rows, shape, six  # noqa: F401  (six: the fixture)

pytestmark = pytest.mark.gpu


def counts(G, W):
    return sorted({1, 15, 16, 17, G - 1, G + 1, W * G - 1, W * G + 1, 2 * W * G + 5, 3 * W * G - G + 3})


def queries(dim):
    return edge_queries(np.random.default_rng(23), dim) + [query(7, dim)]


def tune(blocks=-1, tiles=-1):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune6_scan", blocks, tiles)


def bounds(X, Q):
    """[(I int64 [n], lb f32 [n] as bits)] of the rows X for every query: I and lb of the DEBUG instance, and lb of the
    product's instance of the same launch shape, which must be the same bits"""
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.from_numpy(X)
    try:
        out = []
        for q in Q:
            d = hook_bounds6(idx, q)
            assert not d["bad"]
            lb = d["lb"].view(np.uint32)
            plain = hook_bounds6(idx, q, sums=False)["lb"].view(np.uint32)
            assert np.array_equal(lb, plain), np.argwhere(lb != plain)[:4].ravel()
            out.append((d["I"].copy(), lb.copy()))
        return out
    finally:
        idx.close()


def permutations(n):
    r = np.arange(n)
    return [("shift %d" % s, np.roll(r, s)) for s in (1, 4, 5, 16)] + [("reversed", r[::-1].copy())]


@pytest.mark.parametrize("dim", DIMS)
def test_a_rows_bound_depends_on_the_row_alone(six, dim):
    """I and lb of X and of X with its rows permuted agree row by row: the codes and the constants of a row are the
    builder's of that row alone, and so must be the bound, in whichever lane, tile, group and wave the row lands"""
    G, W = shape(dim)
    Q = queries(dim)
    for n in counts(G, W):
        X = edge_rows(n, dim, seed=n)
        want = bounds(X, Q)
        for name, p in permutations(n):
            if np.array_equal(p, np.arange(n)):
                continue  # a shift by a multiple of n
            got = bounds(np.ascontiguousarray(X[p]), Q)
            for qi, ((I, lb), (Ip, lbp)) in enumerate(zip(want, got)):
                assert np.array_equal(Ip, I[p]), (dim, n, name, qi, np.argwhere(Ip != I[p])[:4].ravel())
                assert np.array_equal(lbp, lb[p]), (dim, n, name, qi, np.argwhere(lbp != lb[p])[:4].ravel())


@pytest.mark.parametrize("dim", DIMS)
def test_the_bound_does_not_depend_on_the_launch_shape(six, dim):
    """blocks a CU in {1, 2, 8} and tiles a request in {1, 2, 4} as far as the dim admits (tiles x dim <= 1024) against
    the default shape.  With W waves and G rows a request of the default shape, 2 W G + 5 and 3 W G - G + 3 end in the
    clamped ragged group of every shape here, and at 8 blocks a CU every n has fewer groups than waves."""
    G, W = shape(dim)
    Q = queries(dim)
    try:
        for n in (17, G + 1, W * G + 1, 2 * W * G + 5, 3 * W * G - G + 3):
            X = edge_rows(n, dim, seed=n)
            tune()
            want = bounds(X, Q)
            for blocks in (1, 2, 8):
                for tiles in (1, 2, 4):
                    if tiles * dim > 1024:
                        continue
                    tune(blocks, tiles)
                    for qi, ((I, lb), (It, lbt)) in enumerate(zip(want, bounds(X, Q))):
                        assert np.array_equal(It, I), (dim, n, blocks, tiles, qi, np.argwhere(It != I)[:4].ravel())
                        assert np.array_equal(lbt, lb), (dim, n, blocks, tiles, qi, np.argwhere(lbt != lb)[:4].ravel())
    finally:
        tune()


@pytest.mark.parametrize("dim", DIMS)
def test_integer_sums_at_every_group_count(six, dim):
    """I equals the numpy integer dot on rows that are their own codes, at every count of `counts` and in every launch
    shape that takes another instance of the kernel"""
    from seesaw_amd.device_index import DeviceIndex
    G, W = shape(dim)
    rng = np.random.default_rng(5)
    Q = [rng.integers(-3, 4, dim).astype(np.float32), edge_queries(rng, dim)[3], rng.standard_normal(dim).astype(np.float32)]
    T = [quantise_query(q) for q in Q]
    try:
        for n in counts(G, W):
            X = int_rows(n, dim, seed=n)
            idx = DeviceIndex.from_numpy(X)
            try:
                c, s, _ = hook_shadow6(idx)
                assert np.array_equal(c, X.astype(np.int8)) and np.all(s == 1)
                want = [integer_sums(c, t) for t in T]
                for tiles in (-1, 1, 2, 4):
                    if tiles * dim > 1024:
                        continue
                    tune(-1, tiles)
                    for q, I in zip(Q, want):
                        got = hook_bounds6(idx, q)["I"]
                        assert np.array_equal(got, I), (dim, n, tiles, np.argwhere(got != I)[:4].ravel())
            finally:
                idx.close()
    finally:
        tune()
