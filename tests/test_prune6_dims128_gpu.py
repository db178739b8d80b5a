"""GPU: the packed 6-bit shadow at dims 384, 640, 896, 1152 and 1280, f32 and float16 rows, on the lab build
(csrc/prune.hip: Q6TilesH, k_q6_build_dims128 / k_q6_build_h16_dims128; csrc/ssw_common.h: q6_word_offset's tail load).
Sizes: one row, a tile and a row, and 2 G W + G + 5 rows (G rows a request, W waves of a full launch): a wave with two
groups, a wave with three and a ragged group.  Results are compared exactly; the band of a6 is the 6-bit tests'."""
import functools
from contextlib import closing

import numpy as np
import pytest

from _prune6_f16_helpers import f16_rows
from _prune768_helpers import (batch6, hook_bounds6, hook_bounds6_mq, hook_shadow6, integer_sums, launch_shape6,
                               launch_shape6_mq, mode6, shadow6)
from _prune_batch_helpers import edge_queries
from _prune_helpers import adversarial_rows, mode, query, same

pytestmark = pytest.mark.gpu

DIMS = [384, 640, 896, 1152, 1280]
DTYPES = [np.float32, np.float16]
# the product's constants (csrc/index_prune.hip): MIN_ROWS_DIMS128's smallest entry with a dim that has it, and the bound
# of MAX_ROWS_DIMS128 at dim 1152
SMALLEST_MIN_ROWS = {np.float32: (640, 1 << 18), np.float16: (640, 1 << 20)}
MAX_ROWS_1152 = 12_500_000


@pytest.fixture()
def six(lab_build):
    """every size takes the 6-bit path, single query and batch, and the three-launch top-k of small indexes, which
    never prunes, is off; the defaults again afterwards"""
    from seesaw_amd import _lib
    mode(lab_build, True)
    mode6(True, 1)
    batch6(1)
    _lib.call("ssw_tune_topk", 2)
    try:
        yield lab_build
    finally:
        _lib.call("ssw_tune_topk", 3)
        batch6(-1)
        mode6(True, -1)
        mode(lab_build, True)


def unpruned(lib, fn):
    mode(lib, False)
    out = fn()
    mode(lib, True)  # (the fixture restores it after a failure)
    return out


@functools.lru_cache(None)
def sizes(dim):
    from seesaw_amd.device_index import DeviceIndex
    probe = DeviceIndex(1 << 20, dim)  # scan_shape clamps the grid to the rows: enough rows for a full launch, not filled
    shapes = [launch_shape6(probe), launch_shape6_mq(probe)]
    probe.close()
    G, W = 16 * max(t for _, t in shapes), 4 * max(b for b, _ in shapes)
    return [1, 17, 2 * G * W + G + 5]


def rows(n, dim, dtype, seed):
    """(what goes up, the f32 rows the index then holds): Gaussian rows of mixed scale with the adversarial rows over
    the first rows, a tile boundary and the last rows"""
    if dtype == np.float16:
        return f16_rows(n, dim, seed=seed)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    adv = adversarial_rows(rng, dim)
    m = adv.shape[0]
    X[:min(m, n)] = adv[:min(m, n)]
    if n >= 6 * m:
        at = ((n // 2) // 16) * 16 - m // 2
        X[at:at + m] = adv
        X[n - m:] = adv[::-1]
    return np.ascontiguousarray(X), X


def make(X, dtype):
    from seesaw_amd.device_index import DeviceIndex
    return closing(DeviceIndex.from_numpy(X, dtype=dtype))


CASES = pytest.mark.parametrize("dim,dtype", [(d, t) for d in DIMS for t in DTYPES])


@CASES
def test_codes_equal_the_twin(six, dim, dtype):
    for n in sizes(dim):
        X, W = rows(n, dim, dtype, seed=n + dim)
        with make(X, dtype) as idx:
            assert idx.prune_stats()["eligible"]
            c, s, a = hook_shadow6(idx)
            tc, ts, ta = shadow6(W)
            assert np.array_equal(c, tc), (n, np.argwhere(c != tc)[:4])
            assert np.array_equal(s.view(np.uint32), ts.view(np.uint32))
            inf = np.isinf(ta)
            assert np.array_equal(np.isinf(a), inf)
            fa, fta = a[~inf].astype(np.float64), ta[~inf].astype(np.float64)
            assert np.all(np.abs(fa - fta) <= 2.0 ** -20 * fta)
            assert idx.prune_stats()["shadow_bytes"] == (n + 15) // 16 * 16 * (3 * dim // 4 + 8)


@CASES
def test_lane_map_on_exact_integers(six, dim, dtype):
    """rows that are their codes (integers in [-31, 31], exact in binary16 too): every integer sum of both scans equals
    numpy's integer dot of the shadow's codes with the hook's own query codes"""
    rng = np.random.default_rng(dim)
    Q = np.ascontiguousarray(rng.standard_normal((16, dim)) * np.exp2(rng.integers(-12, 13, 16))[:, None], dtype=np.float32)
    Q[3] = edge_queries(rng, dim)[3]  # rint ties and clamped lo codes
    for n in sizes(dim):
        X = rng.integers(-31, 32, (n, dim)).astype(np.float32)
        X[np.arange(n), np.arange(n) % dim] = 31.0
        with make(X, dtype) as idx:
            c, s, _ = hook_shadow6(idx)
            assert np.array_equal(c, X.astype(np.int8)) and np.all(s == 1)
            out = hook_bounds6(idx, Q[0])
            assert not out["bad"]
            want = integer_sums(c, dict(d_hi=out["codes"][0], d_lo=out["codes"][1]))
            assert np.array_equal(out["I"], want), (n, np.argwhere(out["I"] != want)[:4])
            for w in (3, 16):
                out = hook_bounds6_mq(idx, Q[16 - w:])
                assert not out["bad"].any()
                for j in range(w):
                    want = integer_sums(c, dict(d_hi=out["codes"][j, 0], d_lo=out["codes"][j, 1]))
                    assert np.array_equal(out["I"][j], want), (n, w, j, np.argwhere(out["I"][j] != want)[:4])


@CASES
def test_certificate_row_by_row(six, dim, dtype):
    Q = edge_queries(np.random.default_rng(11), dim)
    for n in sizes(dim):
        X, _ = rows(n, dim, dtype, seed=n + dim)
        with make(X, dtype) as idx:
            S = unpruned(six, lambda: [idx.scores(q) for q in Q])  # the device's full scan
            _, _, a = hook_shadow6(idx, codes=False)
            fin = np.isfinite(a)
            chunk = hook_bounds6_mq(idx, np.stack(Q), sums=False)
            for j, (q, Sq) in enumerate(zip(Q, S)):
                out = hook_bounds6(idx, q, sums=False)
                for lb, bad in ((out["lb"], out["bad"]), (chunk["lb"][j], chunk["bad"][j])):
                    if bad:
                        continue
                    assert np.all(lb[~fin] == -np.inf), (n, j)
                    late = ~(lb[fin] <= Sq[fin])
                    assert not late.any(), (n, j, np.nonzero(fin)[0][late][:8])


@CASES
def test_pruned_calls_return_the_unpruned_bytes(six, dim, dtype):
    for n in sizes(dim):
        rng = np.random.default_rng(n)
        X = np.ascontiguousarray(rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim)))
        with make(X, dtype) as idx:
            r2i = np.repeat(np.arange(n), rng.integers(1, 5, n))[:n].astype(np.int32)  # 1 .. 4 rows an image
            idx.set_row2image(r2i)
            first = np.concatenate(([True], r2i[1:] != r2i[:-1]))
            idx.set_tile_meta(np.where(first[:, None], np.float32([0, 0, 1, 1]), np.float32([0, 0, .5, .5])),
                              np.where(first, 0, 1).astype(np.int32))
            ex = np.arange(1, idx.n_images, 7)
            k = min(10, idx.n_images - ex.shape[0])
            pos = np.unique(rng.integers(0, idx.n_images, 50))
            calls = [lambda: idx.topk(query(n, dim), k, excluded=ex),
                     lambda: (idx.topk(query(n + 1, dim), k), idx.rescore_avg(pos, "greater"))[1]]
            for nq in (3, 16):
                Qb = np.stack([query(100 * nq + b, dim) for b in range(nq)])
                calls.append(lambda Qb=Qb: idx.topk_batch(Qb, k, [ex.tolist()] * Qb.shape[0], prune=True))
            for call in calls:
                full = unpruned(six, call)
                before = idx.prune_stats()
                got = call()
                st = idx.prune_stats()
                if isinstance(got, list):
                    assert len(got) == len(full)
                    for x, y in zip(full, got):
                        same(x, y)
                else:
                    same(full, got)
                assert st["eligible"] and st["shadow"] == "current" and st["fallbacks"] == before["fallbacks"], (n, st)
                assert st["queries"] > before["queries"], (n, before, st)


@pytest.mark.parametrize("dtype", DTYPES)
def test_product_threshold(lab_build, dtype):
    """without the lab switches an index of the table's smallest entry is pruned on the 6-bit shadow and one of a tile
    fewer rows is not; at dim 1152 an index of MAX_ROWS_DIMS128's rows is eligible and one of a tile more is not"""
    from seesaw_amd.device_index import DeviceIndex
    dim, n_min = SMALLEST_MIN_ROWS[dtype]
    mode(lab_build, True)
    mode6(True, -1)
    batch6(-1)
    block = np.random.default_rng(dim).standard_normal((1 << 16, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X = np.tile(block, (n_min >> 16, 1))
    for n, pruned in ((n_min - 16, False), (n_min, True)):
        with make(X[:n], dtype) as idx:
            assert idx.prune_stats()["eligible"] == pruned
            idx.topk(query(300, dim), 100)
            st = idx.prune_stats()
            assert st["shadow"] == ("current" if pruned else "none") and st["queries"] == int(pruned), st
            assert st["shadow_bytes"] == (n * (3 * dim // 4 + 8) if pruned else 0), st
    for n, eligible in ((MAX_ROWS_1152, True), (MAX_ROWS_1152 + 16, False)):
        with closing(DeviceIndex(n, 1152, dtype=dtype)) as idx:  # rows not filled: nothing is computed on it
            assert idx.prune_stats()["eligible"] == eligible
