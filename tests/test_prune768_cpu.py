"""CPU: the packed 6-bit shadow at dim 768 on the numpy twin (tests/_prune768_helpers.py): the placement is dim-free and
round-trips, a tile is 9216 bytes, the code norm is the one the kernels carry, integer rows tell a wrong placement apart,
and the twin's bound brackets the float64 score."""
import os
import re

import numpy as np
import pytest

from _prune768_helpers import (CODE_NORM_768, DIM, ROW_BYTES, code_norm, integer_sums, lower_bound6, pack, quantise_query,
                               shadow6, shadow_bytes, tile_bytes, unpack, width6)
from _prune_batch_helpers import edge_queries, upper_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 16, 17, 37])
def test_pack_unpack_round_trip(n):
    rng = np.random.default_rng(n)
    c = rng.integers(-31, 32, (n, DIM)).astype(np.int8)
    c[0, :4] = (-31, 31, -1, 0)
    packed = pack(c)
    assert packed.shape == ((n + 15) // 16, 9216) and packed.dtype == np.uint8
    assert np.array_equal(unpack(packed, n, DIM), c)
    # the rows past n of the last tile stay zero: the kernels read them and store nothing for them
    full = unpack(packed, packed.shape[0] * 16, DIM)
    assert not full[n:].any()


def test_tile_and_row_sizes():
    assert tile_bytes(DIM) == 9216 == 9 * 1024  # nine 1-KiB wave loads a tile
    assert ROW_BYTES == 584
    assert shadow_bytes(1) == 16 * 584 and shadow_bytes(16) == 16 * 584 and shadow_bytes(17) == 32 * 584
    assert shadow_bytes(50_000_000) == 50_000_000 * 584


def test_code_norm_constant():
    exact = 31.0 * np.sqrt(np.float64(768.0))
    assert CODE_NORM_768 >= exact  # ||c|| <= 31 sqrt(dim): a smaller constant would void the certificate
    assert (CODE_NORM_768 - exact) / exact <= 1e-8
    assert code_norm(768) == CODE_NORM_768 and code_norm(512) == 701.4499270
    # the kernels carry the same literal, in the dim-768 arm of q6_code_norm
    src = open(os.path.join(ROOT, "seesaw_amd", "csrc", "prune.hip")).read()
    body = re.search(r"constexpr double q6_code_norm\(int dim\) \{(.*?)\}", src, re.S).group(1)
    assert re.search(r"dim == 768 \? 859\.0972006\b", body), body


def test_integer_rows_expose_a_wrong_placement():
    """the rows and queries of the GPU lane-map test at dim 768, on the packed bytes: each mutation of the placement
    changes some integer sum, so a kernel that read the tile that way would fail the comparison with the numpy dot"""
    rng = np.random.default_rng(5)
    n = 50
    X = rng.integers(-31, 32, (n, DIM))
    X[np.arange(n), np.arange(n) % DIM] = 31
    qq = quantise_query(rng.integers(-3, 4, DIM).astype(np.float32))
    want = integer_sums(X, qq)
    packed = pack(X)
    assert np.array_equal(integer_sums(unpack(packed, n, DIM), qq), want)
    tiles = packed.reshape(packed.shape[0], 9, 4, 16, 16)  # [tile, load, lane group, row, byte]
    swapped_rows = tiles[:, :, :, np.arange(16) ^ 1, :]
    swapped_groups = tiles[:, :, [0, 2, 1, 3], :, :]
    words = packed.reshape(packed.shape[0], -1, 4).copy()  # the low two bits of every word's bytes, rotated by a byte
    rotated = ((words & 0xfc) | (np.roll(words, 1, axis=2) & 3)).reshape(packed.shape)
    seen = []
    for name, mut in (("rows", swapped_rows), ("lane groups", swapped_groups), ("low bits", rotated)):
        got = integer_sums(unpack(np.ascontiguousarray(mut).reshape(packed.shape), n, DIM), qq)
        assert np.any(got != want), name
        seen.append(got)
    # ... and tell the mutations apart from one another
    for i in range(3):
        for j in range(i + 1, 3):
            assert np.any(seen[i] != seen[j]), (i, j)


def test_the_twins_bound_brackets_the_score():
    """(***) of csrc/prune.hip at dim 768 on the twin: lb < S <= ub in float64 for Gaussian rows of mixed scale and the
    edge queries, with the width formed from the dim-768 code norm"""
    rng = np.random.default_rng(8)
    n = 37
    X = rng.standard_normal((n, DIM)).astype(np.float32) / np.float32(np.sqrt(DIM))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    c, s, a = shadow6(X)
    assert np.abs(c).max() == 31 and np.all(np.isfinite(a))
    assert np.all(np.sqrt((c.astype(np.float64) ** 2).sum(1)) <= CODE_NORM_768)
    for q in edge_queries(rng, DIM):
        qq = quantise_query(q)
        assert not qq["bad"]
        lb, w, _ = lower_bound6(c, s, a, qq)
        assert np.array_equal(w, width6(s, a, qq))
        S = X.astype(np.float64) @ q.astype(np.float64)
        assert np.all(lb.astype(np.float64) < S) and np.all(S <= upper_bound(lb, w))
