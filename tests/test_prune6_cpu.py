"""CPU: the packed 6-bit shadow's certificate ("6-bit shadow"), restated in numpy

    lb < S < ub,   lb = (s6 / 4) t2 I - w - pads,   ub = lb + 2 w + pads,   w = a6 Q + s6 31 sqrt(dim) e

with S = the f32 scan's score (oracle.scores_kernel_order, the bits of scan.hip) on the adversarial rows of
tests/test_prune_cpu.py; the packing (every code value in every slot survives pack -> unpack, and the masks and shifts
of k_q6_bounds turn the packed words into the int8 values 4 c); and the survivor count that lets the GPU test demand a
pruned call without a fallback."""
import numpy as np
import pytest

from _prune6_helpers import (code_norm, integer_sums, lower_bound6, operand_words, pack, quantise_query, shadow6, slot,
                             unpack, upper_bound, width6)
from _prune_batch_helpers import edge_queries
from _prune_helpers import PAD_ABS, SAFETY, adversarial_rows, gamma, queries

DIMS = (256, 512, 1024)


@pytest.mark.parametrize("dim", DIMS)
def test_pack_unpack_is_the_identity_on_every_code_in_every_slot(dim):
    # row r holds code ((i + 17 r) % 63) - 31 at element i.  17 and 63 are coprime, so over the first 63 rows every
    # element -- every slot of every lane group and k-step -- takes all 63 code values (asserted below); the 79 rows
    # fill four tiles and part of a fifth, so every row position of a tile occurs with several patterns.
    r, i = np.arange(63 + 16)[:, None], np.arange(dim)[None, :]
    codes = ((i + r * 17) % 63 - 31).astype(np.int8)
    for e in range(dim):
        assert set(codes[:63, e].tolist()) == set(range(-31, 32))
    packed = pack(codes)
    assert packed.shape == (5, 16 * dim * 3 // 4)
    assert np.array_equal(unpack(packed, codes.shape[0], dim), codes)
    # no two codes share a bit: the packed bytes of a one-hot row differ from zero in exactly the code's six bits
    for e in (0, 11, 12, 15, 63, 64, dim - 4, dim - 1):
        one = np.zeros((16, dim), np.int8)
        one[5, e] = -1
        assert int(np.unpackbits(pack(one)).sum()) == 6
    # the kernel's unpack: masks and shifts on the three words of a k-step give 4 c in the slots' order
    u, g, j = slot(np.arange(dim))
    for row in (0, 7, 15, 16 + 3):
        for lg in range(4):
            for ks in (0, dim // 64 - 1):
                want = np.zeros(16, np.int64)
                sel = (u == ks) & (g == lg)
                want[j[sel]] = 4 * codes[row, sel].astype(np.int64)
                got = operand_words(packed[row >> 4], 16 * lg + (row & 15), ks)
                assert np.array_equal(got, want), (row, lg, ks)


@pytest.mark.parametrize("dim", DIMS)
def test_bound_holds_on_adversarial_rows(oracle, dim):
    rng = np.random.default_rng(0)
    X = adversarial_rows(rng, dim)
    c, s, a = shadow6(X)
    assert np.abs(c.astype(np.int64)).max() == 31
    bad = ~np.all(np.isfinite(X), axis=1)
    m = np.max(np.abs(np.where(np.isfinite(X), X, 0)), axis=1)
    out_of_range = (m > 0) & ((m < 2.0 ** -60) | (m > 2.0 ** 60))
    assert bad.sum() == 3 and out_of_range.sum() == 10
    unb = bad | out_of_range
    assert np.all(np.isinf(a[unb])) and np.all(np.isfinite(a[~unb])) and np.all(c[unb] == 0) and np.all(s[unb] == 0)
    assert 31 * np.sqrt(dim) <= code_norm(dim) <= 31 * np.sqrt(dim) * (1 + 1e-6)
    Xf = np.where(np.isfinite(X), X, 0).astype(np.float32)
    fin = np.isfinite(a)
    checked = 0
    for q in queries(rng, X) + edge_queries(rng, dim):
        qq = quantise_query(q)
        if qq["bad"]:
            continue  # the zero query: the call takes the full scan
        S = oracle.scores_kernel_order(Xf, q).astype(np.float64)
        lb, w, I = lower_bound6(c, s, a, qq)
        assert np.abs(I).max() < 2 ** 33 and np.abs(c.astype(np.int64) @ qq["d_hi"].astype(np.int64)).max() * 4 < 2 ** 31
        ub = upper_bound(lb, w)
        l = lb.astype(np.float64)
        assert np.all(np.isfinite(l[fin])) and np.all(l[fin] < S[fin]) and np.all(S[fin] < ub[fin]), dim
        assert np.all(lb[~fin] == -np.inf) and not np.any(ub[~fin] < np.inf)  # always rescored
        checked += 1
    assert checked >= 12


@pytest.mark.parametrize("dim", DIMS)
def test_integer_rows_expose_a_wrong_placement(dim):
    """the rows and queries of the GPU lane-map test, on the packed bytes: each mutation of the placement changes
    some integer sum, so a kernel that read the tile that way would fail the comparison with the numpy dot"""
    rng = np.random.default_rng(5)
    n = 50
    X = rng.integers(-31, 32, (n, dim))
    X[np.arange(n), np.arange(n) % dim] = 31
    qq = quantise_query(rng.integers(-3, 4, dim).astype(np.float32))
    want = integer_sums(X, qq)
    packed = pack(X)
    assert np.array_equal(integer_sums(unpack(packed, n, dim), qq), want)
    tiles = packed.reshape(packed.shape[0], dim * 3 // 4 // 64, 4, 16, 16)  # [tile, load, lane group, row, byte]
    swapped_rows = tiles[:, :, :, np.arange(16) ^ 1, :]
    swapped_groups = tiles[:, :, [0, 2, 1, 3], :, :]
    words = packed.reshape(packed.shape[0], -1, 4).copy()  # the low two bits of every word's bytes, rotated by a byte
    rotated = ((words & 0xfc) | (np.roll(words, 1, axis=2) & 3)).reshape(packed.shape)
    for name, mut in (("rows", swapped_rows), ("lane groups", swapped_groups), ("low bits", rotated)):
        got = integer_sums(unpack(np.ascontiguousarray(mut).reshape(packed.shape), n, dim), qq)
        assert np.any(got != want), name


def _block_bounds(seed, rows, dim, qq):
    """(lb f64, ub f64, sum of a6) of `rows` unit Gaussian rows: the twin's formulas with the row passes in f32 (the two
    integer sums are exact in f32: |sum| <= 31 * 127 * 512 < 2^24) and a6 from f32 sums, inflated by 1 + 2^-10 for
    them -- a larger a6 only adds survivors"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, dim), dtype=np.float32)
    X /= np.sqrt(np.einsum("ij,ij->i", X, X))[:, None]
    s = np.abs(X).max(axis=1) / np.float32(31)
    c = np.rint(X / s[:, None])
    I = 4.0 * (256.0 * (c @ qq["d_hi"].astype(np.float32)).astype(np.float64)
               + (c @ qq["d_lo"].astype(np.float32)).astype(np.float64))
    c *= s[:, None]
    c -= X
    g = gamma(dim)
    a = (np.sqrt(np.einsum("ij,ij->i", c, c)).astype(np.float64) + 2 * g * (1 + 1e-3)) * SAFETY * (1 + 2.0 ** -10)
    w = width6(s, a, qq, dim)
    lb = s.astype(np.float64) * (np.float64(qq["t2"]) * 0.25) * I - w
    lb -= np.abs(lb) * 2.0 ** -50 + PAD_ABS
    lb = np.nextafter(lb.astype(np.float32), np.float32(-np.inf)).astype(np.float64)  # at or below the rounded-down f32
    return lb, upper_bound(lb, w), float(a.sum())


def test_survivors_of_gaussian_rows_stay_under_the_cap():
    """the estimate of the issue as a check: 2^22 unit Gaussian rows of dim 512, k = 100; the rows whose upper bound
    reaches the k-th lower bound stay <= 2^18 (SURV_CAP), so a pruned call at this size needs no fallback"""
    import os
    from concurrent.futures import ThreadPoolExecutor
    n, dim, k, block = 1 << 22, 512, 100, 1 << 15
    q = np.random.default_rng(3).standard_normal(dim).astype(np.float32)
    q /= np.float32(np.linalg.norm(q))
    qq = quantise_query(q)
    with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as pool:
        parts = list(pool.map(lambda b: _block_bounds(1000 + b, block, dim, qq), range(n // block)))
    lb, ub = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    a_mean = sum(p[2] for p in parts) / n
    T = np.partition(lb, n - k)[n - k]
    survivors = int((~(ub < T)).sum())
    print(f"6-bit twin: mean a6 {a_mean:.4f}, survivors at 2^22 rows, k = {k}: {survivors}")
    assert 0.025 < a_mean < 0.035
    assert k <= survivors <= 1 << 18
