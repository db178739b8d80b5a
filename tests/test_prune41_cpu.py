"""CPU: the numpy twin of the two-stage 4 + 1-bit shadow (tests/_prune41_helpers.py; csrc/prune.hip, "two-stage 4 + 1-bit
shadow"): the placement of both planes and its inverse, the scan's unpack, the split c = 2 h + b - 16, the identity between
the two-plane sums and the 5-bit scan's integer sum, both certificates in double, a4's band, and four mutations of the twin
that each fail the check that is there to catch them."""
import numpy as np
import pytest

from _prune41_helpers import (COARSE_CAP, E2E_QUERY_SEED, SURV_CAP, SURV_STAGE, TWIN, big_rows, candidates, code_norm4, coarse_tile_bytes, dvec,
                              exact_threshold, integer_sums, lower_bound4, lower_bound5, lower_bound5_from_parts, nibble,
                              operand_bytes, pack_coarse, pack_fine, quantise_query, shadow41, shadow5, split, sums41, survivors,
                              unpack_coarse, unpack_fine, upper_bound)
from _prune6_helpers import slot, word_offset
from _prune_helpers import SAFETY, gamma, query
from test_prune5_cpu import edge_rows

DIMS = (512, 1024)


def rows_for(dim, n):
    """the five edge rows, a row of -max throughout (every 2 h - 15.5 is -15.5: the code norm's extreme) and n Gaussian rows"""
    X = np.random.default_rng(dim).standard_normal((n, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    low = np.full((1, dim), -0.03125, dtype=np.float32)
    return np.concatenate([edge_rows(dim), low, X])


def queries_for(dim):
    """a Gaussian query, a scaled one, and an all-positive one (sum D is large: the per-query offset matters most)"""
    pos = np.abs(query(52, dim))
    return [query(50, dim), query(51, dim) * np.float32(37.5), pos]


# ---- the checks, each on a twin given as a parameter (the mutation tests run them on a changed copy) -------------------
def check_unpack(twin):
    """the scan's two ands and two shift-and-masks give the nibbles of a k-step, slot for slot"""
    rng = np.random.default_rng(2)
    for dim in DIMS:
        h = rng.integers(0, 16, (16, dim))
        tile = pack_coarse(h, swap=twin["swap_nibbles"])[0]
        for lane in range(64):
            r, g = lane & 15, lane >> 4
            for ks in range(dim // 64):
                assert np.array_equal(operand_bytes(tile, lane, ks), h[r, 64 * ks + 16 * g:64 * ks + 16 * g + 16]), (dim, lane, ks)


def check_identity(twin):
    """J = 4 H - 31 sum D is the sum of (4 h - 31) D, and I = 8 (2 H + B - 16 sum D) = 4 J + 8 B - 4 sum D is the 5-bit
    scan's integer sum"""
    for dim in DIMS:
        X = rows_for(dim, 300)
        c, _, _ = shadow5(X)
        h, b, s, a5, a4 = shadow41(X, twin)
        for q in queries_for(dim):
            t = quantise_query(q)
            H, B, sumD = sums41(h, b, t)
            J = 4 * H - twin["offset"] * sumD
            assert np.array_equal(J, (4 * h - 31) @ dvec(t)), dim
            I = integer_sums(c, t)
            assert np.array_equal(8 * (2 * H + B - 16 * sumD), I)
            assert np.array_equal(4 * J + 8 * B - 4 * sumD, I)
            assert np.abs(H).max() < 2 ** 31 and np.abs(B).max() < 2 ** 25


def check_code_norm(twin):
    """the kernel's constant bounds ||2 h - 15.5|| of every row, the row of -max throughout included (15.5 sqrt(dim))"""
    for dim in DIMS:
        h, _, _, _, _ = shadow41(rows_for(dim, 50), twin)
        norms = np.sqrt(((2.0 * h - 15.5) ** 2).sum(1))
        assert np.isclose(norms.max(), 15.5 * np.sqrt(dim), rtol=1e-12)
        assert norms.max() <= code_norm4(dim, twin["mid"]), dim


def check_certificates(twin):
    """lb4 <= S <= ub4 and lb5 <= S <= ub5 row by row; S as the exact dot product in double and as an f32 dot product"""
    for dim in DIMS:
        X = rows_for(dim, 1 << 13 if dim == 512 else 1 << 11)
        c, _, _ = shadow5(X)
        h, b, s, a5, a4 = shadow41(X, twin)
        fin = np.isfinite(a5)
        assert np.array_equal(np.isfinite(a4), fin) and not fin[2] and not fin[3] and fin.sum() == len(X) - 2
        for q in queries_for(dim):
            t = quantise_query(q)
            assert not t["bad"]
            lb4, w4, H = lower_bound4(h, s, a4, t, twin)
            _, B, sumD = sums41(h, b, t)
            lb5, w5, I = lower_bound5_from_parts(H, B, sumD, s, a5, t, dim)
            ref5, _, _ = lower_bound5(c, s, a5, t)
            assert np.array_equal(lb5.view(np.uint32), ref5.view(np.uint32))  # the 5-bit twin's bound, bit for bit
            S64 = X[fin].astype(np.float64) @ q.astype(np.float64)
            S32 = (X[fin] @ q).astype(np.float64)
            for lb, w in ((lb4, w4), (lb5, w5)):
                ub = upper_bound(lb, w)
                for S in (S64, S32):
                    bad = ~((np.float64(lb[fin]) <= S) & (S <= ub[fin]))
                    assert not bad.any(), (dim, int(bad.sum()), np.nonzero(bad)[0][:6])
                assert np.all(lb[~fin] == -np.inf) and np.all(np.isinf(w[~fin]))


def check_a4_band(twin):
    """a4 >= SAFETY (||x - s5 (2 h - 15.5)|| + gamma (||x|| + s5 ||2 h - 15.5||)) in double, and within 2^-20 of it"""
    for dim in DIMS:
        X = rows_for(dim, 500)
        h, _, s, a5, a4 = shadow41(X, twin)
        fin = np.isfinite(a5)
        Xd, sd = X[fin].astype(np.float64), s[fin].astype(np.float64)[:, None]
        mid = 2.0 * h[fin] - 15.5
        g = gamma(dim)
        want = SAFETY * (np.linalg.norm(Xd - sd * mid, axis=1) + g * np.linalg.norm(Xd, axis=1) + g * sd[:, 0] * np.linalg.norm(mid, axis=1))
        got = a4[fin].astype(np.float64)
        assert np.all(got >= want * (1 - 2.0 ** -40)) and np.all(got <= want * (1 + 2.0 ** -20)), dim
        assert np.all(got[6:] > 1.5 * a5[fin].astype(np.float64)[6:])  # Gaussian rows: the 4-bit residual is about twice the 5-bit one


# ---- the twin as it is -------------------------------------------------------------------------------------------------
def test_every_nibble_of_a_tile_is_one_element():
    for dim in DIMS:
        hits = np.zeros((coarse_tile_bytes(dim), 2), dtype=np.int64)
        u, g, j = slot(np.arange(dim))
        for r in range(16):
            for i in range(dim):
                word, byte, shift = nibble(int(u[i]), int(j[i]))
                assert 2 * int(u[i]) <= word < 2 * int(u[i]) + 2
                hits[word_offset(16 * int(g[i]) + r, word) + byte, shift // 4] += 1
        assert np.all(hits == 1), dim


def test_both_planes_round_trip():
    rng = np.random.default_rng(1)
    for dim in DIMS:
        for n in (1, 15, 16, 17, 50):
            h, b = rng.integers(0, 16, (n, dim)), rng.integers(0, 2, (n, dim))
            h[0, :] = np.resize(np.arange(16), dim)
            p = pack_coarse(h)
            assert p.shape == ((n + 15) // 16, coarse_tile_bytes(dim))
            assert np.array_equal(unpack_coarse(p, n, dim), h)
            f = pack_fine(b)
            assert f.shape == (n, dim // 32) and f.dtype == np.uint32
            assert np.array_equal(unpack_fine(f, dim), b)
        one = np.zeros((1, dim), dtype=np.int64)
        one[0, 37] = 1
        assert pack_fine(one)[0, 1] == 1 << 5 and np.count_nonzero(pack_fine(one)) == 1


def test_a_code_is_twice_its_nibble_plus_its_bit_minus_sixteen():
    c = np.arange(-15, 16)
    h, b = split(c)
    assert np.array_equal(2 * h + b - 16, c) and h.min() == 0 and h.max() == 15 and set(b) == {0, 1}
    for dim in DIMS:
        X = rows_for(dim, 200)
        c, _, _ = shadow5(X)
        h, b, _, _, _ = shadow41(X)
        assert np.array_equal(2 * h + b - 16, c.astype(np.int64))


def test_the_scans_unpack_is_the_nibble():
    check_unpack(TWIN)


def test_two_plane_sums_are_the_five_bit_integer_sum():
    check_identity(TWIN)


def test_code_norm_bounds_every_row():
    check_code_norm(TWIN)


def test_both_certificates_in_double():
    check_certificates(TWIN)


def test_a4_within_its_band():
    check_a4_band(TWIN)


# ---- mutations of a twin copy, each caught by the named check ---------------------------------------------------------
@pytest.mark.parametrize("change, check", [
    (dict(swap_nibbles=True), check_unpack),     # nibble order swapped
    (dict(offset=32), check_identity),           # the per-query offset 31 -> 32
    (dict(mid=15.0), check_code_norm),           # code norm 15 sqrt(dim) instead of 15.5 sqrt(dim)
    (dict(a4_is_a5=True), check_certificates),   # a5 used in place of a4
    (dict(a4_is_a5=True), check_a4_band),
    (dict(offset=32), check_certificates),       # (the all-positive query)
])
def test_a_mutated_twin_fails_its_check(change, check):
    with pytest.raises(AssertionError):
        check(dict(TWIN, **change))


def test_survivor_counts_of_the_gpu_tests_rows_stay_under_both_caps():
    """the rows and queries of tests/test_prune41_gpu.py's end-to-end test, on the twin alone: the first stage leaves
    tens of thousands of 100 008 rows, the refine a fraction of them, both far under their caps (2^23, 2^18); at
    k = 1000 one block's 1024-row share of the first stage is not what decides a flush (the lab hook's one-block launch is)"""
    dim = 512
    X = big_rows(dim)
    n = len(X)
    q = query(E2E_QUERY_SEED, dim)
    t = quantise_query(q)
    lb4, lb5, exact = (np.empty(n, np.float32) for _ in range(3))
    w4, w5 = np.empty(n), np.empty(n)
    for at in range(0, n, 1 << 12):  # in blocks that stay in cache: the twin works in float64
        rows = slice(at, at + (1 << 12))
        h, b, s, a5, a4 = shadow41(X[rows])
        lb4[rows], w4[rows], H = lower_bound4(h, s, a4, t)
        _, B, sumD = sums41(h, b, t)
        lb5[rows], w5[rows], _ = lower_bound5_from_parts(H, B, sumD, s, a5, t, dim)
        with np.errstate(invalid="ignore"):
            exact[rows] = X[rows] @ q
    for k in (1, 100, 1000):
        T, _, _ = exact_threshold(lb4, exact, k)
        s1 = survivors(lb4, w4, T)
        s2 = np.intersect1d(s1, survivors(lb5, w5, T))
        assert candidates(k) >= k and k <= s2.size <= s1.size
        assert SURV_STAGE < s1.size < COARSE_CAP and s2.size < SURV_CAP, (k, s1.size, s2.size)
        print(f"k={k}: first stage {s1.size} of {len(X)}, refine {s2.size}")
