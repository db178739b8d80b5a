"""CPU: the numpy twin of the packed 5-bit shadow (tests/_prune5_helpers.py; csrc/prune.hip, "5-bit shadow"): the
placement and its inverse, the scan's unpack, the certificate in double, and the survivors the exact threshold leaves."""
import numpy as np

from _prune5_helpers import (LEVELS, SURV_CAP, candidates, code_norm, exact_threshold, fields, integer_sums, lower_bound5,
                             operand_words, pack, quantise_query, shadow5, survivors, tile_bytes, unpack, width5)
from _prune6_helpers import slot, word_offset
from _prune_helpers import query

DIMS = (512, 1024)


def test_every_bit_of_a_tile_is_one_code_bit():
    """q5_fields places the 5 bits of the 32 codes of a pair of k-steps on the 160 bits of the pair's five words, each
    once; over a tile every bit of every byte belongs to exactly one (row, element, code bit)"""
    for u0 in (0, 2):
        seen = {}
        for u in (u0, u0 + 1):
            for j in range(16):
                fl = fields(u, j)
                assert sorted(b for _, _, _, bits, frm in fl for b in range(frm, frm + bits)) == list(range(5)), (u, j)
                for word, byte, lo, bits, frm in fl:
                    assert 5 * (u0 >> 1) <= word < 5 * (u0 >> 1) + 5 and 0 <= byte < 4 and lo + bits <= 8
                    for t in range(bits):
                        assert seen.setdefault((word, byte, lo + t), (u, j, frm + t)) == (u, j, frm + t)
        assert len(seen) == 160
    for dim in DIMS:
        hits = np.zeros((tile_bytes(dim), 8), dtype=np.int64)
        u, g, j = slot(np.arange(dim))
        for r in range(16):
            for i in range(dim):
                for word, byte, lo, bits, _ in fields(int(u[i]), int(j[i])):
                    hits[word_offset(16 * int(g[i]) + r, word) + byte, lo:lo + bits] += 1
        assert np.all(hits == 1), dim


def test_pack_unpack_round_trip_every_slot():
    rng = np.random.default_rng(1)
    for dim in DIMS:
        for n in (1, 15, 16, 17, 50):
            c = rng.integers(-LEVELS, LEVELS + 1, (n, dim)).astype(np.int8)
            c[0, :] = np.resize(np.arange(-LEVELS, LEVELS + 1), dim)  # every code value, on every slot over the rows
            p = pack(c)
            assert p.shape == ((n + 15) // 16, tile_bytes(dim))
            assert np.array_equal(unpack(p, n, dim), c)
        # one code at a time: a single non-zero element reads back alone, at every slot of one row of every lane group
        # (tile i holds the case of element i)
        i = np.arange(dim)
        c = np.zeros((16 * dim, dim), dtype=np.int8)
        c[16 * i + i % 16, i] = np.where(i % 31 == 15, 1, -LEVELS + i % 31)
        p = pack(c)
        assert np.array_equal(unpack(p, 16 * dim, dim), c), dim
        assert np.all((p != 0).sum(1) <= 3)  # at most three bytes carry a code


def test_the_scans_unpack_is_eight_times_the_code():
    """the five ands, three spill words and two operands of k_q5_bounds give 8 c of the 32 codes of a pair, slot for slot"""
    rng = np.random.default_rng(2)
    for dim in DIMS:
        c = rng.integers(-LEVELS, LEVELS + 1, (16, dim)).astype(np.int8)
        tile = pack(c)[0]
        for lane in range(64):
            r, g = lane & 15, lane >> 4
            for p in range(dim // 128):
                ops = operand_words(tile, lane, p)
                for half, u in enumerate((2 * p, 2 * p + 1)):
                    want = 8 * c[r, 64 * u + 16 * g:64 * u + 16 * g + 16].astype(np.int64)
                    assert np.array_equal(ops[half], want), (dim, lane, u)


def edge_rows(dim):
    """all-zero, one huge element, an inf, a NaN, and a row whose max lands exactly on a code boundary (max = 15 s with
    s a power of two, so x / s is an integer or an exact half for every element)"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X[0] = 0
    X[1, 7] = 3.0e4
    X[2, 9] = np.inf
    X[3, 0] = np.nan
    X[4] = (rng.integers(-30, 31, dim) / 2.0 * 2.0 ** -7).astype(np.float32)  # multiples of s / 2: rint ties
    X[4, 5] = 15 * 2.0 ** -7
    return X


def test_certificate_in_double():
    """| S - (s5 / 8) t2 I | <= w for every row: S as the exact dot product of the f32 values in double, and as an f32
    dot product (any summation order is inside gamma_dim)"""
    for dim in DIMS:
        rng = np.random.default_rng(dim)
        n = 1 << 16 if dim == 512 else 1 << 13
        X = rng.standard_normal((n, dim), dtype=np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
        X = np.concatenate([edge_rows(dim), X])
        c, s, a = shadow5(X)
        assert np.abs(c.astype(np.int64)).max() == LEVELS
        assert np.array_equal(np.isinf(a), np.array([False, False, True, True, False] + [False] * n))
        assert s[0] == 0 and not c[0].any() and not c[2].any() and not c[3].any()
        assert s[4] == np.float32(2.0 ** -7) and c[4, 5] == 15
        for qi in range(2):
            q = query(50 + qi, dim) * np.float32(1.0 if qi == 0 else 37.5)
            t = quantise_query(q)
            assert not t["bad"]
            lb, w, I = lower_bound5(c, s, a, t)
            assert np.all(w >= np.float64(a) * np.float64(t["Q"]))
            mid = np.float64(s) * (np.float64(t["t2"]) * 0.125) * I.astype(np.float64)
            fin = np.isfinite(a)
            S64 = X[fin].astype(np.float64) @ q.astype(np.float64)
            S32 = (X[fin] @ q).astype(np.float64)
            for S in (S64, S32):
                assert np.all(np.abs(S - mid[fin]) <= w[fin]), (dim, qi, float((np.abs(S - mid[fin]) / w[fin]).max()))
                assert np.all(np.float64(lb[fin]) <= S)
            assert np.all(lb[~fin] == -np.inf) and np.all(np.isinf(w[~fin]))
            # the code norm's rounding: 15 sqrt(dim) rounded UP bounds ||c||
            assert code_norm(dim) >= LEVELS * np.sqrt(dim)
            assert np.sqrt((c.astype(np.float64) ** 2).sum(1)).max() <= code_norm(dim)


def test_exact_threshold_keeps_a_fraction_of_the_cap():
    """2^18 unit Gaussian rows of dim 512, k = 100: with T from the 1024 candidates the twin's survivors stay under
    SURV_CAP / 4, where the k-th lower bound alone as the threshold leaves several times as many; every row of the exact
    top-k survives.  A cap, not a measurement: the seed is fixed so that the twin alone meets it."""
    dim, n, k = 512, 1 << 18, 100
    rng = np.random.default_rng(20)
    q = query(7, dim)
    t = quantise_query(q)
    lb, w, exact = np.empty(n, np.float32), np.empty(n), np.empty(n, np.float32)
    for at in range(0, n, 1 << 12):  # in blocks that stay in cache: the twin works in float64
        X = rng.standard_normal((1 << 12, dim), dtype=np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
        c, s, a = shadow5(X)
        d = (256 * t["d_hi"].astype(np.int64) + t["d_lo"].astype(np.int64)).astype(np.float64)
        I = (8.0 * c.astype(np.float64)) @ d  # exact in double: |I| < 2^39
        assert np.array_equal(I[:64], integer_sums(c[:64], t).astype(np.float64))
        wq = width5(s, a, t, dim)
        l = np.float64(s) * (np.float64(t["t2"]) * 0.125) * I - wq
        l = l - (np.abs(l) * 2.0 ** -50 + 2.0 ** -100)
        l32 = l.astype(np.float32)
        lb[at:at + len(X)] = np.where(l32.astype(np.float64) > l, np.nextafter(l32, np.float32(-np.inf)), l32)
        w[at:at + len(X)] = wq
        exact[at:at + len(X)] = X @ q
    assert candidates(k) == 1024
    T, T_lb, T_x = exact_threshold(lb, exact, k)
    kth = np.sort(exact)[::-1][k - 1]
    assert T_lb < T_x <= kth and T == T_x
    surv = survivors(lb, w, T)
    top = np.argsort(-exact, kind="stable")[:k]
    assert np.isin(top, surv).all()
    assert k <= surv.size < SURV_CAP // 4, surv.size
    assert survivors(lb, w, T_lb).size > 3 * surv.size
