"""CPU: the error bound of the int8 shadow (csrc/prune.hip) re-derived in numpy.  For every row the
shadow keeps codes c = rint(x / s) (|c| <= 127, s = max|x| / 127), the scale s and a_r; the claim is

    |S - s * A| <= a_r * ||q||        S = the f32 scan's score (oracle.scores_kernel_order, the bits of scan.hip),
                                      A = any f32 summation of c_i q_i

on adversarial rows: one huge element, all-equal elements, subnormals, zero rows, rows exactly on quantisation-step
boundaries; rows with a non-finite element or an out-of-range scale get a_r = +inf (always rescored)."""
import numpy as np

DIM = 512
U = 2.0 ** -24
GAMMA = DIM * U / (1 - DIM * U)
SAFETY = 1 + 2.0 ** -10
PAD_ABS = 2.0 ** -100


def shadow(X):
    """numpy twin of k_q8_build: (codes int8 [n, dim], s f32 [n], a f32 [n], rounded up)"""
    X = np.asarray(X, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        m = np.max(np.abs(X), axis=1)
    finite = np.all(np.isfinite(X), axis=1)
    ok = finite & ((m == 0) | ((m >= np.float32(2.0 ** -60)) & (m <= np.float32(2.0 ** 60))))
    s = np.where(ok & (m > 0), m / np.float32(127), np.float32(0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(s[:, None] > 0, np.rint(X / s[:, None]), 0.0)
    c = np.clip(np.nan_to_num(c), -127, 127).astype(np.int8)
    Xd = np.where(ok[:, None], X, 0).astype(np.float64)
    e = Xd - s.astype(np.float64)[:, None] * c.astype(np.float64)
    a = SAFETY * (np.sqrt((e * e).sum(1)) + GAMMA * np.sqrt((Xd * Xd).sum(1))
                  + GAMMA * s.astype(np.float64) * np.sqrt((c.astype(np.float64) ** 2).sum(1)))
    a32 = a.astype(np.float32)
    a32 = np.where(a32.astype(np.float64) < a, np.nextafter(a32, np.float32(np.inf)), a32)  # round up
    return c, s, np.where(ok, a32, np.float32(np.inf)).astype(np.float32)


def adversarial_rows(rng):
    base = rng.standard_normal((8, DIM)).astype(np.float32) / np.float32(np.sqrt(DIM))
    huge = base.copy()
    huge[:, 3] = 40.0
    sub = base[:3].copy()  # subnormal f32 elements beside normal ones
    sub[:, ::3] = (rng.standard_normal((3, (DIM + 2) // 3)) * 1e-39).astype(np.float32)
    tiny = (rng.standard_normal((2, DIM)) * 1e-39).astype(np.float32)  # max |x| below 2^-60: unbounded
    bad = base[:3].copy()
    bad[0, 7], bad[1, 9], bad[2, 0] = np.inf, -np.inf, np.nan
    # elements exactly halfway between two quantisation steps (the rint tie), the max pinning the step
    half = ((rng.integers(-126, 126, (4, DIM)) + 0.5) / 127.0).astype(np.float32)
    half[:, 0] = 1.0
    rows = [base, huge, np.full((2, DIM), 0.0442, np.float32), np.full((1, DIM), -3.0, np.float32), sub,
            np.zeros((2, DIM), np.float32), tiny, bad, half, (base * np.float32(2.0 ** 50)).astype(np.float32),
            (base * np.float32(2.0 ** 66)).astype(np.float32)]  # the last 8: scale out of range, unbounded
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)


def queries(rng, X):
    big = rng.standard_normal(DIM)
    big[3] = 1e6
    q = [rng.standard_normal(DIM), np.ones(DIM), X[8] * 7.0, np.zeros(DIM), big, rng.standard_normal(DIM) * 1e-30]
    return [np.asarray(v, dtype=np.float32) for v in q]


def test_bound_holds_on_adversarial_rows(oracle):
    rng = np.random.default_rng(0)
    X = adversarial_rows(rng)
    c, s, a = shadow(X)
    bad = ~np.all(np.isfinite(X), axis=1)
    m = np.max(np.abs(np.where(np.isfinite(X), X, 0)), axis=1)
    out_of_range = (m > 0) & ((m < 2.0 ** -60) | (m > 2.0 ** 60))
    assert bad.sum() == 3 and out_of_range.sum() == 10
    assert np.all(np.isinf(a[bad | out_of_range])) and np.all(np.isfinite(a[~(bad | out_of_range)]))
    Xf = np.where(np.isfinite(X), X, 0).astype(np.float32)
    fin = np.isfinite(a)
    for q in queries(rng, X):
        S = oracle.scores_kernel_order(Xf, q).astype(np.float64)
        Q = np.sqrt(np.sum(q.astype(np.float64) ** 2)) * (1 + 2.0 ** -40)
        prods = c.astype(np.float32) * q[None, :]
        for A in (prods.sum(1, dtype=np.float32),                       # pairwise
                  np.cumsum(prods, axis=1, dtype=np.float32)[:, -1]):  # sequential
            approx = s.astype(np.float64) * A.astype(np.float64)
            err = np.abs(S[fin] - approx[fin])
            lim = a[fin].astype(np.float64) * Q + PAD_ABS
            assert np.all(err <= lim), float((err / lim).max())


def test_bound_is_tight_enough_on_unit_rows(oracle):
    """a unit Gaussian row's a_r is its quantisation error, ~0.0072 at dim 512: the width that lets ~10^3 of 10^8
    synthetic rows survive"""
    X = oracle.synth_rows(5, 0, 2000, DIM)
    _, _, a = shadow(X)
    assert 0.005 < float(np.median(a)) < 0.0095
