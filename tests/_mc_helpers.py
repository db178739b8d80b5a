"""numpy statements of the large-batch top-k's fp16 path and of its error bound E (csrc/index_mc.hip, header), the input
families that strain them, and the ctypes wrapper of the lab hook ssw_debug_mc_candidates.  Shared by
tests/test_topk_mc_certificate_gpu.py, tests/test_topk_matrix_core_gpu.py and tests/test_topk_matrix_core_cpu.py; nothing
here calls the code under test except `hook`."""
import ctypes

import numpy as np

MC_CAP = 4096
MIN_ABS, MAX_ABS = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
# the kernel's constants (k_mc_finish, run_group) and the header's derived ones they round up
EPS_REL = {np.dtype(np.float32): 1.2e-3, np.dtype(np.float16): 6.5e-4}
EPS_REL_DERIVED = {np.dtype(np.float32): 2.0 ** -10 + 2.0 ** -13 + 2.0 ** -20 + 3 * 2.0 ** -22,
                   np.dtype(np.float16): 2.0 ** -11 + 2.0 ** -13 + 2.0 ** -20}


def strip_rows(dim):
    return 128 if dim <= 512 else 64


def pow2_scale(maxabs):
    """the power of two with scale * maxabs in [128, 256)"""
    return float(np.ldexp(1.0, 8 - int(np.frexp(np.float32(maxabs))[1])))


def stored(X, dtype):
    """the f32 rows an index of storage `dtype` holds for X"""
    X = np.asarray(X)
    if np.dtype(dtype) == np.float16:
        return X.astype(np.float16).astype(np.float32)
    return np.ascontiguousarray(X, dtype=np.float32)


def fp16_operands(Xs, Q):
    """-> (scale, scale_q, ah [n, D], ch [nq, D]): the operands of the matrix cores in float64 -- the stored rows and the
    queries, scaled by their powers of two in f32 (exact) and rounded once to binary16, as the kernels convert them"""
    Xs, Q = np.asarray(Xs, dtype=np.float32), np.asarray(Q, dtype=np.float32)
    scale, scale_q = pow2_scale(np.max(np.abs(Xs))), pow2_scale(np.max(np.abs(Q)))
    ah = (Xs * np.float32(scale)).astype(np.float16).astype(np.float64)
    ch = (Q * np.float32(scale_q)).astype(np.float16).astype(np.float64)
    return scale, scale_q, ah, ch


def fp16_path(Xs, Q):
    """-> (scale, scale_q, S16 [nq, n] float64 = ch @ ah.T, the product of the operand norms [nq, n])"""
    scale, scale_q, ah, ch = fp16_operands(Xs, Q)
    norms = np.sqrt((ch * ch).sum(1))[:, None] * np.sqrt((ah * ah).sum(1))[None, :]
    return scale, scale_q, ch @ ah.T, norms


def accumulation_bound(norms, dim):
    """the header's accumulation term: D 2^-23 |ah| |ch|"""
    return dim * 2.0 ** -23 * norms


def derived_E(Xs, Q, dtype):
    """E per (query, row) [nq, n] as the header derives it, in float64, with each row's and query's own norm:
    c1 |x||q| + 2^-16 (1 + 2^-11) (|x| maxabs_q + |q| maxabs_x) + 2^-32 maxabs_x maxabs_q, c1 per storage dtype"""
    X, Qd = np.asarray(Xs, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    nx, nq = np.sqrt((X * X).sum(1))[None, :], np.sqrt((Qd * Qd).sum(1))[:, None]
    mx, mq = np.max(np.abs(X)), np.max(np.abs(Qd))
    return EPS_REL_DERIVED[np.dtype(dtype)] * nx * nq + 2.0 ** -16 * (1 + 2.0 ** -11) * (nx * mq + nq * mx) + 2.0 ** -32 * mx * mq


def kernel_E(Xs, Q, dtype):
    """E per query [nq] with the kernel's constants and the largest row norm, in float64 (the device evaluates the same
    expression in f32 from norms it rounds up, so its E is this one within a few 1e-4 relative, never 6 % below)"""
    X, Qd = np.asarray(Xs, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    maxnorm, nq = np.sqrt((X * X).sum(1)).max(), np.sqrt((Qd * Qd).sum(1))
    mx, mq = np.max(np.abs(X)), np.max(np.abs(Qd))
    return EPS_REL[np.dtype(dtype)] * nq * maxnorm + 1.6e-5 * (maxnorm * mq + nq * mx) + 1e-9 * mx * mq


# ---- input families: f(n, nq, dim, rng) -> (X, Q); X float32 or float16 rows before storage, Q float32 ------------------
def _gauss(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def gaussian(n, nq, dim, rng):
    """unit Gaussian rows and queries: the baseline, where E has three orders of magnitude of slack"""
    return _gauss(rng, n, dim), _gauss(rng, nq, dim)


def _spike(n, nq, dim, rng, e):
    X, Q = _gauss(rng, n, dim), _gauss(rng, nq, dim)
    X[n // 2, dim // 3] = np.float32(2.0 ** e)
    return X, Q


def spike_2_10(n, nq, dim, rng):
    """one element of one row is 2^10 times the rest: the scale follows it and every other element sits ~2^-3 with
    11 bits, the operand rounding term against the maxabs terms of E"""
    return _spike(n, nq, dim, rng, 10)


def spike_2_20(n, nq, dim, rng):
    """one element 2^20 times the rest: the other elements land around 2^-13 after scaling, subnormal in binary16 or
    flushed -- the absolute 2^-14 term of the bound carries nearly the whole index"""
    return _spike(n, nq, dim, rng, 20)


def query_ladder(n, nq, dim, rng):
    """the queries of one group scaled by 2^-30 ... 2^0: scale_q follows the largest, the small queries are subnormal or
    zero in fp16 and their E (maxabs_q terms) exceeds any score they can have"""
    X, Q = _gauss(rng, n, dim), _gauss(rng, nq, dim)
    expo = np.round(np.linspace(-30, 0, nq)) if nq > 1 else np.zeros(1)
    return X, Q * np.ldexp(np.float32(1), expo.astype(np.int32))[:, None].astype(np.float32)


def near_duplicates(n, nq, dim, rng):
    """a few hundred rows = one base row + 2^-12 noise, and queries near the base row, so the duplicates are on top:
    their f32 scores differ below the fp16 path's resolution and its order is another one"""
    X, Q = _gauss(rng, n, dim), _gauss(rng, nq, dim)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    base = X[0].copy()
    m = min(n, 300)
    X[:m] = base + np.float32(2.0 ** -12) * _gauss(rng, m, dim)
    Q = base + np.float32(0.05) * Q
    return X, Q.astype(np.float32)


def all_negative(n, nq, dim, rng):
    """every score negative: thresholds and b below zero, -inf initial thresholds against negative accumulators, and zero
    padding rows / queries (score 0) would beat every real row if one were appended"""
    return -np.abs(_gauss(rng, n, dim)), np.abs(_gauss(rng, nq, dim))


def zeros(n, nq, dim, rng):
    """zero rows in the index (every odd row; score exactly 0 among positive and negative ones) and one zero query
    among non-zero ones (its scores all tie at 0: it can only be proven when its list holds every row)"""
    X, Q = _gauss(rng, n, dim), _gauss(rng, nq, dim)
    X[1::2] = 0
    if nq > 1:
        Q[nq // 2] = 0
    return X, Q


def f16_range(n, nq, dim, rng):
    """binary16 rows whose exponents span the whole format, 65504 and subnormals included: after scaling by
    2^-8 most elements are subnormal or zero in fp16"""
    expo = rng.integers(-24, 16, (n, dim))
    X = (np.ldexp(1.0 + rng.integers(0, 1024, (n, dim)) / 1024.0, expo) * rng.choice([-1.0, 1.0], (n, dim))).astype(np.float16)
    X[0, 0] = np.float16(65504)
    X[n // 2, 1] = np.float16(2.0 ** -24)
    return X, _gauss(rng, nq, dim)


def rows_x1000(n, nq, dim, rng):
    """rows 1000 times larger: scale < 1 (the other side of the scale's exponent from unit rows)"""
    return _gauss(rng, n, dim) * np.float32(1000), _gauss(rng, nq, dim)


def rows_tiny(n, nq, dim, rng):
    """rows times 2^-30 (a scale of ~2^36; f32 rows) -- as float16 rows that would be all zeros, so those are times
    2^-12 instead, half of them subnormal in storage already"""
    return _gauss(rng, n, dim) * np.float32(2.0 ** -30), _gauss(rng, nq, dim)


def _pinned_max(G, value):
    """G rescaled so that its largest |element| is exactly `value`"""
    G = (G / np.max(np.abs(G))).astype(np.float32)
    return G * np.float32(value)


def rows_edge_low(n, nq, dim, rng):
    """the largest row element exactly 2^-40, the smallest the route bounds (f32 rows)"""
    return _pinned_max(_gauss(rng, n, dim), MIN_ABS), _gauss(rng, nq, dim)


def rows_edge_high(n, nq, dim, rng):
    """the largest row element exactly 2^40, the largest the route bounds (f32 rows)"""
    return _pinned_max(_gauss(rng, n, dim), MAX_ABS), _gauss(rng, nq, dim)


def queries_edge_low(n, nq, dim, rng):
    """the group's largest query element exactly 2^-40"""
    return _gauss(rng, n, dim), _pinned_max(_gauss(rng, nq, dim), MIN_ABS)


def queries_edge_high(n, nq, dim, rng):
    """the group's largest query element exactly 2^40"""
    return _gauss(rng, n, dim), _pinned_max(_gauss(rng, nq, dim), MAX_ABS)


FAMILIES = (gaussian, spike_2_10, spike_2_20, query_ladder, near_duplicates, all_negative, zeros, f16_range, rows_x1000,
            rows_tiny, rows_edge_low, rows_edge_high, queries_edge_low, queries_edge_high)
F32_ONLY = (rows_edge_low, rows_edge_high)  # binary16 holds neither 2^-40 nor 2^40


def make(family, n, nq, dim, dtype, seed=0):
    """-> (X as uploaded, Xs = the f32 rows the index holds, Q) of a family at a shape; deterministic"""
    rng = np.random.default_rng([seed, n, nq, dim])
    X, Q = family(n, nq, dim, rng)
    if family is rows_tiny and np.dtype(dtype) == np.float16:
        X = X * np.float32(2.0 ** 18)
    if family is spike_2_20 and np.dtype(dtype) == np.float16:
        X = X * np.float32(2.0 ** -5)  # 2^20 is past binary16: the same ratio with the spike at 2^15
    X =np.ascontiguousarray(X if X.dtype == np.float16 else X.astype(np.float32))
    return X, stored(X, dtype), np.ascontiguousarray(Q, dtype=np.float32)


def outside(which, low, n, nq, dim, rng):
    """rows (`which` = "rows") or queries whose largest element lies one f32 step outside [2^-40, 2^40]"""
    X, Q = _gauss(rng, n, dim), _gauss(rng, nq, dim)
    value = np.nextafter(MIN_ABS, np.float32(0)) if low else np.nextafter(MAX_ABS, np.float32(np.inf))
    if which == "rows":
        X = _pinned_max(X, 1.0) * value
        assert np.max(np.abs(X)) == value
    else:
        Q = _pinned_max(Q, 1.0) * value
        assert np.max(np.abs(Q)) == value
    return X.astype(np.float32), Q.astype(np.float32)


# ---- the hook ---------------------------------------------------------------------------------------------------------
def hook(lib, dev, Q, k, mode):
    """ssw_debug_mc_candidates on the lab build `lib` -> dict(meta..., levels, perm, thr, cnt, scores, rows, flags, b, E);
    scores / rows are lists of per-query arrays cut to the entries the device holds"""
    from seesaw_amd import _lib
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq = Q.shape[0]
    M = 64
    while M < 4 * k:
        M <<= 1
    stride = MC_CAP if mode == 1 else M
    strips = -(-dev.n_rows // strip_rows(dev.dim))
    meta, levels, n_levels = np.zeros(6, np.float32), np.zeros(64, np.int64), ctypes.c_int32(0)
    perm, thr, cnt = np.zeros(strips, np.int32), np.zeros(nq, np.float32), np.zeros(nq, np.uint32)
    scores, rows = np.full((nq, stride), np.nan, np.float32), np.full((nq, stride), -1, np.int64)
    flags, bE = np.full(nq, -1, np.int32), np.full((nq, 2), np.nan, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(lib.ssw_debug_mc_candidates(dev._h, p(Q), nq, k, mode, p(meta), p(levels), levels.shape[0],
                                           ctypes.byref(n_levels), p(perm), p(thr), p(cnt), p(scores), p(rows), p(flags), p(bE)))
    held = np.minimum(cnt, stride).astype(np.int64)
    return dict(scale=float(meta[0]), scale_q=float(meta[1]), maxabs_x=float(meta[2]), maxnorm=float(meta[3]),
                maxabs_q=float(meta[4]), M=int(meta[5]), levels=levels[:n_levels.value].copy(), perm=perm, thr=thr, cnt=cnt,
                scores=[scores[b, :held[b]] for b in range(nq)], rows=[rows[b, :held[b]] for b in range(nq)],
                flags=flags, b=bE[:, 0].copy(), E=bE[:, 1].copy())
