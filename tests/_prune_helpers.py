"""Test infrastructure shared by the pruned top-k's tests (tests/test_prune_cpu.py, tests/test_prune_gpu.py,
tests/test_prune_certificate_gpu.py): the numpy twin of the int8 shadow (csrc/prune.hip, k_q8_build), the adversarial
rows and edge queries, and the helpers that run one call with the pruning off and on.  Never imported by the product."""
import ctypes

import numpy as np

U = 2.0 ** -24
SAFETY = 1 + 2.0 ** -10
PAD_ABS = 2.0 ** -100


def gamma(dim):
    """gamma_dim of DESIGN.md section 4: any f32 summation of dim products"""
    return dim * U / (1 - dim * U)


def shadow(X):
    """numpy twin of k_q8_build: (codes int8 [n, dim], s f32 [n], a f32 [n], rounded up)"""
    X = np.asarray(X, dtype=np.float32)
    g = gamma(X.shape[1])
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
    a = SAFETY * (np.sqrt((e * e).sum(1)) + g * np.sqrt((Xd * Xd).sum(1))
                  + g * s.astype(np.float64) * np.sqrt((c.astype(np.float64) ** 2).sum(1)))
    a32 = a.astype(np.float32)
    a32 = np.where(a32.astype(np.float64) < a, np.nextafter(a32, np.float32(np.inf)), a32)  # round up
    return c, s, np.where(ok, a32, np.float32(np.inf)).astype(np.float32)


def adversarial_rows(rng, dim):
    """49 rows: 0-7 Gaussian, 8-15 one huge element, 16-18 all-equal, 19-21 subnormals beside normals, 22-23 zero,
    24-25 all subnormal, 26-28 +inf / -inf / NaN, 29-32 rint ties, 33-40 scaled by 2^50, 41-48 by 2^66.  Rows 24-28
    and 41-48 cannot be bounded (a = +inf)."""
    base = rng.standard_normal((8, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    huge = base.copy()
    huge[:, 3] = 40.0
    sub = base[:3].copy()  # subnormal f32 elements beside normal ones
    sub[:, ::3] = (rng.standard_normal((3, (dim + 2) // 3)) * 1e-39).astype(np.float32)
    tiny = (rng.standard_normal((2, dim)) * 1e-39).astype(np.float32)  # max |x| below 2^-60: unbounded
    bad = base[:3].copy()
    bad[0, 7], bad[1, 9], bad[2, 0] = np.inf, -np.inf, np.nan
    # elements exactly halfway between two quantisation steps (the rint tie), the max pinning the step
    half = ((rng.integers(-126, 126, (4, dim)) + 0.5) / 127.0).astype(np.float32)
    half[:, 0] = 1.0
    rows = [base, huge, np.full((2, dim), 0.0442, np.float32), np.full((1, dim), -3.0, np.float32), sub,
            np.zeros((2, dim), np.float32), tiny, bad, half, (base * np.float32(2.0 ** 50)).astype(np.float32),
            (base * np.float32(2.0 ** 66)).astype(np.float32)]  # the last 8: scale out of range, unbounded
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)


def queries(rng, X):
    """random, all ones, a multiple of row 8, zero, one component 1e6, norm ~1e-30"""
    dim = X.shape[1]
    big = rng.standard_normal(dim)
    big[3] = 1e6
    q = [rng.standard_normal(dim), np.ones(dim), X[8] * 7.0, np.zeros(dim), big, rng.standard_normal(dim) * 1e-30]
    return [np.asarray(v, dtype=np.float32) for v in q]


# ---- GPU side: one call with the pruning off and on (lab build) -----------------------------------------------------
def stats(idx):
    from seesaw_amd import _lib
    out = np.zeros(6, dtype=np.int64)
    _lib.call("ssw_index_prune_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return out


def mode(lib, on, min_rows=-1, reserve=-1):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune", 1 if on else 0, int(min_rows), int(reserve))


def query(seed, dim=512):
    q = np.random.default_rng(seed).standard_normal(dim).astype(np.float32)
    return (q / np.linalg.norm(q)).astype(np.float32)


def both(lib, idx, fn, min_rows=-1):
    """fn() with pruning off, then on: (full, pruned, stats after the pruned call)"""
    mode(lib, False)
    full = fn()
    mode(lib, True, min_rows)
    got = fn()
    st = stats(idx)
    mode(lib, True)
    return full, got, st


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (x[:8], y[:8])


# ---- the pre-scan's intermediate state (include/seesaw_hip_debug.h, ssw_debug_prune_*) ------------------------------
def hook_shadow(idx, first_row=0, n_rows=None, codes=True):
    """(codes int8 [rows, dim] or None, s f32 [rows], a f32 [rows]) of the shadow the device built"""
    from seesaw_amd import _lib
    m = idx.n_rows - first_row if n_rows is None else int(n_rows)
    c = np.empty((m, idx.dim), dtype=np.int8) if codes else None
    s, a = np.empty(m, dtype=np.float32), np.empty(m, dtype=np.float32)
    _lib.call("ssw_debug_prune_shadow", idx._h, int(first_row), m, None if c is None else ctypes.c_void_p(c.ctypes.data),
              ctypes.c_void_p(s.ctypes.data), ctypes.c_void_p(a.ctypes.data))
    return c, s, a


def hook_bounds(idx, q):
    """k_q8_query + k_q8_bounds: (lb f32 [n], Q f32, the state's "cannot be bounded" word)"""
    from seesaw_amd import _lib
    q = np.ascontiguousarray(q, dtype=np.float32)
    assert q.shape == (idx.dim,)
    lb = np.empty(idx.n_rows, dtype=np.float32)
    Q, bad = ctypes.c_float(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune_bounds", idx._h, ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(lb.ctypes.data),
              ctypes.byref(Q), ctypes.byref(bad))
    return lb, np.float32(Q.value), int(bad.value)


def hook_survivors(idx, threshold, k, sel_count=None, sel_overflow=0, cap=1 << 18):
    """k_survivors + k_prune_publish over the bounds of the last hook_bounds: (published, collected, rows int64)"""
    from seesaw_amd import _lib
    rows = np.full(max(int(cap), 1), -1, dtype=np.int64)
    pub, got = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.call("ssw_debug_prune_survivors", idx._h, ctypes.c_float(float(threshold)), int(k),
              int(k if sel_count is None else sel_count), int(sel_overflow), int(cap), ctypes.byref(pub),
              ctypes.byref(got), ctypes.c_void_p(rows.ctypes.data))
    return int(pub.value), int(got.value), rows[:max(int(pub.value), 0)]
