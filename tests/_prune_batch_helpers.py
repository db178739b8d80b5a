"""Test infrastructure of the pruned batch (tests/test_prune_batch_cpu.py, tests/test_prune_batch_gpu.py): the numpy twin
of the query quantisation (csrc/prune.hip, k_q8_query_mq) and of the bounds (k_q8_bounds_mq, k_survivors_mq), edge
queries, and the lab hooks' wrappers.  Never imported by the product."""
import ctypes

import numpy as np

from _prune_helpers import PAD_ABS, SAFETY  # noqa: F401  (PAD_ABS re-exported)

INFLATE = 1 + 2.0 ** -40
MQ_WIDTH = 16


def code_norm(dim):
    """the kernel's constant >= 127 sqrt(dim)"""
    return {256: 2032.0, 512: 2873.6819588, 1024: 4064.0}[dim]


def _round_up_f32(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < float(v) else f


def _block_sum(vals):
    """the double sum of one 256-thread block: thread t adds elements t, t + 256, ... in order, a wave sums by xor
    butterfly, thread 0 adds the four waves' sums in order"""
    vals = np.asarray(vals, dtype=np.float64)
    per = np.zeros(256, dtype=np.float64)
    for i in range(0, vals.shape[0], 256):
        per = per + vals[i:i + 256]
    waves = per.reshape(4, 64)
    lanes = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        waves = waves + waves[:, lanes ^ off]
    p = waves[:, 0]
    return ((p[0] + p[1]) + p[2]) + p[3]


def quantise_query(q):
    """numpy twin of k_q8_query_mq for one query: dict(d_hi int8 [dim], d_lo int8 [dim], Q, e, t2 (f32), bad)"""
    q = np.asarray(q, dtype=np.float32)
    dim = q.shape[0]
    finite = bool(np.all(np.isfinite(q)))
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.float32(np.max(np.abs(np.where(np.isnan(q), np.float32(0), q))))  # fmaxf ignores a NaN
        qd = q.astype(np.float64)
        Q = _round_up_f32(np.sqrt(_block_sum(qd * qd)) * INFLATE) if finite else np.float32(np.nan)
    bad = (not finite) or not (Q <= np.float32(2.0 ** 40)) or Q == 0 or not (np.float32(2.0 ** -60) <= m <= np.float32(2.0 ** 60))
    hi, lo = np.zeros(dim, dtype=np.int8), np.zeros(dim, dtype=np.int8)
    if bad:
        return dict(d_hi=hi, d_lo=lo, Q=Q, e=np.float32(0), t2=np.float32(0), bad=True, t=np.float32(0))
    t = np.float32(m / np.float32(127))
    t2 = np.float32(t * np.float32(2.0 ** -8))
    dh = np.rint(qd / np.float64(t))
    r1 = qd - np.float64(t) * dh
    dl = np.clip(np.rint(r1 / np.float64(t2)), -127.0, 127.0)
    r2 = r1 - np.float64(t2) * dl
    e = _round_up_f32(np.sqrt(_block_sum(r2 * r2)) * SAFETY)
    assert np.abs(dh).max() <= 127
    return dict(d_hi=dh.astype(np.int8), d_lo=dl.astype(np.int8), Q=Q, e=e, t2=t2, bad=False, t=t)


def width(s, a, qq, dim):
    """w of DESIGN.md section 4, "Pruned batch", as the kernels form it, in float64"""
    wQ = np.float64(qq["Q"]) * INFLATE
    wE = np.float64(qq["e"]) * code_norm(dim) * INFLATE
    with np.errstate(invalid="ignore"):
        return np.asarray(a, dtype=np.float64) * wQ + np.asarray(s, dtype=np.float64) * wE


def lower_bound(c, s, a, qq):
    """twin of k_q8_bounds_mq for one query: (lb f32 [n] rounded down, w f64 [n], I_hi, I_lo int64 [n])"""
    dim = c.shape[1]
    ci = c.astype(np.int64)
    I_hi, I_lo = ci @ qq["d_hi"].astype(np.int64), ci @ qq["d_lo"].astype(np.int64)
    w = width(s, a, qq, dim)
    with np.errstate(invalid="ignore"):
        lb = np.asarray(s, dtype=np.float64) * np.float64(qq["t2"]) * (256.0 * I_hi + I_lo) - w
        lb = lb - (np.abs(lb) * 2.0 ** -50 + PAD_ABS)
        l32 = lb.astype(np.float32)
        l32 = np.where(l32.astype(np.float64) > lb, np.nextafter(l32, np.float32(-np.inf)), l32)
    return l32.astype(np.float32), w, I_hi, I_lo


def upper_bound(lb, w):
    """k_survivors_mq's ub from a lower bound, float64 (NaN where a = +inf: such a row always survives)"""
    l = np.asarray(lb, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return l + 2.0 * w + (np.abs(l) + w) * 2.0 ** -20 + 2.0 * PAD_ABS


def edge_queries(rng, dim):
    """boundable queries that strain the quantisation: one huge element; all equal; every element on a rint tie of the
    hi plane (q / t = k + 1/2: the residual is 128 t2 and the lo code clamps at +-127); residuals just inside the
    clamp; subnormal elements beside normal ones; a tiny and a large norm"""
    big = rng.standard_normal(dim)
    big[3] = 1e6
    ties = rng.integers(-126, 126, dim) + 0.5
    ties[0] = 127.0  # t = 1 exactly
    near = rng.integers(-126, 126, dim) + rng.choice([-0.4999, 0.4999, 0.4961, -0.4961], dim)
    near[0] = 127.0
    sub = rng.standard_normal(dim)
    sub[::3] = rng.standard_normal((dim + 2) // 3) * 1e-39
    return [np.asarray(v, dtype=np.float32) for v in
            (big, np.full(dim, 0.37), np.full(dim, -3.0), ties, near, sub, rng.standard_normal(dim) * 1e-15,
             rng.standard_normal(dim) * 2.0 ** 30)]


def flagged_queries(dim):
    """queries that cannot be bounded: zero, NaN, +inf, norm above 2^40, largest element below 2^-60"""
    nan, inf = np.ones(dim, np.float32), np.ones(dim, np.float32)
    nan[dim // 2], inf[5] = np.nan, np.inf
    return [np.zeros(dim, np.float32), nan, inf, np.full(dim, 2.0 ** 37, np.float32),
            np.full(dim, 2.0 ** -70, np.float32)]


def thresholds(ub):
    """f32 thresholds between two neighbouring upper bounds that lie clearly apart (the device may contract the formula's
    products and sums), keeping none, one, a few and all of the finite ones"""
    u = np.sort(ub[np.isfinite(ub)])[::-1]
    if u.size == 0:
        return [np.float32(0)]
    out = [np.float32(2) * np.float32(abs(u[0])) + np.float32(1)]
    for keep in (1, 5, 37):
        if u.size > keep:
            hi, lo = u[keep - 1], u[keep]
            t = np.float32((hi + lo) / 2)
            if lo < float(t) < hi and (hi - lo) > 1e-6 * max(abs(hi), abs(lo)):
                out.append(t)
    out.append(np.float32(-2) * np.float32(np.abs(u).max()) - np.float32(1))
    return out


# ---- lab hooks (include/seesaw_hip_debug.h) --------------------------------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def launch_shape(idx):
    """(four-wave blocks, 16-row tiles of one request) of the next k_q8_bounds_mq launch over idx"""
    from seesaw_amd import _lib
    b, t = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune_scan_mq_shape", idx._h, ctypes.byref(b), ctypes.byref(t))
    return int(b.value), int(t.value)


def hook_bounds_mq(idx, Q, sums=True):
    """k_q8_query_mq + k_q8_bounds_mq: dict(I_hi, I_lo int32 [nq, n] (or None), lb f32 [nq, n], Q, e, t2 f32 [nq],
    bad bool [nq], codes int8 [nq, 2, dim])"""
    from seesaw_amd import _lib
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq, n = Q.shape[0], idx.n_rows
    hi = np.empty((nq, n), np.int32) if sums else None
    lo = np.empty((nq, n), np.int32) if sums else None
    lb, qe = np.empty((nq, n), np.float32), np.empty((nq, 4), np.float32)
    codes = np.empty((nq, 2, idx.dim), np.int8)
    _lib.call("ssw_debug_prune_bounds_mq", idx._h, _p(Q), nq, _p(hi), _p(lo), _p(lb), _p(qe), _p(codes))
    return dict(I_hi=hi, I_lo=lo, lb=lb, Q=qe[:, 0].copy(), e=qe[:, 1].copy(), t2=qe[:, 2].copy(), bad=qe[:, 3] != 0,
                codes=codes)


def hook_survivors_mq(idx, nq, slot, threshold, k, sel_count=None, sel_overflow=0, cap=1 << 18):
    """k_survivors_mq of one slot + k_prune_publish_mq: (published, collected, rows int64)"""
    from seesaw_amd import _lib
    rows = np.full(max(int(cap), 1), -1, dtype=np.int64)
    pub, got = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.call("ssw_debug_prune_survivors_mq", idx._h, int(nq), int(slot), ctypes.c_float(float(threshold)), int(k),
              int(k if sel_count is None else sel_count), int(sel_overflow), int(cap), ctypes.byref(pub),
              ctypes.byref(got), _p(rows))
    return int(pub.value), int(got.value), rows[:max(int(pub.value), 0)]
