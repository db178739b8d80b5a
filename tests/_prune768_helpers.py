"""Test infrastructure of the packed 6-bit shadow at dim 768 (tests/test_prune768_cpu.py, tests/test_prune768_gpu.py).
The placement, the builder's twin, the integer sums and the query's twin are the dim-free ones of _prune6_helpers; what
knows the dim is the code norm (csrc/prune.hip, q6_code_norm), so the width and the lower bound are formed here with the
dim-768 constant (the older `width6` has no entry for it).  Never imported by the product."""
import ctypes

import numpy as np

from _prune6_helpers import (INFLATE, hook_bounds6, hook_shadow6, integer_sums, launch_shape6, mode6,  # noqa: F401
                             pack, quantise_query, shadow6, tile_bytes, unpack)  # (re-exported)
from _prune_helpers import PAD_ABS

DIM = 768
ROW_BYTES = DIM * 3 // 4 + 8  # of the shadow: 576 bytes of codes, s6 and a6
CODE_NORM_768 = 859.0972006   # the kernel's constant >= 31 sqrt(768) = 859.09720055...


def code_norm(dim):
    """the kernel's constant >= 31 sqrt(dim)"""
    return {256: 496.0, 512: 701.4499270, 768: CODE_NORM_768, 1024: 992.0}[dim]


def shadow_bytes(n, dim=DIM):
    """device memory of the 6-bit shadow: whole 16-row tiles of 3 dim / 4 code bytes and two floats a row"""
    return (n + 15) // 16 * 16 * (dim * 3 // 4 + 8)


def width6(s, a, qq, dim=DIM):
    """w of DESIGN.md section 4, "6-bit shadow", as the kernels form it, in float64"""
    wQ = np.float64(qq["Q"]) * INFLATE
    wE = np.float64(qq["e"]) * code_norm(dim) * INFLATE
    with np.errstate(invalid="ignore"):
        return np.asarray(a, dtype=np.float64) * wQ + np.asarray(s, dtype=np.float64) * wE


def batch6(min_rows):
    """the batch's own 6-bit threshold (ssw_tune_prune6_batch); < 0: the product's constants"""
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune6_batch", int(min_rows))


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def launch_shape6_mq(idx):
    """(four-wave blocks, 16-row tiles of one request) of the next k_q6_bounds_mq launch over idx"""
    from seesaw_amd import _lib
    b, t = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune6_scan_mq_shape", idx._h, ctypes.byref(b), ctypes.byref(t))
    return int(b.value), int(t.value)


def hook_bounds6_mq(idx, Q, sums=True):
    """k_q6_query_mq + k_q6_bounds_mq: dict(I int64 [nq, n] (or None), lb f32 [nq, n], Q, e, t2 f32 [nq], bad bool [nq],
    codes int8 [nq, 2, dim])"""
    from seesaw_amd import _lib
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq, n = Q.shape[0], idx.n_rows
    I = np.empty((nq, n), np.int64) if sums else None
    lb, qe = np.empty((nq, n), np.float32), np.empty((nq, 4), np.float32)
    codes = np.empty((nq, 2, idx.dim), np.int8)
    _lib.call("ssw_debug_prune6_bounds_mq", idx._h, _p(Q), nq, _p(I), _p(lb), _p(qe), _p(codes))
    return dict(I=I, lb=lb, Q=qe[:, 0].copy(), e=qe[:, 1].copy(), t2=qe[:, 2].copy(), bad=qe[:, 3] != 0, codes=codes)


def lower_bound6(c, s, a, qq):
    """twin of k_q6_bounds: (lb f32 [n] rounded down, w f64 [n], I int64 [n])"""
    dim = c.shape[1]
    I = integer_sums(c, qq)
    w = width6(s, a, qq, dim)
    with np.errstate(invalid="ignore"):
        lb = np.asarray(s, dtype=np.float64) * (np.float64(qq["t2"]) * 0.25) * I.astype(np.float64) - w
        lb = lb - (np.abs(lb) * 2.0 ** -50 + PAD_ABS)
        l32 = lb.astype(np.float32)
        l32 = np.where(l32.astype(np.float64) > lb, np.nextafter(l32, np.float32(-np.inf)), l32)
    return l32.astype(np.float32), w, I
