"""Test infrastructure of the packed 6-bit shadow (tests/test_prune6_cpu.py, tests/test_prune6_gpu.py): the numpy twin
of the placement function (csrc/ssw_common.h, q6_slot / q6_word_offset), of the builder (csrc/prune.hip, k_q6_build) and
of the bound (k_q6_bounds, k_survivors_mq with the 6-bit code norm), and the lab hooks' wrappers.  The query's twin is the
pruned batch's (_prune_batch_helpers.quantise_query).  Never imported by the product."""
import ctypes

import numpy as np

from _prune_batch_helpers import INFLATE, quantise_query, upper_bound  # noqa: F401  (re-exported)
from _prune_helpers import PAD_ABS, SAFETY, gamma

LEVELS = 31


def code_norm(dim):
    """the kernel's constant >= 31 sqrt(dim)"""
    return {256: 496.0, 512: 701.4499270, 1024: 992.0}[dim]


# ---- placement: element i of row r -> the bytes of its code in the row's tile ---------------------------------------
def slot(i):
    """q6_slot: (k-step u, lane group g, slot j) of element i"""
    i = np.asarray(i)
    return i >> 6, (i & 63) >> 4, i & 15


def word_offset(lane, wi):
    """q6_word_offset: byte offset in the tile of word wi of a lane"""
    return (wi >> 2) * 1024 + lane * 16 + (wi & 3) * 4


def tile_bytes(dim):
    return 16 * dim * 3 // 4


def pack(codes):
    """codes int [n, dim], |c| <= 31 -> uint8 [ceil(n / 16), tile_bytes]: the device's buffer (pad rows zero)"""
    codes = np.asarray(codes, dtype=np.int64)
    n, dim = codes.shape
    out = np.zeros(((n + 15) // 16, tile_bytes(dim)), dtype=np.uint8)
    u, g, j = slot(np.arange(dim))
    r = np.arange(n)
    tile, lane = (r >> 4)[:, None], 16 * g[None, :] + (r & 15)[:, None]
    c6 = codes & 0x3f
    main = j < 12
    # slots 0 .. 11: the upper six bits of byte j % 4 of word 3 u + j / 4
    off = word_offset(lane[:, main], (3 * u[main] + j[main] // 4)[None, :]) + (j[main] % 4)[None, :]
    np.bitwise_or.at(out, (np.broadcast_to(tile, off.shape), off), (c6[:, main] << 2).astype(np.uint8))
    # slots 12 + b: code bits 5:4, 3:2, 1:0 in the low two bits of byte b of words 3 u, 3 u + 1, 3 u + 2
    for part in range(3):
        off = word_offset(lane[:, ~main], (3 * u[~main] + part)[None, :]) + (j[~main] - 12)[None, :]
        bits = ((c6[:, ~main] >> (4 - 2 * part)) & 3).astype(np.uint8)
        np.bitwise_or.at(out, (np.broadcast_to(tile, off.shape), off), bits)
    return out


def unpack(packed, n, dim):
    """the inverse: int8 [n, dim]"""
    u, g, j = slot(np.arange(dim))
    r = np.arange(n)
    tile, lane = (r >> 4)[:, None], 16 * g[None, :] + (r & 15)[:, None]
    out = np.zeros((n, dim), dtype=np.int64)
    main = j < 12
    off = word_offset(lane[:, main], (3 * u[main] + j[main] // 4)[None, :]) + (j[main] % 4)[None, :]
    out[:, main] = packed[np.broadcast_to(tile, off.shape), off].astype(np.int8).astype(np.int64) >> 2
    bits = np.zeros((n, int((~main).sum())), dtype=np.int64)
    for part in range(3):
        off = word_offset(lane[:, ~main], (3 * u[~main] + part)[None, :]) + (j[~main] - 12)[None, :]
        bits = (bits << 2) | (packed[np.broadcast_to(tile, off.shape), off].astype(np.int64) & 3)
    out[:, ~main] = (bits ^ 32) - 32
    return out.astype(np.int8)


def operand_words(packed_tile, lane, u):
    """what k_q6_bounds feeds the matrix core for k-step u of a lane: the 16 int8 values 4 c, from the tile's bytes"""
    w = [int.from_bytes(bytes(packed_tile[word_offset(lane, 3 * u + p):word_offset(lane, 3 * u + p) + 4]), "little")
         for p in range(3)]
    ops = [x & 0xfcfcfcfc for x in w]
    ops.append((((w[0] & 0x03030303) << 6) | ((w[1] & 0x03030303) << 4) | ((w[2] & 0x03030303) << 2)) & 0xffffffff)
    return np.frombuffer(b"".join(int(x).to_bytes(4, "little") for x in ops), dtype=np.int8).astype(np.int64)


# ---- the builder and the bound ---------------------------------------------------------------------------------------
def shadow6(X):
    """numpy twin of k_q6_build: (codes int8 [n, dim], s6 f32 [n], a6 f32 [n] rounded up); a6's double sums are taken
    in numpy's order, so the device's a6 is compared within a band (as the int8 test does)"""
    X = np.asarray(X, dtype=np.float32)
    g = gamma(X.shape[1])
    with np.errstate(invalid="ignore"):
        m = np.max(np.abs(X), axis=1)
    finite = np.all(np.isfinite(X), axis=1)
    ok = finite & ((m == 0) | ((m >= np.float32(2.0 ** -60)) & (m <= np.float32(2.0 ** 60))))
    s = np.where(ok & (m > 0), m / np.float32(LEVELS), np.float32(0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = np.where(s[:, None] > 0, np.rint(X / s[:, None]), 0.0)
    c = np.clip(np.nan_to_num(c), -LEVELS, LEVELS).astype(np.int8)
    Xd = np.where(ok[:, None], X, 0).astype(np.float64)
    e = Xd - s.astype(np.float64)[:, None] * c.astype(np.float64)
    a = SAFETY * (np.sqrt((e * e).sum(1)) + g * np.sqrt((Xd * Xd).sum(1))
                  + g * s.astype(np.float64) * np.sqrt((c.astype(np.float64) ** 2).sum(1)))
    a32 = a.astype(np.float32)
    a32 = np.where(a32.astype(np.float64) < a, np.nextafter(a32, np.float32(np.inf)), a32)  # round up
    return c, s, np.where(ok, a32, np.float32(np.inf)).astype(np.float32)


def width6(s, a, qq, dim):
    """w of DESIGN.md section 4, "6-bit shadow", as the kernels form it, in float64"""
    wQ = np.float64(qq["Q"]) * INFLATE
    wE = np.float64(qq["e"]) * code_norm(dim) * INFLATE
    with np.errstate(invalid="ignore"):
        return np.asarray(a, dtype=np.float64) * wQ + np.asarray(s, dtype=np.float64) * wE


def integer_sums(c, qq):
    """I_r = sum_i 4 c_ri (256 d_hi,i + d_lo,i), int64"""
    d = 256 * qq["d_hi"].astype(np.int64) + qq["d_lo"].astype(np.int64)
    return (4 * c.astype(np.int64)) @ d


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


# ---- lab hooks (include/seesaw_hip_debug.h) --------------------------------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def mode6(on, min_rows=-1):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune6", 1 if on else 0, int(min_rows))


def launch_shape6(idx):
    """(four-wave blocks, 16-row tiles of one request) of the next k_q6_bounds launch over idx"""
    from seesaw_amd import _lib
    b, t = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune6_scan_shape", idx._h, ctypes.byref(b), ctypes.byref(t))
    return int(b.value), int(t.value)


def hook_shadow6(idx, first_row=0, n_rows=None, codes=True):
    """(codes int8 [rows, dim] unpacked by the device library, or None; s6 f32 [rows]; a6 f32 [rows])"""
    from seesaw_amd import _lib
    m = idx.n_rows - first_row if n_rows is None else int(n_rows)
    c = np.empty((m, idx.dim), dtype=np.int8) if codes else None
    s, a = np.empty(m, dtype=np.float32), np.empty(m, dtype=np.float32)
    _lib.call("ssw_debug_prune6_shadow", idx._h, int(first_row), m, _p(c), _p(s), _p(a))
    return c, s, a


def hook_bounds6(idx, q, sums=True):
    """k_q6_query + k_q6_bounds: dict(I int64 [n] or None, lb f32 [n], Q, e, t2 f32, bad, codes int8 [2, dim])"""
    from seesaw_amd import _lib
    q = np.ascontiguousarray(q, dtype=np.float32)
    assert q.shape == (idx.dim,)
    n = idx.n_rows
    I = np.empty(n, np.int64) if sums else None
    lb, qe, codes = np.empty(n, np.float32), np.empty(4, np.float32), np.empty((2, idx.dim), np.int8)
    _lib.call("ssw_debug_prune6_bounds", idx._h, _p(q), _p(I), _p(lb), _p(qe), _p(codes))
    return dict(I=I, lb=lb, Q=qe[0], e=qe[1], t2=qe[2], bad=bool(qe[3] != 0), codes=codes)
