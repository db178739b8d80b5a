"""Test infrastructure of the two-stage 4 + 1-bit shadow (tests/test_prune41_cpu.py, tests/test_prune41_gpu.py): the
numpy twin of the placement function (csrc/ssw_common.h, q4_nibble over q6_slot / q6_word_offset), of the builder
(csrc/prune.hip, k_q41_build), of the coarse bound (k_q4_bounds) and of the fine bound (k_q41_refine), and the lab hooks'
wrappers.  The codes, s5 and a5 are the 5-bit twin's (_prune5_helpers.shadow5); the query's twin is the pruned batch's.
Never imported by the product."""
import ctypes
import functools

import numpy as np

from _prune5_helpers import (SURV_CAP, candidates, code_norm as code_norm5, exact_threshold, integer_sums,  # noqa: F401
                             lower_bound5, ord_key, shadow5, survivors, width5)
from _prune6_helpers import slot, word_offset
from _prune_batch_helpers import INFLATE, quantise_query, upper_bound  # noqa: F401  (re-exported)
from _prune_helpers import PAD_ABS, SAFETY, gamma

COARSE_CAP = 1 << 23
SURV_STAGE = 1024

E2E_QUERY_SEED = 11  # of the end-to-end GPU test's query; test_prune41_cpu.py checks its survivor counts on the twin


def gaussian(n, dim, seed):
    X = np.random.default_rng(seed).standard_normal((n, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(X)


@functools.lru_cache(maxsize=None)
def big_rows(dim):
    """the five edge rows of the 5-bit tests + 100 003 unit Gaussian rows (read-only: shared between the tests)"""
    from test_prune5_cpu import edge_rows  # (the rows of test_prune5_gpu.edge_rows: the same function, seed and values)
    X = np.ascontiguousarray(np.concatenate([edge_rows(dim), gaussian(100_003, dim, seed=dim)]))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def mid_rows(dim):
    """the first 20 008 of them: what the twin is run on in the GPU tests"""
    X = np.ascontiguousarray(big_rows(dim)[:20_008])
    X.setflags(write=False)
    return X


def positive_query(seed, dim):
    """a unit query without a negative element: sum D is as large as a unit query's gets, and a per-query offset of the
    coarse bound that is wrong by one sum D moves the bound by about its width (a Gaussian query's sum D: a twentieth)"""
    from _prune_helpers import query
    return np.abs(query(seed, dim))


def ulps_apart(a, b):
    """distance of two f32 arrays in units in the last place (their ordinal keys' difference)"""
    return np.abs(ord_key(a) - ord_key(b))


# the constants a mutation test changes on a copy (test_prune41_cpu.py)
TWIN = dict(offset=31, mid=15.5, swap_nibbles=False, a4_is_a5=False)


def code_norm4(dim, mid=15.5):
    """the kernel's constant >= 15.5 sqrt(dim)"""
    if mid == 15.5:
        return {512: 350.7249635, 1024: 496.0}[dim]
    return mid * np.sqrt(dim) * (1 + 2.0 ** -30)


def bytes41(n, dim):
    """both planes, s5, a5, a4 and H of the rows padded to whole tiles"""
    return (n + 15) // 16 * 16 * (dim * 5 // 8 + 16)


# ---- the split of a 5-bit code and the placement of its two parts -------------------------------------------------------
def split(c):
    """c in [-15, 15] -> (h in [0, 15], b in {0, 1}) with c == 2 h + b - 16"""
    u = np.asarray(c, dtype=np.int64) + 16
    return u >> 1, u & 1


def nibble(u, j, swap=False):
    """q4_nibble: (word, byte, shift) of slot j of k-step u among a lane's words"""
    shift = 4 * ((j >> 2) & 1)
    return 2 * u + (j >> 3), j & 3, (4 - shift) if swap else shift


def coarse_tile_bytes(dim):
    return 16 * dim // 2


def pack_coarse(h, swap=False):
    """h int [n, dim] in [0, 15] -> uint8 [ceil(n / 16), coarse_tile_bytes]: the device's buffer (pad rows zero)"""
    h = np.asarray(h, dtype=np.int64)
    n, dim = h.shape
    out = np.zeros(((n + 15) // 16, coarse_tile_bytes(dim)), dtype=np.uint8)
    r = np.arange(n)
    tile, row = r >> 4, 16 * (r & 15)
    u, g, j = slot(np.arange(dim))
    for i in range(dim):
        word, byte, shift = nibble(int(u[i]), int(j[i]), swap)
        out[tile, word_offset(16 * int(g[i]), word) + byte + row] |= (h[:, i] << shift).astype(np.uint8)
    return out


def unpack_coarse(packed, n, dim):
    r = np.arange(n)
    tile, row = r >> 4, 16 * (r & 15)
    u, g, j = slot(np.arange(dim))
    out = np.zeros((n, dim), dtype=np.int64)
    for i in range(dim):
        word, byte, shift = nibble(int(u[i]), int(j[i]))
        out[:, i] = (packed[tile, word_offset(16 * int(g[i]), word) + byte + row].astype(np.int64) >> shift) & 15
    return out


def operand_bytes(packed_tile, lane, ks):
    """what k_q4_bounds feeds the matrix core for k-step ks of a lane: the 16 bytes of its four operand words"""
    w = [int.from_bytes(bytes(packed_tile[word_offset(lane, 2 * ks + t):word_offset(lane, 2 * ks + t) + 4]), "little")
         for t in range(2)]
    ops = [w[0] & 0x0f0f0f0f, (w[0] >> 4) & 0x0f0f0f0f, w[1] & 0x0f0f0f0f, (w[1] >> 4) & 0x0f0f0f0f]
    return np.frombuffer(b"".join(int(x).to_bytes(4, "little") for x in ops), dtype=np.uint8).astype(np.int64)


def pack_fine(b):
    """b int [n, dim] in {0, 1} -> uint32 [n, dim / 32]: bit i & 31 of word i >> 5 is b of element i"""
    b = np.asarray(b, dtype=np.uint64)
    n, dim = b.shape
    sh = np.arange(32, dtype=np.uint64)
    return (b.reshape(n, dim // 32, 32) << sh).sum(axis=2).astype(np.uint32)


def unpack_fine(words, dim):
    w = np.asarray(words, dtype=np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], dim).astype(np.int64)


# ---- the builder and the two bounds ---------------------------------------------------------------------------------
def shadow41(X, twin=TWIN):
    """numpy twin of k_q41_build: (h [n, dim], b [n, dim], s5, a5, a4); a4 is a5's expression with 2 h - mid in the code's
    place, its double sums in numpy's order (compared within a band, as a5 is)"""
    X = np.asarray(X, dtype=np.float32)
    c, s, a5 = shadow5(X)
    h, b = split(c)
    g = gamma(X.shape[1])
    ok = np.isfinite(a5)
    Xd = np.where(ok[:, None], X, 0).astype(np.float64)
    mid = 2.0 * h.astype(np.float64) - twin["mid"]
    e = Xd - s.astype(np.float64)[:, None] * mid
    a = SAFETY * (np.sqrt((e * e).sum(1)) + g * np.sqrt((Xd * Xd).sum(1)) + g * s.astype(np.float64) * np.sqrt((mid * mid).sum(1)))
    a32 = a.astype(np.float32)
    a32 = np.where(a32.astype(np.float64) < a, np.nextafter(a32, np.float32(np.inf)), a32)  # round up
    a4 = np.where(ok, a32, np.float32(np.inf)).astype(np.float32)
    return h, b, s, a5, (a5 if twin["a4_is_a5"] else a4)


def dvec(qq):
    return 256 * qq["d_hi"].astype(np.int64) + qq["d_lo"].astype(np.int64)


def sums41(h, b, qq):
    """(H, B, sum D): H_r = sum_i h_ri D_i, B_r = sum_i b_ri D_i, int64"""
    d = dvec(qq)
    return np.asarray(h, dtype=np.int64) @ d, np.asarray(b, dtype=np.int64) @ d, int(d.sum())


def width4(s, a4, qq, dim, twin=TWIN):
    wQ = np.float64(qq["Q"]) * INFLATE
    wE = np.float64(qq["e"]) * code_norm4(dim, twin["mid"]) * INFLATE
    with np.errstate(invalid="ignore"):
        return np.asarray(a4, dtype=np.float64) * wQ + np.asarray(s, dtype=np.float64) * wE


def _certified(sd, t2q, I, w):
    with np.errstate(invalid="ignore"):
        lb = sd * t2q * I.astype(np.float64) - w
        lb = lb - (np.abs(lb) * 2.0 ** -50 + PAD_ABS)
        l32 = lb.astype(np.float32)
        l32 = np.where(l32.astype(np.float64) > lb, np.nextafter(l32, np.float32(-np.inf)), l32)
    return l32.astype(np.float32)


def lower_bound4(h, s, a4, qq, twin=TWIN):
    """twin of k_q4_bounds: (lb4 f32 [n] rounded down, w4 f64 [n], H int64 [n])"""
    dim = np.asarray(h).shape[1]
    H, _, sumD = sums41(h, np.zeros_like(h), qq)
    J = 4 * H - twin["offset"] * sumD
    w = width4(s, a4, qq, dim, twin)
    return _certified(np.asarray(s, dtype=np.float64), np.float64(qq["t2"]) * 0.5, J, w), w, H


def lower_bound5_from_parts(H, B, sumD, s, a5, qq, dim):
    """twin of k_q41_refine's bound: (lb5 f32, w5 f64, I int64) with I = 8 (2 H + B - 16 sum D)"""
    I = 8 * (2 * np.asarray(H, dtype=np.int64) + np.asarray(B, dtype=np.int64) - 16 * sumD)
    w = width5(s, a5, qq, dim)
    return _certified(np.asarray(s, dtype=np.float64), np.float64(qq["t2"]) * 0.125, I, w), w, I


# ---- lab hooks (include/seesaw_hip_debug.h) --------------------------------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def mode41(on, min_rows=-1, coarse_cap=-1):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune41", 1 if on else 0, int(min_rows), int(coarse_cap))


def tune_scan41(blocks_per_cu, tiles):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune41_scan", int(blocks_per_cu), int(tiles))


def launch_shape41(idx):
    from seesaw_amd import _lib
    b, t = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune41_scan_shape", idx._h, ctypes.byref(b), ctypes.byref(t))
    return int(b.value), int(t.value)


def coarse_stats(idx):
    """[first-stage survivors of the last call, dense refines so far, two-stage calls so far]"""
    from seesaw_amd import _lib
    out = np.zeros(3, dtype=np.int64)
    _lib.call("ssw_index_prune_coarse_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return out


def hook_shadow41(idx, planes=True):
    """(h uint8 [n, dim] or None, fine uint32 [n, dim / 32] or None, s5, a5, a4)"""
    from seesaw_amd import _lib
    n, dim = idx.n_rows, idx.dim
    h = np.empty((n, dim), dtype=np.uint8) if planes else None
    fine = np.empty((n, dim // 32), dtype=np.uint32) if planes else None
    s, a5, a4 = (np.empty(n, dtype=np.float32) for _ in range(3))
    _lib.call("ssw_debug_prune41_shadow", idx._h, 0, n, _p(h), _p(fine), _p(s), _p(a5), _p(a4))
    return h, fine, s, a5, a4


def hook_stage1(idx, q):
    """k_q41_query + k_q4_bounds: dict(H int32 [n], lb f32 [n], Q, e, t2, bad, sumD (hi, lo))"""
    from seesaw_amd import _lib
    q = np.ascontiguousarray(q, dtype=np.float32)
    n = idx.n_rows
    H, lb, qe, sd = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(4, np.float32), np.empty(2, np.int32)
    _lib.call("ssw_debug_prune41_stage1", idx._h, _p(q), _p(H), _p(lb), _p(qe), _p(sd))
    return dict(H=H, lb=lb, Q=qe[0], e=qe[1], t2=qe[2], bad=bool(qe[3] != 0), sumD=(int(sd[0]), int(sd[1])))


def hook_survivors1(idx, threshold, k, blocks=0):
    """k_survivors_q4 over the bounds of the last hook_stage1: (count, rows uint32 [min(count, 2^23)])"""
    from seesaw_amd import _lib
    rows = np.empty(idx.n_rows, dtype=np.uint32)
    cnt = ctypes.c_int64(0)
    _lib.call("ssw_debug_prune41_survivors1", idx._h, ctypes.c_float(float(threshold)), int(k), int(blocks), rows.size,
              ctypes.byref(cnt), _p(rows))
    return int(cnt.value), rows[:min(int(cnt.value), rows.size)]


def hook_refine(idx, rows, threshold, k, dense=False):
    """k_q41_refine over `rows` (uint32, repeats allowed) after hook_stage1, or over every row when the list is longer
    than the coarse cap (dense): (lb5 f32, B int32 per entry / per row, survivors, surviving rows int64)"""
    from seesaw_amd import _lib
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    m = idx.n_rows if dense else rows.size
    lb5, B = np.empty(max(m, 1), np.float32), np.empty(max(m, 1), np.int32)
    surv = np.full(SURV_CAP, -1, dtype=np.int64)
    cnt = ctypes.c_int64(0)
    _lib.call("ssw_debug_prune41_refine", idx._h, _p(rows), rows.size, ctypes.c_float(float(threshold)), int(k), _p(lb5),
              _p(B), ctypes.byref(cnt), _p(surv))
    return lb5[:m], B[:m], int(cnt.value), surv[:min(int(cnt.value), SURV_CAP)]
