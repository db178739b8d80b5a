"""Test infrastructure of the packed 5-bit shadow (tests/test_prune5_cpu.py, tests/test_prune5_gpu.py): the numpy twin
of the placement function (csrc/ssw_common.h, q5_fields over q6_slot / q6_word_offset), of the builder (csrc/prune.hip,
k_q5_build), of the scan's unpack and bound (k_q5_bounds, k_survivors_mq with the 5-bit code norm) and of the exact
threshold (k_exact_threshold), and the lab hooks' wrappers.  The query's twin is the pruned batch's
(_prune_batch_helpers.quantise_query).  Never imported by the product."""
import ctypes

import numpy as np

from _prune6_helpers import slot, word_offset
from _prune_batch_helpers import INFLATE, quantise_query, upper_bound  # noqa: F401  (re-exported)
from _prune_helpers import PAD_ABS, SAFETY, gamma

LEVELS = 15
SURV_CAP = 1 << 18
MAX_TOPK = 4096


def code_norm(dim):
    """the kernel's constant >= 15 sqrt(dim)"""
    return {512: 339.4112550, 1024: 480.0}[dim]


def candidates(k):
    """keys of the threshold selection on the 5-bit path"""
    return min(MAX_TOPK, max(1024, 4 * k))


# ---- placement: element i of row r -> the bits of its code in the row's tile ----------------------------------------
def fields(u, j):
    """q5_fields: the (word, byte, lo, bits, from) of the code in slot j of k-step u of a lane"""
    w, b = 5 * (u >> 1), j & 3
    if u & 1 == 0:
        if j < 12:
            return [(w + (j >> 2), b, 3, 5, 0)]
        return [(w, b, 0, 3, 2), (w + 1, b, 0, 2, 0)]
    if j < 8:
        return [(w + 3 + (j >> 2), b, 3, 5, 0)]
    if j < 12:
        return [(w + 2, b, 0, 3, 2), (w + 3, b, 0, 2, 0)]
    return [(w + 4, b, 0, 3, 2), (w + 1, b, 2, 1, 1), (w + 3, b, 2, 1, 0)]


def tile_bytes(dim):
    return 16 * dim * 5 // 8


def _field_table(dim):
    """per element i: list of (byte offset in the tile for lane group g's row 0, lo, bits, from); the row adds 16 r"""
    u, g, j = slot(np.arange(dim))
    out = []
    for i in range(dim):
        out.append([(word_offset(16 * int(g[i]), word) + byte, lo, bits, frm)
                    for word, byte, lo, bits, frm in fields(int(u[i]), int(j[i]))])
    return out


def pack(codes):
    """codes int [n, dim], |c| <= 15 -> uint8 [ceil(n / 16), tile_bytes]: the device's buffer (pad rows zero)"""
    codes = np.asarray(codes, dtype=np.int64)
    n, dim = codes.shape
    out = np.zeros(((n + 15) // 16, tile_bytes(dim)), dtype=np.uint8)
    r = np.arange(n)
    tile, row = r >> 4, 16 * (r & 15)
    c5 = codes & 0x1f
    for i, fl in enumerate(_field_table(dim)):
        for off, lo, bits, frm in fl:
            # (a field of one element lands on another byte for every row: a plain |= sees no index twice)
            out[tile, off + row] |= (((c5[:, i] >> frm) & ((1 << bits) - 1)) << lo).astype(np.uint8)
    return out


def unpack(packed, n, dim):
    """the inverse: int8 [n, dim]"""
    r = np.arange(n)
    tile, row = r >> 4, 16 * (r & 15)
    out = np.zeros((n, dim), dtype=np.int64)
    for i, fl in enumerate(_field_table(dim)):
        for off, lo, bits, frm in fl:
            out[:, i] |= ((packed[tile, off + row].astype(np.int64) >> lo) & ((1 << bits) - 1)) << frm
    return ((out ^ 16) - 16).astype(np.int8)


def operand_words(packed_tile, lane, p):
    """what k_q5_bounds feeds the matrix core for the pair of k-steps 2 p, 2 p + 1 of a lane: 2 x 16 int8 values 8 c"""
    w = [int.from_bytes(bytes(packed_tile[word_offset(lane, 5 * p + t):word_offset(lane, 5 * p + t) + 4]), "little")
         for t in range(5)]
    m = [x & 0xf8f8f8f8 for x in w]
    x0 = (((w[0] & 0x07070707) << 5) | ((w[1] & 0x03030303) << 3)) & 0xffffffff
    x1 = (((w[2] & 0x07070707) << 5) | ((w[3] & 0x03030303) << 3)) & 0xffffffff
    x2 = (((w[4] & 0x07070707) << 5) | ((w[1] & 0x04040404) << 2) | ((w[3] & 0x04040404) << 1)) & 0xffffffff
    ops = [[m[0], m[1], m[2], x0], [m[3], m[4], x1, x2]]
    return [np.frombuffer(b"".join(int(x).to_bytes(4, "little") for x in o), dtype=np.int8).astype(np.int64) for o in ops]


# ---- the builder and the bound ---------------------------------------------------------------------------------------
def shadow5(X):
    """numpy twin of k_q5_build: (codes int8 [n, dim], s5 f32 [n], a5 f32 [n] rounded up); a5's double sums are taken
    in numpy's order, so the device's a5 is compared within a band (as the int8 and 6-bit tests do)"""
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


def width5(s, a, qq, dim):
    """w of DESIGN.md section 4, "5-bit shadow", as the kernels form it, in float64"""
    wQ = np.float64(qq["Q"]) * INFLATE
    wE = np.float64(qq["e"]) * code_norm(dim) * INFLATE
    with np.errstate(invalid="ignore"):
        return np.asarray(a, dtype=np.float64) * wQ + np.asarray(s, dtype=np.float64) * wE


def integer_sums(c, qq):
    """I_r = sum_i 8 c_ri (256 d_hi,i + d_lo,i), int64"""
    d = 256 * qq["d_hi"].astype(np.int64) + qq["d_lo"].astype(np.int64)
    return (8 * c.astype(np.int64)) @ d


def lower_bound5(c, s, a, qq):
    """twin of k_q5_bounds: (lb f32 [n] rounded down, w f64 [n], I int64 [n])"""
    dim = c.shape[1]
    I = integer_sums(c, qq)
    w = width5(s, a, qq, dim)
    with np.errstate(invalid="ignore"):
        lb = np.asarray(s, dtype=np.float64) * (np.float64(qq["t2"]) * 0.125) * I.astype(np.float64) - w
        lb = lb - (np.abs(lb) * 2.0 ** -50 + PAD_ABS)
        l32 = lb.astype(np.float32)
        l32 = np.where(l32.astype(np.float64) > lb, np.nextafter(l32, np.float32(-np.inf)), l32)
    return l32.astype(np.float32), w, I


def ord_key(v):
    """f32_to_ord: ascending unsigned order == ascending float order"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000)


def exact_threshold(lb, exact, k, excluded=None):
    """twin of the 5-bit path's threshold: (T f32, T_lb f32, T_x f32) from the lower bounds and the exact scores of all
    rows.  The candidates are the kc rows of the largest lower bounds (ties: the smaller row first, as the composite key
    orders them), T_x the k-th largest exact score among them that is not NaN (-inf with fewer than k), T the larger of
    the two in the key domain.  None when fewer than k rows are left."""
    lb = np.asarray(lb, dtype=np.float32)
    n = lb.shape[0]
    alive = np.ones(n, bool)
    if excluded is not None:
        alive[np.asarray(excluded, dtype=np.int64)] = False
    rows = np.nonzero(alive)[0]
    if rows.size < k:
        return None
    top = rows[np.lexsort((rows, -ord_key(lb[rows])))[:candidates(k)]]
    t_lb = lb[top[k - 1]]
    ex = np.asarray(exact, dtype=np.float32)[top]
    ex = ex[~np.isnan(ex)]
    t_x = np.float32(-np.inf) if ex.size < k else np.sort(ex)[::-1][k - 1]
    t = t_x if ord_key(t_x) > ord_key(t_lb) else t_lb
    return np.float32(t), np.float32(t_lb), np.float32(t_x)


def survivors(lb, w, T):
    """the rows k_survivors_mq lists: !(ub < T), NaN bounds and unboundable rows included"""
    with np.errstate(invalid="ignore"):
        return np.nonzero(~(upper_bound(lb, w) < np.float64(T)))[0]


# ---- lab hooks (include/seesaw_hip_debug.h) --------------------------------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def mode5(on, min_rows=-1):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune5", 1 if on else 0, int(min_rows))


def tune_scan5(blocks_per_cu, tiles):
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune5_scan", int(blocks_per_cu), int(tiles))


def launch_shape5(idx):
    """(four-wave blocks, 16-row tiles of one request) of the next k_q5_bounds launch over idx"""
    from seesaw_amd import _lib
    b, t = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.call("ssw_debug_prune5_scan_shape", idx._h, ctypes.byref(b), ctypes.byref(t))
    return int(b.value), int(t.value)


def hook_shadow5(idx, first_row=0, n_rows=None, codes=True):
    """(codes int8 [rows, dim] unpacked by the device library, or None; s5 f32 [rows]; a5 f32 [rows])"""
    from seesaw_amd import _lib
    m = idx.n_rows - first_row if n_rows is None else int(n_rows)
    c = np.empty((m, idx.dim), dtype=np.int8) if codes else None
    s, a = np.empty(m, dtype=np.float32), np.empty(m, dtype=np.float32)
    _lib.call("ssw_debug_prune5_shadow", idx._h, int(first_row), m, _p(c), _p(s), _p(a))
    return c, s, a


def hook_bounds5(idx, q, sums=True):
    """k_q6_query + k_q5_bounds: dict(I int64 [n] or None, lb f32 [n], Q, e, t2 f32, bad, codes int8 [2, dim])"""
    from seesaw_amd import _lib
    q = np.ascontiguousarray(q, dtype=np.float32)
    assert q.shape == (idx.dim,)
    n = idx.n_rows
    I = np.empty(n, np.int64) if sums else None
    lb, qe, codes = np.empty(n, np.float32), np.empty(4, np.float32), np.empty((2, idx.dim), np.int8)
    _lib.call("ssw_debug_prune5_bounds", idx._h, _p(q), _p(I), _p(lb), _p(qe), _p(codes))
    return dict(I=I, lb=lb, Q=qe[0], e=qe[1], t2=qe[2], bad=bool(qe[3] != 0), codes=codes)


def hook_survivors5(idx, threshold, k, sel_count=None, sel_overflow=0, cap=SURV_CAP):
    """k_survivors_mq (5-bit code norm) + k_prune_publish_mq over the bounds of the last hook_bounds5 against a threshold
    written by hand: (published, collected, rows int64)"""
    from seesaw_amd import _lib
    rows = np.full(max(int(cap), 1), -1, dtype=np.int64)
    pub, got = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.call("ssw_debug_prune5_survivors", idx._h, ctypes.c_float(float(threshold)), int(k),
              int(k if sel_count is None else sel_count), int(sel_overflow), int(cap), ctypes.byref(pub),
              ctypes.byref(got), ctypes.c_void_p(rows.ctypes.data))
    return int(pub.value), int(got.value), rows[:max(int(pub.value), 0)]
