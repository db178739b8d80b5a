"""Shared by the device-side tile pyramid's tests: a numpy restatement of Pillow's 8-bit bilinear resample (what
csrc/tiler.hip computes), pass by pass so that a failure can say which pass differs, and the argument packing of the
ssw_clip_embed_multiscale_u8 family."""
import ctypes
import math

import numpy as np

PRECISION_BITS = 22


def coefficients(in_size, out_size):
    """-> (k [out, ksize] int64 fixed-point weights, bounds [out, 2] = (first, n))"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int64)
    bounds = np.zeros((out_size, 2), np.int64)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        j = np.arange(n)
        a = np.abs((j + xmin - center + 0.5) * ss)
        w = np.where(a < 1.0, 1.0 - a, 0.0)
        ww = 0.0
        for v in w:  # Pillow's running sum, in its order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        kk[xx, :n] = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
        bounds[xx] = (xmin, n)
    return kk, bounds


def resample_axis1(a, out_size):
    """one pass along axis 1 of [H, W, 3] uint8 -> [H, out, 3] uint8"""
    kk, bounds = coefficients(a.shape[1], out_size)
    out = np.zeros((a.shape[0], out_size, a.shape[2]), np.uint8)
    ai = a.astype(np.int64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        s = (1 << (PRECISION_BITS - 1)) + np.tensordot(ai[:, xmin:xmin + n, :], kk[xx, :n], axes=([1], [0]))
        out[:, xx, :] = np.clip(s >> PRECISION_BITS, 0, 255)
    return out


def horizontal_pass(a, out_w):
    return resample_axis1(a, out_w)


def vertical_pass(a, out_h):
    return resample_axis1(a.transpose(1, 0, 2), out_h).transpose(1, 0, 2)


def resize(a, out_w, out_h):
    """PIL.Image.fromarray(a).resize((out_w, out_h), BILINEAR) as an array"""
    h, w, _ = a.shape
    if (out_w, out_h) == (w, h):
        return a.copy()
    if out_w != w:
        a = horizontal_pass(a, out_w)
    if out_h != h:
        a = vertical_pass(a, out_h)
    return np.ascontiguousarray(a)


def which_pass_differs(a, got, out_w, out_h):
    """words for an assertion message: compares `got` with the twin's passes"""
    h, w, _ = a.shape
    hz = horizontal_pass(a, out_w) if out_w != w else a
    if out_h == h:
        return f"horizontal pass: {int((hz != got).sum())} bytes differ from the twin"
    full = vertical_pass(hz, out_h)
    if out_w == w:
        return f"vertical pass: {int((full != got).sum())} bytes differ from the twin"
    # would the vertical pass of the twin's intermediate explain the rows?  If so the horizontal pass was right.
    rows_bad = np.nonzero((full != got).any(axis=(1, 2)))[0]
    cols_bad = np.nonzero((full != got).any(axis=(0, 2)))[0]
    return (f"{int((full != got).sum())} bytes differ from the twin's two passes; rows {rows_bad[:5].tolist()}.. "
            f"columns {cols_bad[:5].tolist()}.. (whole columns wrong: horizontal coefficients; whole rows: vertical)")


def pack_call(images, level_sizes, align=8):
    """images: list of [h, w, 3] uint8; level_sizes: per image a list of (w', h') -> (buffer, offsets int64 [n + 1],
    hw int32 [n, 2], level_first int32 [n + 1], level_wh int32 [L, 2]) as the C entries take them"""
    offsets = [0]
    for im in images:
        offsets.append(-(-(offsets[-1] + im.size) // align) * align)
    buf = np.zeros(max(offsets[-1], 1), np.uint8)
    for im, o in zip(images, offsets):
        buf[o:o + im.size] = np.ascontiguousarray(im).reshape(-1)
    hw = np.array([[im.shape[0], im.shape[1]] for im in images], np.int32).reshape(-1, 2)
    first = np.cumsum([0] + [len(ls) for ls in level_sizes]).astype(np.int32)
    wh = np.array([s for ls in level_sizes for s in ls], np.int32).reshape(-1, 2)
    return buf, np.array(offsets, np.int64), hw, first, wh


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def device_tiles(lib, model, images, level_sizes, cap=None):
    """ssw_debug_clip_multiscale_tiles on the lab build -> [n, tile, tile, 3] uint8"""
    buf, offsets, hw, first, wh = pack_call(images, level_sizes)
    t = model.image_size
    cap = sum(tile_count(s, t) for ls in level_sizes for s in ls) if cap is None else cap
    out = np.zeros((max(cap, 1), t, t, 3), np.uint8)
    n = ctypes.c_int64(-1)
    lib.call("ssw_debug_clip_multiscale_tiles", model._h, _p(buf), len(images), _p(offsets), _p(hw), _p(first), _p(wh),
             _p(out), cap, ctypes.byref(n))
    return out[:n.value]


def device_resize(lib, model, a, out_w, out_h):
    a = np.ascontiguousarray(a)
    out = np.zeros((out_h, out_w, 3), np.uint8)
    lib.call("ssw_debug_resize_u8", model._h, _p(a), a.shape[1], a.shape[0], out_w, out_h, _p(out))
    return out


def tile_count(size, tile):
    (w, h) = size
    half = tile // 2
    return sum(max(h - sy, 0) // tile * (max(w - sx, 0) // tile) for sx in (0, half) for sy in (0, half))
