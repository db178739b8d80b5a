"""Shared by the coarse-mean tests: the float64 oracle of ssw_index_coarse_mean's arithmetic, the plain f32 transcription
of the reference's infer_coarse_embedding, ulp distances, and a generator of small multiscale indexes."""
import numpy as np
import pandas as pd


def coarse_oracle(X, row_start, keep, images):
    """the arithmetic of csrc/coarse.hip in numpy float64: per listed image the ascending-row sum of its kept rows
    (np.add.reduce over axis 0: one row added after the other), / c, / max(f64 norm, 1e-6), ONE rounding to f32.
    X: the rows the index holds (an f16 index: the widened rounded rows) -> f32 [m, dim]"""
    X = np.asarray(X)
    row_start = np.asarray(row_start, dtype=np.int64)
    keep = np.asarray(keep).reshape(-1) != 0
    out = np.empty((len(images), X.shape[1]), dtype=np.float32)
    for j, i in enumerate(np.asarray(images, dtype=np.int64).tolist()):
        rows = row_start[i] + np.flatnonzero(keep[row_start[i]:row_start[i + 1]])
        assert rows.size, f"image {i} has no kept row"
        s = np.add.reduce(X[rows].astype(np.float64), axis=0)
        mean = s / np.float64(rows.size)
        nrm = np.sqrt(np.sum(mean * mean))
        out[j] = (mean / max(nrm, 1e-6)).astype(np.float32)
    return out


def reference_f32(X, row_start, keep, images):
    """infer_coarse_embedding (seesaw/indices/coarse/preprocessor.py:11-19) in the f32 the reference runs it in: the
    sequential f32 sum of the kept rows / c, then res / np.maximum(np.linalg.norm(res), 1e-6) -> (f32 [m, dim], c [m])"""
    X = np.asarray(X, dtype=np.float32)
    row_start = np.asarray(row_start, dtype=np.int64)
    keep = np.asarray(keep).reshape(-1) != 0
    out = np.empty((len(images), X.shape[1]), dtype=np.float32)
    counts = np.empty(len(images), dtype=np.int64)
    for j, i in enumerate(np.asarray(images, dtype=np.int64).tolist()):
        rows = row_start[i] + np.flatnonzero(keep[row_start[i]:row_start[i + 1]])
        res = np.add.reduce(X[rows], axis=0, dtype=np.float32) / np.float32(rows.size)
        out[j] = res / np.maximum(np.linalg.norm(res), np.float32(1e-6))
        counts[j] = rows.size
    return out, counts


def _ordered(a, uint, sign):
    u = np.ascontiguousarray(a).view(uint).astype(np.int64)
    return np.where(u & sign, sign - u, u)  # -0.0 and +0.0 both map to 0


def ulp_distance_f32(a, b):
    """elementwise distance in units of f32 spacing (0 = the same value)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(_ordered(a, np.uint32, 1 << 31) - _ordered(b, np.uint32, 1 << 31))


def ulp_distance_f16(a, b):
    a, b = np.asarray(a, dtype=np.float16), np.asarray(b, dtype=np.float16)
    return np.abs(_ordered(a, np.uint16, 1 << 15) - _ordered(b, np.uint16, 1 << 15))


def unit_rows(rng, n, dim, direction=None, noise=0.3):
    """n unit-norm f32 rows: a shared unit direction plus a noise vector of norm `noise`, normalised.  With noise 0.3
    every row has cosine >= (1 - 0.3) / 1.3 > 1/2 with the direction, so the mean of any of them has norm >= 1/2"""
    if direction is None:
        direction = rng.standard_normal(dim)
    direction = direction / np.linalg.norm(direction)
    e = rng.standard_normal((n, dim))
    e *= noise / np.linalg.norm(e, axis=1, keepdims=True)
    x = direction[None, :] + e
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def tile_counts(rng, n_images, mean_tiles=13):
    """tile counts in [1, 70], mostly small, with both ends present"""
    t = np.minimum(70, rng.geometric(1.0 / mean_tiles, size=n_images)).astype(np.int64)
    if n_images >= 4:
        t[1], t[n_images // 2], t[-2] = 70, 1, 65
    return t


def make_index(seed, n_images, dim, absent=(), mean_tiles=13, dbidx_step=3):
    """a small multiscale index: X f32 [n, dim] unit rows, vector_meta (dbidx, zoom_level, max_zoom_level, x1 .. y2)
    sorted by dbidx, row_start, keep (= zoom_level == max_zoom_level) and the positions of the images with a kept row.
    An image keeps between 1 and all of its tiles, at random places; the images in `absent` have no row at their
    max_zoom_level (as after a min_zoom_level filter)"""
    rng = np.random.default_rng(seed)
    tiles = tile_counts(rng, n_images, mean_tiles)
    row_start = np.concatenate(([0], np.cumsum(tiles))).astype(np.int64)
    n = int(row_start[-1])
    zoom = np.empty(n, dtype=np.int16)
    for i in range(n_images):
        t = int(tiles[i])
        z = rng.integers(0, 2, size=t)
        if i not in absent:
            k = t if i % 7 == 0 else int(rng.integers(1, t + 1))
            z[rng.permutation(t)[:k]] = 2
        zoom[row_start[i]:row_start[i + 1]] = z
    dbidx = np.repeat(np.arange(n_images, dtype=np.int64) * dbidx_step + 5, tiles)
    meta = pd.DataFrame({"dbidx": dbidx, "zoom_level": zoom, "max_zoom_level": np.int16(2),
                         "x1": np.float32(0), "y1": np.float32(0), "x2": np.float32(224), "y2": np.float32(224)})
    keep = (zoom == 2).astype(np.uint8)
    images = np.array([i for i in range(n_images) if i not in absent], dtype=np.int64)
    return {"X": unit_rows(rng, n, dim), "meta": meta, "row_start": row_start, "keep": keep, "images": images,
            "row2image": np.repeat(np.arange(n_images, dtype=np.int32), tiles), "tiles": tiles}
