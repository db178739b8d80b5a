"""DeviceIndex: the [N, d] vector matrix resident in HBM + scan / top-k over the C-ABI.

The matrix is f32 by default; `dtype=np.float16` stores it as IEEE binary16 (half the bytes), and every result is then
the bits an f32 index of the widened rows `X.astype(np.float16).astype(np.float32)` returns.

This is the object the reference-shaped indices (`seesaw_amd.indices.*`,
`seesaw_amd.vector_index.VectorIndex`) delegate their numeric work to.  It replaces
`vectors @ q` + `np.argsort` + `_get_top_dbidxs` of the reference
(seesaw/indices/multiscale/multiscale_index.py:170-199, coarse_index.py:57-96).
numpy arrays in, numpy arrays out; everything in between runs in libseesaw_hip.so.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Optional

import numpy as np

from . import _lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


_DTYPE_CODES = {np.dtype(np.float32): _lib.SSW_DTYPE_F32, np.dtype(np.float16): _lib.SSW_DTYPE_F16}


def vector_dtype(dtype) -> np.dtype:
    """np.float32 / np.float16 (or "float32" / "float16", "f4" / "f2") -> the numpy dtype of the index's storage;
    anything else raises ValueError"""
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt not in _DTYPE_CODES:
        raise ValueError(f"vector dtype {dtype!r} unsupported (float32 or float16)")
    return dt


def round_vectors(vectors: np.ndarray, dtype) -> np.ndarray:
    """the f32 rows an index of storage `dtype` holds for `vectors`: the rows themselves for float32, the widened
    binary16 rounding (numpy's astype(float16): nearest even) for float16"""
    dt = vector_dtype(dtype)
    if dt == np.float16:
        return np.asarray(vectors).astype(np.float16).astype(np.float32)
    return np.ascontiguousarray(vectors, dtype=np.float32)


def view_rows(row_start: np.ndarray, positions: np.ndarray):
    """the rows of a view of the images `positions` (strictly ascending) of an index whose image p holds the rows
    [row_start[p], row_start[p + 1]): -> (parent_rows int64 [n_view], the view's own row_start int64 [m + 1]) -- what
    ssw_index_create_view builds on the host (row_start = np.arange(n + 1) for an index without an image map)"""
    row_start = np.asarray(row_start, dtype=np.int64)
    positions = np.asarray(positions, dtype=np.int64).reshape(-1)
    if positions.size == 0 or positions[0] < 0 or positions[-1] >= row_start.shape[0] - 1 or np.any(np.diff(positions) <= 0):
        raise ValueError("positions must be strictly ascending image positions of the index, at least one")
    counts = row_start[positions + 1] - row_start[positions]
    start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    # row j of image i of the view: row_start[positions[i]] + (j - start[i])
    parent_rows = np.repeat(row_start[positions] - start[:-1], counts) + np.arange(start[-1], dtype=np.int64)
    return parent_rows, start


def kept_images(row_start: np.ndarray, keep: np.ndarray) -> np.ndarray:
    """positions (int64, ascending) of the images with at least one kept row: image p holds the rows
    [row_start[p], row_start[p + 1]) and `keep[r] != 0` marks a kept row -- `coarse_mean`'s default `images`"""
    row_start = np.asarray(row_start, dtype=np.int64)
    keep = np.asarray(keep).reshape(-1)
    if keep.shape[0] != row_start[-1]:
        raise ValueError(f"keep has {keep.shape[0]} entries for {int(row_start[-1])} rows")
    kept_before = np.concatenate(([0], np.cumsum(keep != 0, dtype=np.int64)))
    return np.flatnonzero(kept_before[row_start[1:]] > kept_before[row_start[:-1]]).astype(np.int64)


class DeviceIndex:
    _row_start: Optional[np.ndarray] = None  # int64 [n_images + 1] host mirror of the image map, None without one

    def __init__(self, n_rows: int, dim: int = 512, device: int = 0, dev_ptr: int = 0, dtype=np.float32):
        self._h = ctypes.c_void_p()
        self.n_rows = int(n_rows)
        self.dim = int(dim)
        self.device = int(device)
        self.n_images = self.n_rows
        self.dtype = vector_dtype(dtype)
        _lib.call("ssw_index_create_typed", self.device, self.n_rows, self.dim, _DTYPE_CODES[self.dtype],
                  ctypes.c_void_p(dev_ptr) if dev_ptr else None, ctypes.byref(self._h))

    # -- construction -----------------------------------------------------------------
    @classmethod
    def from_numpy(cls, vectors: np.ndarray, row2image: Optional[np.ndarray] = None,
                   device: int = 0, chunk_rows: int = 1 << 18, dtype=np.float32) -> "DeviceIndex":
        """dtype=np.float16: the rows become numpy's `vectors.astype(np.float16)`.  binary16 input goes up as it is, f32
        input is rounded on the device, any other input (f64, ...) is rounded on the host chunk by chunk -- directly, as
        numpy rounds it, not through f32 (f64 -> f32 -> f16 could round a tie differently)"""
        vectors = np.asarray(vectors)
        assert vectors.ndim == 2, "vectors must be [N, d]"
        idx = cls(vectors.shape[0], vectors.shape[1], device=device, dtype=dtype)
        raw = idx.dtype == np.float16 and vectors.dtype != np.float32
        for r0 in range(0, vectors.shape[0], chunk_rows):
            if raw:
                chunk = np.ascontiguousarray(vectors[r0:r0 + chunk_rows], dtype=np.float16)
                _lib.call("ssw_index_upload_f16", idx._h, _ptr(chunk), r0, chunk.shape[0])
            else:
                chunk = np.ascontiguousarray(vectors[r0:r0 + chunk_rows], dtype=np.float32)
                _lib.call("ssw_index_upload", idx._h, _ptr(chunk), r0, chunk.shape[0])
        if row2image is not None:
            idx.set_row2image(row2image)
        return idx

    @classmethod
    def synthetic(cls, n_rows: int, dim: int = 512, seed: int = 0, first_row: int = 0,
                  device: int = 0, dtype=np.float32) -> "DeviceIndex":
        """rows oracle.synth_rows(seed, first_row, n_rows, dim) generated on the device (rounded to binary16 for
        dtype=np.float16)"""
        idx = cls(n_rows, dim, device=device, dtype=dtype)
        _lib.call("ssw_index_fill_random", idx._h, ctypes.c_uint64(seed), int(first_row))
        return idx

    def set_row2image(self, row2image: Optional[np.ndarray]):
        """row2image[r] = position (0..n_images-1) of row r's image; non-decreasing."""
        if row2image is None:
            _lib.call("ssw_index_set_row2image", self._h, None, 0)
            self.n_images = self.n_rows
            self._row_start = None
            return
        r2i = np.ascontiguousarray(row2image, dtype=np.int32)
        assert r2i.shape == (self.n_rows,)
        n_images = int(r2i[-1]) + 1 if self.n_rows else 0
        _lib.call("ssw_index_set_row2image", self._h, _ptr(r2i), n_images)
        self.n_images = n_images
        self._row_start = np.concatenate(([0], np.cumsum(np.bincount(r2i, minlength=n_images)))).astype(np.int64)

    # -- zero-copy subset views -------------------------------------------------------
    is_view = False  # a view scans its member rows in place, out of `parent`'s matrix
    parent: Optional["DeviceIndex"] = None
    parent_rows: Optional[np.ndarray] = None  # int64 [n_rows]: the parent row of every row of the view

    def view(self, image_positions) -> "DeviceIndex":
        """a DeviceIndex over the rows of the given images (positions of this index, strictly ascending; row positions
        for an index without an image map) that reads them out of THIS index's resident matrix
        (ssw_index_create_view): no rows are copied, the view holds a 4-byte row table, its own score buffer, selection
        workspace and image map, and returns what `from_numpy(X[rows], row2image=compact)` returns, bit for bit.  It
        sees this index's current rows and keeps it alive; `close()` of this index is refused while a view is open.
        What reads or writes the matrix by row number (upload, download, `scores_batch` / `topk_batch` and the other
        batched entries, knn, ...) raises on a view; a view batches through `view_scores_batch`, `view_topk_batch` and
        `view_topk_batch_avg`; `score_rows` / `gather_rows` take the view's rows.  Close views before their parent: `__del__` cannot
        raise, so a parent that is collected while a view is still open (interpreter shutdown, a reference cycle) keeps
        its device memory until the process ends -- the refusal is silent there."""
        pos = np.ascontiguousarray(image_positions, dtype=np.int64).reshape(-1)
        v = object.__new__(DeviceIndex)
        v._h = ctypes.c_void_p()
        _lib.call("ssw_index_create_view", self._h, _ptr(pos), pos.shape[0], ctypes.byref(v._h))
        n_rows, dim, n_images = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        _lib.call("ssw_index_shape", v._h, ctypes.byref(n_rows), ctypes.byref(dim), ctypes.byref(n_images))
        v.n_rows, v.dim, v.n_images = int(n_rows.value), int(dim.value), int(n_images.value)
        v.device, v.dtype = self.device, self.dtype
        v.is_view, v.parent = True, self
        v.parent_rows = np.empty(v.n_rows, dtype=np.int64)
        _lib.call("ssw_index_view_rows", v._h, _ptr(v.parent_rows))
        if self._row_start is not None:  # the view's own image map: its members' tile counts
            v._row_start = np.concatenate(([0], np.cumsum(self._row_start[pos + 1] - self._row_start[pos]))).astype(np.int64)
        return v

    # -- the coarse index's rows ------------------------------------------------------
    def coarse_mean(self, keep, images=None, dtype=np.float32) -> "DeviceIndex":
        """one row per image out of this index's resident rows (ssw_index_coarse_mean; infer_coarse_embedding of the
        reference, seesaw/indices/coarse/preprocessor.py:11-19): the mean of the image's KEPT rows (`keep[r] != 0`, one
        entry a row of this index) summed in float64 in row order, divided by max(its norm, 1e-6), rounded once to f32
        -> a new owning DeviceIndex of `len(images)` rows and storage `dtype`, without an image map, on this index's
        device.  `images`: positions in this index's image map, strictly ascending, each with a kept row; None: every
        image that has one.  Works on an f32 or float16 index and on a view (keep and images in the view's numbering);
        the rows never leave the device.  A row depends on its own image's kept rows alone."""
        if self._row_start is None and images is None:  # (with a list the library refuses: it owns that message)
            raise ValueError("coarse_mean needs an index with an image map (set_row2image)")
        keep =np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint8)
        if keep.shape[0] != self.n_rows:
            raise ValueError(f"keep has {keep.shape[0]} entries, the index has {self.n_rows} rows")
        pos = kept_images(self._row_start, keep) if images is None else \
            np.ascontiguousarray(np.asarray(images).reshape(-1), dtype=np.int64)
        if pos.shape[0] == 0:
            raise ValueError("coarse_mean: no image to derive a row for (no kept row, or an empty list)")
        out = DeviceIndex(pos.shape[0], self.dim, device=self.device, dtype=dtype)
        try:
            _lib.call("ssw_index_coarse_mean", self._h, _ptr(keep), _ptr(pos), pos.shape[0], out._h)
        except Exception:
            out.close()
            raise
        return out

    def close(self):
        if self._h:
            _lib.check(_lib.load().ssw_index_destroy(self._h))  # refused while views of this index are open
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data movement ----------------------------------------------------------------
    def download(self, first_row: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.n_rows - first_row if n is None else n
        out = np.empty((n, self.dim), dtype=np.float32)
        _lib.call("ssw_index_download", self._h, _ptr(out), int(first_row), int(n))
        return out

    def device_ptrs(self):
        """(matrix, scores) device pointers.  An f16 index's matrix is in its private lane-interleaved layout."""
        v, s = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("ssw_index_device_ptrs", self._h, ctypes.byref(v), ctypes.byref(s))
        return v.value, s.value

    HIP_STREAM_LEGACY = 1  # hipStreamLegacy: the handle that names the default (NULL) stream explicitly

    def set_stream(self, stream_ptr: int):
        """run this handle's work on the caller's stream.  torch's default stream has the handle 0, which the
        C-ABI reads as "back to the handle's own stream": it is passed as hipStreamLegacy instead, so the scan
        and the selection are ordered with the torch ops issued around them."""
        _lib.call("ssw_index_set_stream", self._h, ctypes.c_void_p(int(stream_ptr) or self.HIP_STREAM_LEGACY))

    def restore_own_stream(self):
        _lib.call("ssw_index_set_stream", self._h, None)

    def sync(self):
        _lib.call("ssw_index_sync", self._h)

    # -- scan / top-k -----------------------------------------------------------------
    def _query(self, q: np.ndarray) -> np.ndarray:
        q = np.ascontiguousarray(np.asarray(q).reshape(-1), dtype=np.float32)
        assert q.shape[0] == self.dim, f"query has {q.shape[0]} components, index dim is {self.dim}"
        return q

    def scores(self, q: np.ndarray) -> np.ndarray:
        """index.score(vec): all N cosine scores (multiscale_index.py:284-285)."""
        q = self._query(q)
        out = np.empty(self.n_rows, dtype=np.float32)
        _lib.call("ssw_index_scan", self._h, _ptr(q), _ptr(out))
        return out

    def scan(self, q: np.ndarray):
        """Run the scan and leave the scores resident on the device."""
        q = self._query(q)
        _lib.call("ssw_index_scan", self._h, _ptr(q), None)

    def topk(self, q: Optional[np.ndarray], k: int, excluded: Optional[Iterable[int]] = None):
        """Top-k distinct images (positions), their max score and the row attaining it.
        q=None reuses the scores of the previous scan.  With a query, a large index (f32 or float16 rows alike) scans a
        quantised shadow of the rows first and scores only the rows that can still reach the k-th image exactly: the
        int8 shadow from 2^22 rows, the packed 6-bit shadow from 2^23 f32 or 2^24 float16 rows; a dim-768 index the
        6-bit shadow alone, from 2^20 rows.  The results are the full scan's bits."""
        k = int(k)
        qa = None if q is None else self._query(q)
        ex = None
        n_ex = 0
        if excluded is not None:
            ex = np.ascontiguousarray(np.fromiter(excluded, dtype=np.int64))
            n_ex = ex.shape[0]
            if n_ex == 0:
                ex = None
        imgs = np.empty(k, dtype=np.int64)
        scs = np.empty(k, dtype=np.float32)
        rows = np.empty(k, dtype=np.int64)
        cnt = ctypes.c_int32(0)
        _lib.call("ssw_index_topk", self._h, _ptr(qa), _ptr(ex), n_ex, k, _ptr(imgs), _ptr(scs),
                  _ptr(rows), ctypes.byref(cnt))
        c = cnt.value
        return imgs[:c], scs[:c], rows[:c]

    def _queries(self, Q) -> np.ndarray:
        Q = np.asarray(Q)
        if Q.ndim == 1:
            Q = Q.reshape(1, -1)
        Q = np.ascontiguousarray(Q.reshape(Q.shape[0], -1), dtype=np.float32)
        if Q.shape[0] < 1 or Q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq >= 1, {self.dim}], got {Q.shape}")
        return Q

    @staticmethod
    def _excluded_batch(excluded, nq: int):
        """None, or nq iterables (each may be None) -> (ids int64 or None, offsets int64 [nq + 1] or None)"""
        if excluded is None:
            return None, None
        lists = list(excluded)
        if len(lists) != nq:
            raise ValueError(f"excluded has {len(lists)} lists for {nq} queries")
        arrs = [np.empty(0, dtype=np.int64) if e is None else np.fromiter(e, dtype=np.int64) for e in lists]
        offsets = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([a.shape[0] for a in arrs], out=offsets[1:])
        ids = np.ascontiguousarray(np.concatenate(arrs)) if offsets[-1] else None
        return ids, offsets

    def scores_batch(self, Q: np.ndarray) -> np.ndarray:
        """[nq, n_rows] f32: row b is the bits of `scores(Q[b])`, all from one pass over the rows per chunk of queries
        (ssw_index_scan_batch).  The resident scores are then those of the last query."""
        Q = self._queries(Q)
        out = np.empty((Q.shape[0], self.n_rows), dtype=np.float32)
        _lib.call("ssw_index_scan_batch", self._h, _ptr(Q), Q.shape[0], _ptr(out))
        return out

    def topk_batch(self, Q: np.ndarray, k: int, excluded=None, prune: bool = False):
        """`[topk(Q[b], k, excluded[b]) for b]` with the rows read once per chunk of queries (ssw_index_topk_batch):
        a list of (images, scores, rows), bit for bit what the single calls return.  `excluded` is None or a sequence of
        nq iterables of image positions, each of which may be None.  The handle is left as after the last query's topk.
        `prune=True` (ssw_index_topk_batch_pruned): on an index whose single `topk` is pruned, one pass over a shadow
        -- from 25 M rows the packed 6-bit one single queries scan there, below that (or where that one is refused for
        memory) the int8 one; at dim 768 the 6-bit one from 2^20 rows and no other -- bounds a chunk of up to 16 queries
        and only each query's survivors are scored exactly -- the same results; `prune_stats` counts every query.  Any
        other index takes the plain batch."""
        k = int(k)
        Q = self._queries(Q)
        nq = Q.shape[0]
        ids, offsets = self._excluded_batch(excluded, nq)
        imgs = np.empty((nq, k), dtype=np.int64)
        scs = np.empty((nq, k), dtype=np.float32)
        rows = np.empty((nq, k), dtype=np.int64)
        cnt = np.zeros(nq, dtype=np.int32)
        _lib.call("ssw_index_topk_batch_pruned" if prune else "ssw_index_topk_batch", self._h, _ptr(Q), nq, _ptr(ids),
                  _ptr(offsets), k, _ptr(imgs), _ptr(scs), _ptr(rows), _ptr(cnt))
        return [(imgs[b, :c].copy(), scs[b, :c].copy(), rows[b, :c].copy()) for b, c in enumerate(cnt.tolist())]

    # -- the same on a view: the member rows read once per chunk of queries, in place ----
    def view_scores_batch(self, Q: np.ndarray) -> np.ndarray:
        """`scores_batch` of a view (ssw_index_view_scan_batch): [nq, n_rows] f32, row b the bits of `scores(Q[b])` --
        those of `parent.scores(Q[b])[parent_rows]` -- from one pass over the member rows per chunk of queries.  The
        resident scores are then those of the last query.  Raises on an index that is not a view."""
        Q = self._queries(Q)
        out = np.empty((Q.shape[0], self.n_rows), dtype=np.float32)
        _lib.call("ssw_index_view_scan_batch", self._h, _ptr(Q), Q.shape[0], _ptr(out))
        return out

    def view_topk_batch(self, Q: np.ndarray, k: int, excluded=None):
        """`topk_batch` of a view (ssw_index_view_topk_batch): `[topk(Q[b], k, excluded[b]) for b]`, bit for bit, with
        the member rows read out of the parent's matrix once per chunk of queries; what `topk_batch` of the copied
        subset returns.  `excluded` as there.  There is no pruned form: a view holds no shadow.  The view is left as
        after the last query's topk.  Raises on an index that is not a view."""
        k = int(k)
        Q = self._queries(Q)
        nq = Q.shape[0]
        ids, offsets = self._excluded_batch(excluded, nq)
        imgs = np.empty((nq, k), dtype=np.int64)
        scs = np.empty((nq, k), dtype=np.float32)
        rows = np.empty((nq, k), dtype=np.int64)
        cnt = np.zeros(nq, dtype=np.int32)
        _lib.call("ssw_index_view_topk_batch", self._h, _ptr(Q), nq, _ptr(ids), _ptr(offsets), k, _ptr(imgs), _ptr(scs),
                  _ptr(rows), _ptr(cnt))
        return [(imgs[b, :c].copy(), scs[b, :c].copy(), rows[b, :c].copy()) for b, c in enumerate(cnt.tolist())]

    def load_scores(self, scores: np.ndarray):
        """overwrite the resident per-row scores (f32; -inf rows are never selected)."""
        s = np.ascontiguousarray(scores, dtype=np.float32)
        assert s.shape == (self.n_rows,)
        _lib.call("ssw_index_load_scores", self._h, _ptr(s))

    def gather_scores(self, rows: np.ndarray) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty(rows.shape[0], dtype=np.float32)
        _lib.call("ssw_index_gather_scores", self._h, _ptr(rows), rows.shape[0], _ptr(out))
        return out

    def gather_rows(self, rows: np.ndarray) -> np.ndarray:
        """`vectors[rows]` [n, dim] f32 out of the resident matrix (widened for an f16 index)"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((rows.shape[0], self.dim), dtype=np.float32)
        _lib.call("ssw_index_gather_rows", self._h, _ptr(rows), rows.shape[0], _ptr(out))
        return out

    def score_rows(self, q: np.ndarray, rows: np.ndarray) -> np.ndarray:
        """`vectors[rows] @ q` on the device, same summation order as the scan."""
        q = self._query(q)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty(rows.shape[0], dtype=np.float32)
        _lib.call("ssw_index_score_rows", self._h, _ptr(q), _ptr(rows), rows.shape[0], _ptr(out))
        return out

    # -- second stage: avg_score aggregation ------------------------------------------
    AUG_LARGER = {"all": 0, "greater": 1, "adjacent": 2}
    RESCORE_MAX_TILES = 2048  # tiles of one image the aggregation kernel keeps in LDS (csrc/ssw_common.h)

    def set_tile_meta(self, boxes: np.ndarray, zoom_level: np.ndarray):
        """tile boxes [n_rows, 4] = x1, y1, x2, y2 (f32) and zoom levels [n_rows] of every row"""
        b = np.ascontiguousarray(boxes, dtype=np.float32)
        z = np.ascontiguousarray(zoom_level, dtype=np.int32)
        assert b.shape == (self.n_rows, 4) and z.shape == (self.n_rows,)
        _lib.call("ssw_index_set_tile_meta", self._h, _ptr(b), _ptr(z))

    def rescore_avg(self, image_positions: np.ndarray, aug_larger: str, minus_scores: Optional[np.ndarray] = None,
                    aug_weight: str = "level_max"):
        """score_frame2's `avg_score` for the given candidate images over the resident tile scores:
        -> (aggregated score of the image's best tile f32 [m], that tile's row int64 [m])"""
        pos = np.ascontiguousarray(image_positions, dtype=np.int64)
        m = pos.shape[0]
        minus = None if minus_scores is None else np.ascontiguousarray(minus_scores, dtype=np.float32)
        scores = np.empty(m, dtype=np.float32)
        rows = np.empty(m, dtype=np.int64)
        aug = self.AUG_LARGER[aug_larger] | {"level_max": 0, "cont_weighted": 4}[aug_weight]
        _lib.call("ssw_index_rescore_avg", self._h, _ptr(pos), m, aug, _ptr(minus), _ptr(scores), _ptr(rows))
        return scores, rows

    def topk_batch_avg(self, Q: np.ndarray, k: int, aug_larger: str, excluded=None, aug_weight: str = "level_max",
                       prune: bool = False):
        """both stages for a batch (ssw_index_topk_batch_avg): `topk_batch(Q, k, excluded)` and, for every query, what
        `rescore_avg(images, aug_larger, aug_weight=aug_weight)` returns for the images it selected while that query's
        scores are resident -- read from the query's own score slab inside the batch.  A list of
        (images, scores, rows, avg_scores, avg_rows), `avg_*[i]` belonging to `images[i]` (selection order, not the
        ascending order `rescore_avg` is usually given).  The handle is left as after the last query's topk.
        `prune=True` (ssw_index_topk_batch_avg_pruned): the first stage is `topk_batch(prune=True)`'s, on the same
        shadow (6-bit or int8), and only the tiles of each query's selected images are then scored exactly into its
        slab for the second stage -- the same results;
        `prune_stats` counts every query and the rows rescored.  Any other index takes the plain batch."""
        k = int(k)
        Q = self._queries(Q)
        nq = Q.shape[0]
        ids, offsets = self._excluded_batch(excluded, nq)
        aug = self.AUG_LARGER[aug_larger] | {"level_max": 0, "cont_weighted": 4}[aug_weight]
        imgs = np.empty((nq, k), dtype=np.int64)
        scs = np.empty((nq, k), dtype=np.float32)
        rows = np.empty((nq, k), dtype=np.int64)
        avg_scs = np.empty((nq, k), dtype=np.float32)
        avg_rows = np.empty((nq, k), dtype=np.int64)
        cnt = np.zeros(nq, dtype=np.int32)
        _lib.call("ssw_index_topk_batch_avg_pruned" if prune else "ssw_index_topk_batch_avg", self._h, _ptr(Q), nq,
                  _ptr(ids), _ptr(offsets), k, aug, _ptr(imgs),
                  _ptr(scs), _ptr(rows), _ptr(avg_scs), _ptr(avg_rows), _ptr(cnt))
        return [(imgs[b, :c].copy(), scs[b, :c].copy(), rows[b, :c].copy(), avg_scs[b, :c].copy(), avg_rows[b, :c].copy())
                for b, c in enumerate(cnt.tolist())]

    def view_topk_batch_avg(self, Q: np.ndarray, k: int, aug_larger: str, excluded=None, aug_weight: str = "level_max"):
        """`topk_batch_avg` of a view (ssw_index_view_topk_batch_avg): both stages for a batch over the member rows,
        the second over the view's own image map and tile meta; a list of (images, scores, rows, avg_scores, avg_rows)
        as there, what `topk_batch_avg` of the copied subset returns.  No pruned form.  Raises on an index that is not a
        view."""
        k = int(k)
        Q = self._queries(Q)
        nq = Q.shape[0]
        ids, offsets = self._excluded_batch(excluded, nq)
        aug = self.AUG_LARGER[aug_larger] | {"level_max": 0, "cont_weighted": 4}[aug_weight]
        imgs = np.empty((nq, k), dtype=np.int64)
        scs = np.empty((nq, k), dtype=np.float32)
        rows = np.empty((nq, k), dtype=np.int64)
        avg_scs = np.empty((nq, k), dtype=np.float32)
        avg_rows = np.empty((nq, k), dtype=np.int64)
        cnt = np.zeros(nq, dtype=np.int32)
        _lib.call("ssw_index_view_topk_batch_avg", self._h, _ptr(Q), nq, _ptr(ids), _ptr(offsets), k, aug, _ptr(imgs),
                  _ptr(scs), _ptr(rows), _ptr(avg_scs), _ptr(avg_rows), _ptr(cnt))
        return [(imgs[b, :c].copy(), scs[b, :c].copy(), rows[b, :c].copy(), avg_scs[b, :c].copy(), avg_rows[b, :c].copy())
                for b, c in enumerate(cnt.tolist())]

    AGG_PLAIN, AGG_AVG = 0, 1  # ssw_index_stage2_pair_batch's `agg`

    def stage2_pair(self, Q: np.ndarray, Q2: np.ndarray, positions: np.ndarray, counts: np.ndarray, agg: str,
                    aug_larger: str = "all", aug_weight: str = "level_max", out=None):
        """the second stage of a batch of two-vector queries in one launch (ssw_index_stage2_pair_batch): for query b
        and each of its first `counts[b]` candidate images `positions[b, :]` (int64 [nq, k], any order), the image's
        tiles are scored from the index rows for Q[b] and Q2[b] and the differences aggregated -- agg "avg_score" (any
        agg_method other than "plain_score"): what `rescore_avg(pos, aug_larger, score_rows(Q2[b], rows), aug_weight)`
        returns while Q[b]'s scores are resident; "plain_score": the first tile with the highest non-NaN
        `gather_scores(rows) - score_rows(Q2[b], rows)`.  -> (scores f32 [nq, k], best rows int64 [nq, k]); entries from
        counts[b] on are `out`'s (a pair of such arrays to write into) or unspecified.  The handle's scores, results,
        exclusion set and prune counters are not touched."""
        Q, Q2 = self._queries(Q), self._queries(Q2)
        nq = Q.shape[0]
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if Q2.shape != Q.shape or pos.ndim != 2 or pos.shape[0] != nq or cnt.shape[0] != nq:
            raise ValueError(f"stage2_pair: Q {Q.shape}, Q2 {Q2.shape}, positions {pos.shape}, counts {cnt.shape} disagree")
        k = pos.shape[1]
        if out is None:
            scores, rows = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)
        else:
            scores, rows = out
            assert scores.dtype == np.float32 and rows.dtype == np.int64 and scores.shape == rows.shape == (nq, k) \
                and scores.flags.c_contiguous and rows.flags.c_contiguous
        if agg == "plain_score":
            code, aug = self.AGG_PLAIN, 0
        else:
            code, aug = self.AGG_AVG, self.AUG_LARGER[aug_larger] | {"level_max": 0, "cont_weighted": 4}[aug_weight]
        _lib.call("ssw_index_stage2_pair_batch", self._h, _ptr(Q), _ptr(Q2), nq, _ptr(pos), _ptr(cnt), k, code, aug,
                  _ptr(scores), _ptr(rows))
        return scores, rows

    def rescore_avg_f64(self, dev_scores_ptr: int, image_positions: np.ndarray, aug_larger: str,
                        aug_weight: str = "level_max"):
        """rescore_avg over float64 tile scores resident on the device (one per index row, e.g. the label-propagation
        output): -> (aggregated score f64 [m], best tile's row int64 [m])"""
        pos = np.ascontiguousarray(image_positions, dtype=np.int64)
        m = pos.shape[0]
        scores = np.empty(m, dtype=np.float64)
        rows = np.empty(m, dtype=np.int64)
        aug = self.AUG_LARGER[aug_larger] | {"level_max": 0, "cont_weighted": 4}[aug_weight]
        _lib.call("ssw_index_rescore_avg_f64", self._h, ctypes.c_void_p(int(dev_scores_ptr)), _ptr(pos), m, aug,
                  _ptr(scores), _ptr(rows))
        return scores, rows

    # -- device-resident forms (bench / sharded index) --------------------------------
    def set_excluded(self, excluded: Optional[Iterable[int]]):
        ex = None
        n_ex = 0
        if excluded is not None:
            ex = np.ascontiguousarray(np.fromiter(excluded, dtype=np.int64))
            n_ex = ex.shape[0]
            if n_ex == 0:
                ex = None
        _lib.call("ssw_index_set_excluded", self._h, _ptr(ex), n_ex)

    def topk_dev(self, q_dev_ptr: int, k: int):
        _lib.call("ssw_index_topk_dev", self._h, ctypes.c_void_p(q_dev_ptr) if q_dev_ptr else None, int(k))

    def select_deep_dev(self, k: int):
        """exact selection for the mass-tie case (result_ptrs' overflow word set): same result buffers"""
        _lib.call("ssw_index_select_deep_dev", self._h, int(k))

    def set_exchange_target_batch(self, dev_msgs_ptr: int, n_slots: int, k_max: int, with_best: bool, image_offset: int = 0,
                                  row_offset: int = 0):
        """attach (0 / None: detach) the message block [n_slots, msg_len] u64 that `topk_batch_dev` fills, one slot a
        query (ssw_index_set_exchange_target_batch); the single exchange target is a state of its own beside it"""
        _lib.call("ssw_index_set_exchange_target_batch", self._h, ctypes.c_void_p(dev_msgs_ptr) if dev_msgs_ptr else None,
                  int(n_slots), int(k_max), int(bool(with_best)), int(image_offset), int(row_offset))

    def topk_batch_dev(self, Q: np.ndarray, k: int, excluded=None, first_slot: int = 0, prune: bool = False):
        """`topk_batch` that stays on the device (ssw_index_topk_batch_dev; enqueue only): the rows are read once per
        chunk of queries and query b's selection writes its exchange message into slot `first_slot + b` of the attached
        block.  An overflowed selection is not repaired: its flag travels in the slot (`topk_slot_deep_dev`).  The
        handle is left as after `topk_dev` of the last query with its exclusion list.
        `prune=True` (ssw_index_topk_batch_dev_pruned): on an index the pruned batch serves, one pass over the shadow
        `topk_batch(prune=True)` would scan (6-bit or int8) bounds a chunk of up to 16 queries and one launch scores
        every query's survivors exactly, still without a host wait.  A query whose certificate failed on this shard is flagged with the value 2 in its slot and repaired the
        same way; `prune_batch_dev_counts` reads what the device decided.  Any other index takes the plain call."""
        Q = self._queries(Q)
        nq = Q.shape[0]
        ids, offsets = self._excluded_batch(excluded, nq)
        _lib.call("ssw_index_topk_batch_dev_pruned" if prune else "ssw_index_topk_batch_dev", self._h, _ptr(Q), nq,
                  _ptr(ids), _ptr(offsets), int(k), int(first_slot))

    def stage2_avg_batch_dev(self, Q: np.ndarray, keys_ptr: int, counts_ptr: int, k_max: int, k: int, aug_larger: str,
                             out_ptr: int, image_offset: int = 0, row_offset: int = 0, aug_weight: str = "level_max"):
        """the second stage of a sharded chunk on this shard (ssw_index_stage2_avg_batch_dev; enqueue only): for the
        merged keys [nq, k_max] / counts [nq] at the device pointers `keys_ptr` / `counts_ptr` (what
        `ssw_topk_merge_msgs_batch_dev` wrote; global image positions), every candidate among the first `k` of query b
        that is one of this shard's images -- positions [image_offset, image_offset + n_images) -- is scored for Q[b]
        straight from the index rows and aggregated as `rescore_avg` aggregates it.  The block [nq, 2, k_max] u64 at
        `out_ptr` receives `1 << 32 | f32 bits of the score` and `row_offset + best row`, zeros where the image is
        another shard's.  The handle's scores, results and prune counters are not touched."""
        Q = self._queries(Q)
        aug = self.AUG_LARGER[aug_larger] | {"level_max": 0, "cont_weighted": 4}[aug_weight]
        _lib.call("ssw_index_stage2_avg_batch_dev", self._h, _ptr(Q), Q.shape[0], ctypes.c_void_p(int(keys_ptr)),
                  ctypes.c_void_p(int(counts_ptr)), int(k_max), int(k), aug, int(image_offset), int(row_offset),
                  ctypes.c_void_p(int(out_ptr)))

    def prune_batch_dev_counts(self):
        """what the device decided for the last chunk of the last `topk_batch_dev(prune=True)`
        (ssw_index_prune_batch_dev_read; synchronises): (survivors int64 [w], fail_bits int32 [w]) -- the raw survivor
        count of each slot and why it was not certified (1 threshold selection failed, 2 unboundable query, 4 more
        survivors than the cap; 0 = certified).  w = 0 when that call took the plain scan."""
        out = np.zeros(32, dtype=np.int32)
        w = ctypes.c_int32(0)
        _lib.call("ssw_index_prune_batch_dev_read", self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                  ctypes.byref(w))
        pairs = out[:2 * w.value].reshape(-1, 2)
        return pairs[:, 0].astype(np.int64), pairs[:, 1].copy()

    def topk_slot_deep_dev(self, q: np.ndarray, k: int, excluded: Optional[Iterable[int]], slot: int):
        """the repair of one flagged query of a batch (ssw_index_topk_slot_deep_dev): full scan of q, exact deep
        selection, message into `slot`; synchronises inside"""
        qa = self._query(q)
        ex = None if excluded is None else np.ascontiguousarray(np.fromiter(excluded, dtype=np.int64))
        n_ex = 0 if ex is None else ex.shape[0]
        _lib.call("ssw_index_topk_slot_deep_dev", self._h, _ptr(qa), _ptr(ex) if n_ex else None, n_ex, int(k), int(slot))

    def scan_dev(self, q_dev_ptr: int):
        _lib.call("ssw_index_scan_dev", self._h, ctypes.c_void_p(q_dev_ptr))

    def result_ptrs(self):
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("ssw_index_result_ptrs", self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    def topk_fetch(self, k: int):
        k = int(k)
        imgs = np.empty(k, dtype=np.int64)
        scs = np.empty(k, dtype=np.float32)
        rows = np.empty(k, dtype=np.int64)
        cnt = ctypes.c_int32(0)
        _lib.call("ssw_index_topk_fetch", self._h, k, _ptr(imgs), _ptr(scs), _ptr(rows), ctypes.byref(cnt))
        c = cnt.value
        return imgs[:c], scs[:c], rows[:c]

    # -- k-NN graph -------------------------------------------------------------------
    def knn(self, k: int, seed: int = 0):
        """Exact k nearest rows of every row (compute_exact_knn, knn_graph.py:170-191):
        returns (dst int32 [n, k+1], score f32 [n, k+1], n_recomputed).  Each row lists the k+1
        best rows including itself by (score desc, row id asc); scores are scan-order f32.
        Rows the fp16 candidate pass could not certify are redone with the ordinary exact scan."""
        k = int(k)
        n = self.n_rows
        dst = np.empty((n, k + 1), dtype=np.int32)
        score = np.empty((n, k + 1), dtype=np.float32)
        cert = np.empty(n, dtype=np.uint8)
        _lib.call("ssw_knn_build", self._h, k, ctypes.c_uint64(int(seed)), _ptr(dst), _ptr(score), _ptr(cert))
        redo = np.nonzero(cert == 0)[0]
        if redo.shape[0]:
            view = DeviceIndex(n, self.dim, device=self.device, dev_ptr=self.device_ptrs()[0])  # rows, no image map
            try:
                for r in redo.tolist():
                    ids, sc, _ = view.topk(self.download(r, 1)[0], k + 1)
                    dst[r, :ids.shape[0]] = ids
                    score[r, :ids.shape[0]] = sc
            finally:
                view.close()
        return dst, score, int(redo.shape[0])

    # -- pruned top-k ----------------------------------------------------------------
    _SHADOW_STATES = ("none", "current", "stale", "refused")

    def prune_stats(self, completions: bool = False) -> dict:
        """state of the certified pre-scan of `topk` with a query (ssw_index_prune_stats).  `shadow` describes the
        shadow single queries scan -- the packed 6-bit one on an index of at least 2^23 f32 or 2^24 float16 rows, else
        the int8 one: "none", "current", "stale" (the rows changed since it was built; the next pruned call rebuilds
        it) or "refused" (too little free device memory beside it); `eligible`: the next top-k with a query is pruned;
        `last_survivors`: rows the last pruned call rescored (-1 = it fell back to the full scan); `queries` /
        `fallbacks`: pruned calls and how many of them fell back; `shadow_bytes`: device memory the shadows hold
        (dim + 8 bytes a row for the int8 one, 3 dim / 4 + 8 for the 6-bit one; from 25 M rows a pruned batch scans
        the 6-bit one single queries scan and builds no other, below that it builds and scans the int8 one).
        A dim-768 index (CLIP ViT-L/14) has the 6-bit shadow alone, 584 bytes a row: `shadow` and `shadow_bytes`
        ((n + 15) // 16 * 16 * 584) are that shadow's, and single queries and pruned batches scan it from 2^20 rows
        on, f32 or float16; below that every call is the full-precision one.
        An f32 index of dim 512 or 1024 without an image map and of at least 25 M rows: `shadow` is the packed 5-bit
        shadow single queries scan there, 5 dim / 8 + 8 bytes a row of (n + 15) // 16 * 16 rows in `shadow_bytes`.
        From 100 M rows such an index holds the two-stage form of those codes instead (a 4-bit plane scanned for every
        row, a 1-bit plane read for that scan's survivors), 5 dim / 8 + 16 bytes a row, and no packed 5-bit shadow.
        `completions=True` adds the two words of ssw_index_prune_completions (the six above stay what they were for
        callers that compare the whole dict): `completions`: full scans that completed a partial score buffer or slab
        for a reader; `rescored_rows`: rows the second-stage readers (`rescore_avg`, `gather_scores`, `topk_batch_avg`)
        scored exactly on demand instead"""
        out = np.zeros(6, dtype=np.int64)
        _lib.call("ssw_index_prune_stats", self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        st = {"shadow": self._SHADOW_STATES[int(out[0])], "eligible": bool(out[1]), "last_survivors": int(out[2]),
              "queries": int(out[3]), "fallbacks": int(out[4]), "shadow_bytes": int(out[5])}
        if completions:
            more = np.zeros(2, dtype=np.int64)
            _lib.call("ssw_index_prune_completions", self._h, more.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
            st.update(completions=int(more[0]), rescored_rows=int(more[1]))
        return st

    # -- profiling --------------------------------------------------------------------
    def profile(self, enable: bool):
        _lib.call("ssw_index_profile", self._h, int(bool(enable)))

    def profile_read(self) -> np.ndarray:
        out = np.empty(4096, dtype=np.float32)
        n = ctypes.c_int32(0)
        _lib.call("ssw_index_profile_read", self._h, _ptr(out), 4096, ctypes.byref(n))
        return out[:n.value].copy()


def decode_keys(keys: np.ndarray):
    """(score_key << 32 | ~image) composite keys -> (images int64, scores f32)."""
    keys = np.asarray(keys, dtype=np.uint64)
    imgs = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    o = (keys >> np.uint64(32)).astype(np.uint32)
    neg = (o & np.uint32(0x80000000)) == 0
    u = np.where(neg, ~o, o & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    return imgs, u.view(np.float32)
