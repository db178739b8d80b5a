"""CoarseIndex: one vector per image, exact cosine top-k on the GPU.

Interface of seesaw/indices/coarse/coarse_index.py:16-134 (CoarseIndex, CoarseQuery).  The
reference masks the included rows, copies them (`vectors[metas]`), runs `vecs @ q` and a
full `np.argsort` per query (:67-78); here the matrix stays resident in HBM, the excluded
images are skipped through a device bitmap, and the scan + exact top-k run in
libseesaw_hip.so (ssw_index_topk).
"""
from __future__ import annotations

import json
import os

import numpy as np
import pandas as pd

from ...bitmap import BitMap, FrozenBitMap
from ...device_index import DeviceIndex, round_vectors, vector_dtype as _vector_dtype
from ...query_interface import AccessMethod, InteractiveQuery
from ..interface import ActivationFrames, resolve_path


def _positions_of(sorted_dbidx: np.ndarray, ids) -> np.ndarray:
    ids = np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids, dtype=np.int64).reshape(-1)
    if ids.size == 0:
        return ids
    pos = np.searchsorted(sorted_dbidx, ids)
    pos = np.clip(pos, 0, sorted_dbidx.shape[0] - 1)
    return pos[sorted_dbidx[pos] == ids]


class CoarseIndex(AccessMethod):
    def __init__(self, embedding, vectors: np.ndarray, vector_meta: pd.DataFrame, path: str = None,
                 device: int = 0, vector_dtype: str = "float32", _view_of=None, _device_index=None):
        """vector_dtype="float16": the resident matrix is binary16 and `self.vectors` holds the widened rounded rows
        (what every host-side expression then reads is what the device scans).  `_view_of` (subset_view): (the parent's
        DeviceIndex, the member images' positions in it) -- the device index is then a view of the parent's resident
        rows, not an upload of `vectors`.  `_device_index` (MultiscaleIndex.coarse_index): an owning DeviceIndex that
        already holds these rows in `vector_dtype` on `device` -- it becomes this index's, nothing is uploaded, and
        `vectors` is its download"""
        self.path = path
        self.embedding = embedding
        self.vector_dtype = _vector_dtype(vector_dtype)
        self.vectors = round_vectors(vectors, self.vector_dtype)
        self.vector_meta = vector_meta
        dbidx = np.asarray(vector_meta.dbidx.values, dtype=np.int64)
        assert np.all(np.diff(dbidx) > 0), "one vector per image, sorted by dbidx (coarse_index.py:49)"
        self._dbidx = dbidx
        self.all_indices = FrozenBitMap(dbidx)
        self.device = device
        if _device_index is not None:
            assert _view_of is None and not _device_index.is_view
            assert (_device_index.n_rows, _device_index.dim) == self.vectors.shape and \
                _device_index.dtype == self.vector_dtype and _device_index.device == device
            self._dev = _device_index
        elif _view_of is not None:
            self._dev = _view_of[0].view(_view_of[1])
            assert self._dev.n_rows == self.vectors.shape[0]
        else:
            self._dev = DeviceIndex.from_numpy(self.vectors, device=device, dtype=self.vector_dtype)

    def __len__(self):
        return len(self.all_indices)

    def string2vec(self, string: str) -> np.ndarray:
        vec = self.embedding.from_string(string=string)
        return vec / np.linalg.norm(vec)

    def score(self, tvec) -> np.ndarray:
        return self._dev.scores(tvec)

    @staticmethod
    def from_path(index_path: str, *, use_vec_index=False, exclude=None, device: int = 0, vector_dtype: str = "float32",
                  **_):
        """<index>/vectors.npy [N,512] f32 + <index>/vector_meta.parquet (dbidx, ...) + info.json."""
        index_path = resolve_path(index_path)
        info = json.load(open(f"{index_path}/info.json"))
        from ...models.embeddings import load_embedding
        embedding = load_embedding(info.get("model"), device=device)
        vectors = np.load(f"{index_path}/vectors.npy", mmap_mode="r")
        meta = pd.read_parquet(f"{index_path}/vector_meta.parquet")
        assert meta.dbidx.is_monotonic_increasing, "sanity check"
        return CoarseIndex(embedding=embedding, vectors=np.asarray(vectors), vector_meta=meta,
                           path=index_path, device=device, vector_dtype=vector_dtype)

    def query(self, *, topk, vector=None, exclude=None, startk=None, **kwargs):
        exclude = BitMap() if exclude is None else exclude
        excl_pos = _positions_of(self._dbidx, np.asarray(exclude, dtype=np.int64))
        n_included = self._dbidx.shape[0] - excl_pos.shape[0]
        if n_included == 0:
            return np.array([]), np.array([])
        topk = min(int(topk), n_included)
        if vector is None:  # random order over the included images (coarse_index.py:70-71)
            mask = np.ones(self._dbidx.shape[0], dtype=bool)
            mask[excl_pos] = False
            pos = np.random.permutation(np.nonzero(mask)[0])[:topk]
            scores = np.random.randn(topk)
        else:
            pos, scores, _ = self._dev.topk(vector, topk, excluded=excl_pos)
        ret = self._dbidx[pos]
        assert ret.shape[0] == topk
        # one whole-image box per result (coarse_index.py:88-93), as lazily built one-row frames
        boxes = np.tile(np.array([[0, 0, 224, 224]], dtype=np.int64), (ret.shape[0], 1))
        return {"dbidxs": ret, "nextstartk": len(exclude) + ret.shape[0],
                "activations": ActivationFrames(boxes, ret, np.asarray(scores))}

    def query_batch(self, *, topk, vectors, excludes=None, prune=False, vectors2=None, **kwargs):
        """one `DeviceIndex.topk_batch` call for the vectors that are given (on a subset_view index one
        `DeviceIndex.view_topk_batch` call: the member rows read in place, once a chunk of queries; `prune` is consumed
        and means that plain view batch; a call with `vectors2` or `vector2` stays the loop over `query` there, as on a
        multiscale view index): the list of dicts `query` returns, entry by entry identical to it.  A `None`
        vector (random order) and a query whose exclude set covers the whole index
        keep going through `query`.  `prune` is `DeviceIndex.topk_batch`'s: the same results from the shared int8
        pre-scan on an index large enough for it.  `vectors2` is dropped: `query` ignores `vector2`."""
        vectors = list(vectors)
        excludes = [None] * len(vectors) if excludes is None else list(excludes)
        if len(excludes) != len(vectors):
            raise ValueError(f"excludes has {len(excludes)} entries for {len(vectors)} vectors")
        is_view = getattr(self._dev, "is_view", False)
        if is_view and (vectors2 is not None or kwargs.get("vector2") is not None):  # as on a multiscale view: the loop
            return [self.query(topk=topk, vector=v, exclude=e, **kwargs) for v, e in zip(vectors, excludes)]
        out = [None] * len(vectors)
        n = self._dbidx.shape[0]
        excl_pos = [_positions_of(self._dbidx, np.asarray(BitMap() if e is None else e, dtype=np.int64)) for e in excludes]
        batch = [i for i, v in enumerate(vectors) if v is not None and excl_pos[i].shape[0] < n]
        for i in range(len(vectors)):
            if i not in batch:
                out[i] = self.query(topk=topk, vector=vectors[i], exclude=excludes[i], **kwargs)
        if batch:
            Q = np.stack([np.asarray(vectors[i], dtype=np.float32).reshape(-1) for i in batch])
            # one k for the launch; every query keeps its own min(topk, included) results
            ks = [min(int(topk), n - excl_pos[i].shape[0]) for i in batch]
            if is_view:
                res = self._dev.view_topk_batch(Q, max(ks), excluded=[excl_pos[i] for i in batch])
            else:
                res = self._dev.topk_batch(Q, max(ks), excluded=[excl_pos[i] for i in batch], prune=prune)
            for i, k_i, (pos, scores, _) in zip(batch, ks, res):
                ret = self._dbidx[pos[:k_i]]
                assert ret.shape[0] == k_i
                boxes = np.tile(np.array([[0, 0, 224, 224]], dtype=np.int64), (ret.shape[0], 1))
                n_excl = 0 if excludes[i] is None else len(excludes[i])
                out[i] = {"dbidxs": ret, "nextstartk": n_excl + ret.shape[0],
                          "activations": ActivationFrames(boxes, ret, np.asarray(scores[:k_i]))}
        return out

    def new_query(self):
        return CoarseQuery(self)

    def subset(self, indices: BitMap):
        mask = np.isin(self._dbidx, np.asarray(indices, dtype=np.int64))
        return CoarseIndex(embedding=self.embedding, vectors=self.vectors[mask],
                           vector_meta=self.vector_meta[mask].reset_index(drop=True), device=self.device,
                           vector_dtype=self.vector_dtype)

    def subset_view(self, indices: BitMap):
        """`subset(indices)` whose device index is a view of this index's resident rows (DeviceIndex.view): no second
        copy of the member rows in HBM, no upload, the same results bit for bit; all of the index is the index itself"""
        mask = np.isin(self._dbidx, np.asarray(indices, dtype=np.int64))
        if mask.all():
            return self
        if getattr(self._dev, "is_view", False):
            raise NotImplementedError("subset_view of a subset view: take it from the index that holds the rows")
        return CoarseIndex(embedding=self.embedding, vectors=self.vectors[mask],
                           vector_meta=self.vector_meta[mask].reset_index(drop=True), device=self.device,
                           vector_dtype=self.vector_dtype, _view_of=(self._dev, np.nonzero(mask)[0]))


class CoarseQuery(InteractiveQuery):
    def __init__(self, db: CoarseIndex):
        super().__init__(db)

    def getXy(self, get_positions=False):
        seen = np.asarray(self.label_db.get_seen(), dtype=np.int64)
        positions = _positions_of(self.index._dbidx, seen)
        # the reference takes all_indices.rank(idx) - 1 for every seen id (coarse_index.py:116-118), which for
        # an id outside the index silently lands on its predecessor's vector; labels and vectors must pair up
        assert positions.shape[0] == seen.shape[0], "labels recorded for images that are not in this index"
        yt = np.array([len(self.label_db.get(int(d), format="box")) > 0 for d in seen], dtype=bool)
        if get_positions:
            return positions[yt], positions[~yt]
        return self.index.vectors[positions], yt.astype("float")
