"""The coarse index out of a finished multiscale index: interface of seesaw/indices/coarse/preprocessor.py:11-52
(infer_coarse_embedding, from_fine_grained), the one way the reference builds an `i_name="coarse"` index.

The reference reads the whole multiscale table into pandas, keeps each image's rows at `zoom_level == max_zoom_level`,
takes `groupby("dbidx").vectors.mean()` and divides by `np.maximum(norm, 1e-6)`.  Here the multiscale rows are resident
in HBM already, so the masked per-image mean runs there (DeviceIndex.coarse_mean, csrc/coarse.hip): the host sends one
mask byte a row and reads the `m x dim` result once; sums, mean, norm and division are float64 with one rounding to f32.
"""
from __future__ import annotations

import json
import os
import shutil

import numpy as np
import pandas as pd

from ...device_index import DeviceIndex, kept_images
from ..interface import resolve_path

COARSE_CONSTRUCTOR = "seesaw.indices.coarse.coarse_index.CoarseIndex"


def coarse_keep(vector_meta: pd.DataFrame) -> np.ndarray:
    """uint8 [n_rows]: 1 where `zoom_level == max_zoom_level` -- the COLUMN the tiler wrote, as preprocessor.py:15 reads
    it, not a maximum recomputed from the rows that are present"""
    if "max_zoom_level" not in vector_meta or "zoom_level" not in vector_meta:
        raise ValueError("the multiscale index's vector_meta needs the columns zoom_level and max_zoom_level "
                         "(vectors.sorted.cached as create_multiscale_index writes it)")
    return (vector_meta.zoom_level.values == vector_meta.max_zoom_level.values).astype(np.uint8)


def coarse_selection(row_dbidx: np.ndarray, keep: np.ndarray):
    """rows sorted by dbidx + their keep mask -> (positions int64 of the images with a kept row among the distinct
    dbidx in ascending order, their dbidx): an image without a row at its max_zoom_level is absent, as from the
    reference's groupby over the filtered frame"""
    row_dbidx = np.asarray(row_dbidx, dtype=np.int64)
    assert np.all(np.diff(row_dbidx) >= 0), "rows must be sorted by dbidx"
    dbidx, counts = np.unique(row_dbidx, return_counts=True)
    positions = kept_images(np.concatenate(([0], np.cumsum(counts))), keep)
    return positions, dbidx[positions]


def infer_coarse_embedding(index, vector_dtype="float32"):
    """MultiscaleIndex -> (DataFrame(dbidx), DeviceIndex): one normalised mean row per image that has a row at its
    max_zoom_level, in ascending dbidx order, derived on the device from the index's resident rows (an f32 or float16
    index, or a subset_view: its member rows are read in place).  `vector_dtype`: storage of the derived index."""
    dev = getattr(index, "_dev", None)
    if dev is None:
        raise NotImplementedError("this multiscale index holds no whole-matrix device index (a sharded index): derive "
                                  "the coarse index from the unsharded one")
    keep = coarse_keep(index.vector_meta)
    positions, dbidx = coarse_selection(index._row_dbidx, keep)
    if positions.shape[0] == 0:
        raise ValueError("no image has a row at its max_zoom_level")
    return pd.DataFrame({"dbidx": dbidx}), dev.coarse_mean(keep, images=positions, dtype=vector_dtype)


def from_fine_grained(fine_grained_path, output_path, device: int = 0, vector_dtype: str = "float32"):
    """<fine_grained_path> (a multiscale index, either on-disk layout MultiscaleIndex.from_path reads; resident as
    `vector_dtype`) -> <output_path>/{info.json, vectors.npy f32 [m, dim], vector_meta.parquet (dbidx)}, the layout
    CoarseIndex.from_path reads.  An existing output_path is refused (preprocessor.py:26); everything is written into
    the sibling `.tmp.<name>` and renamed at the end (:28-32, :52).  Returns the output path."""
    from ..multiscale.multiscale_index import MultiscaleIndex
    fine_grained_path = resolve_path(fine_grained_path)
    output_path = resolve_path(output_path).rstrip("/")
    assert os.path.isdir(fine_grained_path), fine_grained_path
    if os.path.exists(output_path):
        raise FileExistsError(output_path)
    outdir, outname = os.path.dirname(output_path), os.path.basename(output_path)
    tmp = os.path.join(outdir, f".tmp.{outname}")
    if os.path.exists(tmp):
        shutil.rmtree(tmp)
    src_info = json.load(open(f"{fine_grained_path}/info.json"))
    index = MultiscaleIndex.from_path(fine_grained_path, device=device, vector_dtype=vector_dtype)
    meta, dev = infer_coarse_embedding(index)
    try:
        vectors = dev.download()  # the one transfer of the result
    finally:
        dev.close()
    assert meta.dbidx.is_monotonic_increasing
    os.makedirs(tmp)
    info = {"constructor": COARSE_CONSTRUCTOR}
    info.update({k: src_info[k] for k in ("model", "dataset") if k in src_info})
    with open(f"{tmp}/info.json", "w") as f:
        json.dump(info, f, indent=2)
    np.save(f"{tmp}/vectors.npy", vectors)
    meta.to_parquet(f"{tmp}/vector_meta.parquet")
    os.rename(tmp, output_path)
    return output_path
