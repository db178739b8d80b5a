#!/usr/bin/env python3
"""MultiscaleIndex.query_batch against the per-query loop in one process ("Batched multiscale
query").

    python tools/perf_query_batch.py [--cases f32:1560000 f16:1560000 f32:4194304] [--nq 2 4 8 16] [--reps 9]
                                     [--warmup-pairs 2] [--topk 10] [--shortlist 50] [--prune]
    python tools/perf_query_batch.py --single [--cases ...] [--calls 20] [--warmup-calls 4]

For each case: a synthetic index of `rows` x 512 f32 or binary16 rows generated on the device, 13 tiles an image (a
1 + 4 + 8 pyramid of overlapping boxes); at 2^22 rows the single `query` is pruned by the int8 pre-scan, the batch
only with `--prune`.  For each nq and each of agg_method = plain_score and avg_score (aug_larger = "greater"): `warmup-pairs`
untimed pairs, then `reps` pairs of `index.query_batch(...)` and the loop `AccessMethod.query_batch(index, ...)` in
turn, every pair on fresh queries.  Both end with their results on the host, so the host clock around a call covers
the device work.  Prints one JSON line per configuration: wall ms per QUERY (median and min .. max of the reps) of
both forms, their ratio, and whether all entries were identical.  `--prune` times `query_batch(prune=True)` as a
third form beside them ("Pruned two-stage query"): the batch is the unpruned one, the loop is the loop of the pruned
`query`.

`--single` times the principal query by itself: `calls` calls of `index.query(agg_method="avg_score",
aug_larger="greater")` on fixed queries after `warmup-calls` untimed ones; one JSON line a case with the median and
min .. max wall ms of a call, a hash of all results, and the handle's prune counters.  It asks nothing of the library
that an older build lacks, so the same file times two builds in a process each (SSW_PRODUCT_LIB names the library)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILES = 13


def tile_meta(n_images):
    """13 tiles an image: the whole image, a 2 x 2 and a 4 x 2 grid of tiles 1.5 cells wide (neighbours overlap)"""
    w, h = 640.0, 480.0
    boxes, zoom = [(0.0, 0.0, w, h)], [0]
    for level, (gx, gy) in ((1, (2, 2)), (2, (4, 2))):
        sw, sh = w / gx * 1.5, h / gy * 1.5
        for iy in range(gy):
            for ix in range(gx):
                x1, y1 = ix * (w - sw) / (gx - 1), iy * (h - sh) / (gy - 1)
                boxes.append((x1, y1, x1 + sw, y1 + sh))
                zoom.append(level)
    b = np.tile(np.asarray(boxes, dtype=np.float32), (n_images, 1))
    return pd.DataFrame({"dbidx": np.repeat(np.arange(n_images, dtype=np.int64), TILES),
                         "zoom_level": np.tile(np.asarray(zoom, dtype=np.int16), n_images),
                         "x1": b[:, 0], "y1": b[:, 1], "x2": b[:, 2], "y2": b[:, 3]})


def make_index(rows, dtype):
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex

    class SyntheticMultiscale(MultiscaleIndex):
        def _init_device(self):  # the rows are generated on the device: no rows x 512 host matrix
            self._dev = DeviceIndex.synthetic(self._row_dbidx.shape[0], 512, seed=2024, dtype=self.vector_dtype)
            self._dev.set_row2image(self._row2pos.astype(np.int32))
            self._dev.set_tile_meta(self._box, self.vector_meta.zoom_level.values)

    n_images = -(-rows // TILES)
    meta = tile_meta(n_images)
    return SyntheticMultiscale(embedding=None, vectors=np.zeros((meta.shape[0], 0), dtype=np.float32), vector_meta=meta,
                               vector_dtype=dtype)


def queries(seed, nq):
    q = np.random.default_rng(seed).standard_normal((nq, 512)).astype(np.float32)
    return list((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32))


def identical(a, b):
    return len(a) == len(b) and all(np.array_equal(x["dbidxs"], y["dbidxs"]) and
                                    x["activations"].records() == y["activations"].records() for x, y in zip(a, b))


def result_hash(results):
    import hashlib
    h = hashlib.sha256()
    for r in results:
        h.update(np.ascontiguousarray(r["dbidxs"], dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(r["activations"].records()).tobytes())
    return h.hexdigest()[:16]


def single(args):
    kw = dict(topk=args.topk, shortlist_size=args.shortlist, agg_method="avg_score", aug_larger="greater",
              rescore_method=None)
    for case in args.cases:
        fmt, rows = case.split(":")
        index = make_index(int(rows), {"f32": "float32", "f16": "float16"}[fmt])
        try:
            vectors = queries(77, args.warmup_calls + args.calls)
            wall, out = [], []
            for i, v in enumerate(vectors):
                t0 = time.perf_counter()
                r = index.query(vector=v, exclude=None, **kw)
                if i >= args.warmup_calls:
                    wall.append(1e3 * (time.perf_counter() - t0))
                    out.append(r)
            try:
                st = index._dev.prune_stats(completions=True)
            except TypeError:  # a build from before ssw_index_prune_completions
                st = index._dev.prune_stats()
            print(json.dumps({"mode": "single", "rows": index._row_dbidx.shape[0], "dtype": fmt, "calls": len(wall),
                              "ms_median": round(float(np.median(wall)), 4),
                              "ms_min_max": [round(float(np.min(wall)), 4), round(float(np.max(wall)), 4)],
                              "hash": result_hash(out), "prune": st}), flush=True)
        finally:
            index._dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["f32:1560000", "f16:1560000", "f32:4194304"])
    ap.add_argument("--nq", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup-pairs", type=int, default=2)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--shortlist", type=int, default=50)
    ap.add_argument("--prune", action="store_true", help="also time query_batch(prune=True)")
    ap.add_argument("--single", action="store_true", help="time MultiscaleIndex.query (avg_score) by itself")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup-calls", type=int, default=4)
    args = ap.parse_args()
    if args.single:
        return single(args)
    from seesaw_amd.indices.interface import AccessMethod
    forms = ("batch", "loop", "pruned_batch") if args.prune else ("batch", "loop")

    seed = 0
    for case in args.cases:
        fmt, rows = case.split(":")
        index = make_index(int(rows), {"f32": "float32", "f16": "float16"}[fmt])
        try:
            for agg in ("plain_score", "avg_score"):
                kw = dict(topk=args.topk, shortlist_size=args.shortlist, agg_method=agg, aug_larger="greater",
                          rescore_method=None)
                for nq in args.nq:
                    wall = {form: [] for form in forms}
                    same = True
                    for i in range(-args.warmup_pairs, args.reps):
                        seed += 1
                        vectors = queries(seed, nq)
                        out = {}
                        for form in forms:
                            t0 = time.perf_counter()
                            if form == "batch":
                                out[form] = index.query_batch(vectors=vectors, **kw)
                            elif form == "pruned_batch":
                                out[form] = index.query_batch(vectors=vectors, prune=True, **kw)
                            else:
                                out[form] = AccessMethod.query_batch(index, vectors=vectors, **kw)
                            if i >= 0:
                                wall[form].append(1e3 * (time.perf_counter() - t0) / nq)
                        same = same and all(identical(out[form], out["loop"]) for form in forms)
                    res = {"rows": index._row_dbidx.shape[0], "dtype": fmt, "agg_method": agg, "nq": nq,
                           "single_query_pruned": bool(index._dev.prune_stats()["queries"] > 0)}
                    for form in forms:
                        res[f"{form}_ms_per_query_median"] = round(float(np.median(wall[form])), 4)
                        res[f"{form}_ms_per_query_min_max"] = [round(float(np.min(wall[form])), 4),
                                                               round(float(np.max(wall[form])), 4)]
                    res["batch_over_loop"] = round(res["batch_ms_per_query_median"] / res["loop_ms_per_query_median"], 3)
                    if args.prune:
                        res["pruned_batch_over_loop"] = round(res["pruned_batch_ms_per_query_median"] /
                                                              res["loop_ms_per_query_median"], 3)
                        res["pruned_batch_over_batch"] = round(res["pruned_batch_ms_per_query_median"] /
                                                               res["batch_ms_per_query_median"], 3)
                    res["identical"] = bool(same)
                    print(json.dumps(res), flush=True)
        finally:
            index._dev.close()


if __name__ == "__main__":
    main()
