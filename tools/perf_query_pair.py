#!/usr/bin/env python3
"""MultiscaleIndex.query_batch(vectors2=...) against the loop of query(vector=, vector2=) in one process (DESIGN.md
section 4, "Batched two-vector query").

    python tools/perf_query_pair.py [--cases f32:1560000 f32:4194304:prune f16:1560000] [--nq 2 4 8 16] [--reps 9]
                                    [--warmup-rounds 2] [--topk 10] [--shortlist 50]

The index of a case is tools/perf_query_batch.py's: `rows` x 512 f32 or binary16 rows generated on the device, 13 tiles
an image.  `:prune` times `query_batch(prune=True, vectors2=...)`; the loop beside it is the loop of single queries,
which on an index of at least 2^22 rows are pruned by themselves.  For each nq and each of agg_method = plain_score and
avg_score (aug_larger = "greater"): `warmup-rounds` untimed rounds, then `reps` rounds of the batch and the loop in turn,
every round on fresh vector pairs.  Both end with their results on the host, so the host clock around a call covers the
device work.  Prints one JSON line per configuration: wall ms per QUERY of both forms (median, max - min of the reps),
their ratio, and whether every entry of every round was identical (dbidxs, activation boxes, activation score bits)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from perf_query_batch import make_index, queries  # noqa: E402


def records(acts):
    if hasattr(acts, "records"):
        return np.asarray(acts.records(), dtype=np.float64)
    return np.asarray([a[["x1", "y1", "x2", "y2", "score"]].to_numpy(dtype=np.float64)[0] for a in acts]).reshape(-1, 5)


def identical(a, b):
    return len(a) == len(b) and all(np.array_equal(x["dbidxs"], y["dbidxs"]) and
                                    np.array_equal(records(x["activations"]).view(np.uint64),
                                                   records(y["activations"]).view(np.uint64)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["f32:1560000", "f32:4194304:prune", "f16:1560000"])
    ap.add_argument("--nq", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup-rounds", type=int, default=2)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--shortlist", type=int, default=50)
    args = ap.parse_args()
    seed = 0
    for case in args.cases:
        fmt, rows, *flags = case.split(":")
        prune = "prune" in flags
        index = make_index(int(rows), {"f32": "float32", "f16": "float16"}[fmt])
        try:
            for agg in ("plain_score", "avg_score"):
                kw = dict(topk=args.topk, shortlist_size=args.shortlist, agg_method=agg, aug_larger="greater",
                          rescore_method=None)
                for nq in args.nq:
                    wall = {"batch": [], "loop": []}
                    same = True
                    for i in range(-args.warmup_rounds, args.reps):
                        seed += 2
                        vectors = queries(seed, nq)
                        second = [np.float32(0.5) * v for v in queries(seed + 1, nq)]
                        t0 = time.perf_counter()
                        got = index.query_batch(vectors=vectors, vectors2=second, prune=prune, **kw)
                        t1 = time.perf_counter()
                        ref = [index.query(vector=v, vector2=v2, exclude=None, **kw) for v, v2 in zip(vectors, second)]
                        t2 = time.perf_counter()
                        if i >= 0:
                            wall["batch"].append(1e3 * (t1 - t0) / nq)
                            wall["loop"].append(1e3 * (t2 - t1) / nq)
                        same = same and identical(got, ref)
                    st = index._dev.prune_stats()
                    res = {"rows": index._row_dbidx.shape[0], "dtype": fmt, "agg_method": agg, "nq": nq,
                           "batch_pruned": prune, "single_query_pruned": bool(st["eligible"])}
                    for form in ("batch", "loop"):
                        res[f"{form}_ms_per_query_median"] = round(float(np.median(wall[form])), 4)
                        res[f"{form}_ms_per_query_max_minus_min"] = round(float(np.max(wall[form]) - np.min(wall[form])), 4)
                    res["batch_over_loop"] = round(res["batch_ms_per_query_median"] / res["loop_ms_per_query_median"], 3)
                    res["identical"] = bool(same)
                    print(json.dumps(res), flush=True)
        finally:
            index._dev.close()


if __name__ == "__main__":
    main()
