#!/usr/bin/env python3
"""The sharded batch with its second stage against the per-query loop, in one process ("Sharded
batch: second stage"; ssw_index_stage2_avg_batch_dev).

    python tools/perf_sharded_stage2.py [--rows 12.5e6] [--dtype float32] [--reps 9] [--prune] [--out FILE]

World 1 with the collectives of the exchange forced over RCCL: one rank's share of the 8-GPU configuration (12.5 M x
512 rows generated on the device, 13 tiles an image as in tools/perf_query_batch.py).  One row format per invocation
(run each under its own `timeout`, chained with `&&`).  The query is the principal one: `agg_method="avg_score"`,
`aug_larger="greater"`, shortlist 50, topk 10.  For nq = 2 / 4 / 8 / 16:

  A  `index.query_batch(vectors=Q[:nq], ...)`: the rows read once per chunk, ONE all-gather and ONE merge launch, then
     ONE stage-2 launch, ONE more all-gather and one host combine (with --prune: `prune=True`, the chunk's first stage
     from the certified pre-scan);
  B  `AccessMethod.query_batch(index, vectors=Q[:nq], ...)`: the per-query loop -- nq scans (pruned by themselves on an
     index of this size), all-gathers and merges, nq `rescore_avg` calls.  NOTE: at world 1 the loop's own stage-2
     gather is skipped by `_gather_stage2` (it needs no collective there), so B pays one collective a query, not two;
     on more ranks it pays both.

A and B alternate after two warm-up rounds; one JSON line per nq with the median, minimum, quartiles and max - min
spread of the wall ms per query of either form, the ratio of the medians and whether both returned the same entries.
The raw lines are appended to --out (profiles/sharded_batch_stage2_ab.txt).  `--trace-only N` runs N batched calls of 16
queries and nothing else, for a kernel trace of its own."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NQS = (2, 4, 8, 16)


def spread(ms):
    a = np.sort(np.asarray(ms))
    return {"median": float(np.median(a)), "min": float(a[0]), "q1": float(np.percentile(a, 25)),
            "q3": float(np.percentile(a, 75)), "max": float(a[-1]), "spread": float(a[-1] - a[0])}


def make_index(rows, dtype):
    import torch
    from perf_query_batch import TILES, tile_meta
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.indices.multiscale.sharded_index import DeviceShard, ShardedMultiscaleIndex
    from seesaw_amd.sharded import _DevArray

    class SyntheticShard(DeviceShard):
        def __init__(self, vectors, row2image, boxes, zoom, device, vector_dtype="float32"):
            # the rows are generated on the device: no rows x 512 host matrix (`vectors` is a [rows, 0] placeholder)
            self.torch, self.tdev = torch, torch.device("cuda", device)
            self.index = DeviceIndex.synthetic(row2image.shape[0], 512, seed=2024, device=device, dtype=vector_dtype)
            self.index.set_row2image(row2image.astype(np.int32))
            self.index.set_tile_meta(boxes, zoom)
            self.index.set_stream(torch.cuda.current_stream(self.tdev).cuda_stream)
            keys_ptr, count_ptr, best_ptr = self.index.result_ptrs()
            self.keys = torch.as_tensor(_DevArray(keys_ptr, (_lib.SSW_MAX_TOPK,), "<i8"), device=self.tdev)
            self.count = torch.as_tensor(_DevArray(count_ptr, (2,), "<i4"), device=self.tdev)
            self.best = torch.as_tensor(_DevArray(best_ptr, (_lib.SSW_MAX_TOPK,), "<i4"), device=self.tdev)

    meta = tile_meta(-(-rows // TILES))
    index = ShardedMultiscaleIndex(embedding=None, vectors=None, local_vectors=np.zeros((meta.shape[0], 0), dtype=np.float32),
                                   vector_meta=meta, rank=0, world=1, device=0, k_max=128, vector_dtype=dtype,
                                   shard_factory=SyntheticShard)
    index._xchg.force_collective = True  # world 1, but the all-gathers are really issued
    return index


def identical(a, b):
    return len(a) == len(b) and all(np.array_equal(x["dbidxs"], y["dbidxs"]) and
                                    x["activations"].records() == y["activations"].records() for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=12.5e6)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--prune", action="store_true", help="the batch's first stage from the certified pre-scan")
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_batch_stage2_ab.txt"))
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    from seesaw_amd.indices.interface import AccessMethod

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    index = make_index(int(args.rows), args.dtype)
    rng = np.random.default_rng(4242)
    Q = rng.standard_normal((max(NQS), 512)).astype(np.float32)
    Q = list(np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32))
    kw = dict(topk=10, shortlist_size=50, agg_method="avg_score", aug_larger="greater", rescore_method=None)
    bkw = dict(kw, prune=True) if args.prune else kw

    def batch(nq):
        t0 = time.perf_counter()
        res = index.query_batch(vectors=Q[:nq], **bkw)
        return (time.perf_counter() - t0) * 1e3 / nq, res

    def loop(nq):
        t0 = time.perf_counter()
        res = AccessMethod.query_batch(index, vectors=Q[:nq], **kw)
        return (time.perf_counter() - t0) * 1e3 / nq, res

    if args.trace_only:
        for _ in range(args.trace_only):
            batch(16)
        index.close()
        dist.destroy_process_group()
        return
    with open(args.out, "a") as f:
        for nq in NQS:
            for _ in range(2):
                batch(nq), loop(nq)
            a_ms, b_ms, same = [], [], True
            for _ in range(args.reps):
                ta, ra = batch(nq)
                tb, rb = loop(nq)
                a_ms.append(ta), b_ms.append(tb)
                same = same and identical(ra, rb)
            a, b = spread(a_ms), spread(b_ms)
            line = json.dumps({"rows": int(args.rows), "dtype": args.dtype, "prune": bool(args.prune), "nq": nq,
                               "agg_method": "avg_score", "aug_larger": "greater", "shortlist": 50, "topk": 10,
                               "batch_ms_per_query": a, "loop_ms_per_query": b,
                               "loop_over_batch": b["median"] / a["median"], "identical": bool(same),
                               "prune_stats": index._shard.index.prune_stats(completions=True)})
            print(line, flush=True)
            f.write(line + "\n")
    index.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
