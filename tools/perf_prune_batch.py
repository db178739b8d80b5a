#!/usr/bin/env python3
"""The pruned batch against the plain batch and against pruned single calls, in one process (csrc/prune.hip
k_q8_bounds_mq, DESIGN.md section 4, "Pruned batch").

    python tools/perf_prune_batch.py [--rows 4194304 ... 100e6] [--nq 2 4 8 16 64] [--k 100] [--reps 7]
                                     [--dtype float32|float16] [--warmup-rounds 2] [--tiles T] [--blocks B]

For each index size: a synthetic N x 512 index, one first pruned call (builds the int8 shadow), then per nq
`warmup-rounds` untimed rounds and `reps` timed rounds; a round runs the three variants in turn on the same handle with
fresh queries -- topk_batch(prune=True), topk_batch (plain), nq pruned single topk calls.  The lab build lowers the
thresholds to 1 row so that every size is pruned (ssw_tune_prune).  Prints one JSON line per (size, nq): host wall ms
PER QUERY of each variant (median, min, max), the HIP-event ms per chunk of the pruned batch's replacement of the scan,
survivors per query, fallbacks, and whether all three returned the same bits."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, nargs="+", default=[1 << 22, 1 << 23, 12.5e6, 1 << 24, 25e6, 50e6, 100e6])
    ap.add_argument("--nq", type=int, nargs="+", default=[2, 4, 8, 16, 64])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--warmup-rounds", type=int, default=2)
    ap.add_argument("--tiles", type=int, default=-1)
    ap.add_argument("--blocks", type=int, default=-1)
    args = ap.parse_args()
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex

    def stats(idx):
        out = np.zeros(6, dtype=np.int64)
        _lib.call("ssw_index_prune_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return out

    def queries(seed, nq):
        Q = np.random.default_rng(10_000 + seed).standard_normal((nq, 512)).astype(np.float32)
        return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)

    def same(a, b):
        return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
                   for ra, rb in zip(a, b) for x, y in zip(ra, rb))

    with _lib.debug_hooks():
        _lib.call("ssw_tune_prune_scan_mq", args.blocks, args.tiles)
        for rows in args.rows:
            n = int(rows)
            idx = DeviceIndex.synthetic(n, 512, seed=2024, dtype=np.dtype(args.dtype))
            try:
                _lib.call("ssw_tune_prune", 1, 1, -1)
                idx.topk(queries(0, 1)[0], args.k)
                seed = 1
                for nq in args.nq:
                    wall = {"pruned_batch": [], "plain_batch": [], "pruned_singles": []}
                    ev, surv, identical = [], [], True
                    st0 = stats(idx)
                    for r in range(-args.warmup_rounds, args.reps):
                        Q = queries(seed, nq)
                        seed += 1
                        out = {}
                        idx.profile(True)
                        t0 = time.perf_counter()
                        out["pruned_batch"] = idx.topk_batch(Q, args.k, prune=True)
                        t1 = time.perf_counter()
                        chunk_ms = idx.profile_read().tolist()
                        idx.profile(False)
                        last = int(stats(idx)[2])
                        t2 = time.perf_counter()
                        out["plain_batch"] = idx.topk_batch(Q, args.k)
                        t3 = time.perf_counter()
                        out["pruned_singles"] = [idx.topk(q, args.k) for q in Q]
                        t4 = time.perf_counter()
                        if r < 0:
                            continue
                        wall["pruned_batch"].append(1e3 * (t1 - t0) / nq)
                        wall["plain_batch"].append(1e3 * (t3 - t2) / nq)
                        wall["pruned_singles"].append(1e3 * (t4 - t3) / nq)
                        ev.extend(chunk_ms)
                        surv.append(last)
                        identical = identical and same(out["pruned_batch"], out["plain_batch"]) and \
                            same(out["pruned_batch"], out["pruned_singles"])
                    st = stats(idx)
                    res = {"rows": n, "dtype": args.dtype, "k": args.k, "nq": nq}
                    for name, v in wall.items():
                        res[name + "_ms_per_query"] = [round(float(np.median(v)), 3), round(float(np.min(v)), 3),
                                                       round(float(np.max(v)), 3)]
                    res.update({"pruned_batch_chunk_event_ms_median": round(float(np.median(ev)), 3) if ev else None,
                                "last_query_survivors": surv, "pruned_queries": int(st[3] - st0[3]),
                                "fallbacks": int(st[4] - st0[4]), "identical": bool(identical)})
                    print(json.dumps(res), flush=True)
            finally:
                _lib.call("ssw_tune_prune", 1, -1, -1)
                idx.close()
        _lib.call("ssw_tune_prune_scan_mq", -1, -1)


if __name__ == "__main__":
    main()
