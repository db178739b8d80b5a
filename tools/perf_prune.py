#!/usr/bin/env python3
"""Pruned against full-scan top-k in one process (csrc/prune.hip).

    python tools/perf_prune.py [--rows 12.5e6 25e6 50e6 100e6] [--k 100] [--reps 10] [--dtype float32|float16]
                               [--warmup-pairs 2]

For each index size: a synthetic N x 512 index of f32 or binary16 rows, one first top-k (builds the int8 shadow, timed
on its own), `warmup-pairs` untimed pairs, then `reps` pairs of top-k calls with the pruning switched off and on in turn
(the lab build's ssw_tune_prune; the threshold is lowered to 1 row so that every size is pruned), each a different
query.  Prints per size: host wall ms per call (median, and the spread min .. max), the HIP-event ms of the scan phase
(the full scan, or shadow scan + threshold selection + survivors + rescoring), survivors and fallbacks, and whether
both forms returned the same images, scores and best rows."""
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
    ap.add_argument("--rows", type=float, nargs="+", default=[12.5e6, 25e6, 50e6, 100e6])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--warmup-pairs", type=int, default=2)
    args = ap.parse_args()
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex

    def stats(idx):
        out = np.zeros(6, dtype=np.int64)
        _lib.call("ssw_index_prune_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return out

    def query(i):
        q = np.random.default_rng(10_000 + i).standard_normal(512).astype(np.float32)
        return (q / np.linalg.norm(q)).astype(np.float32)

    with _lib.debug_hooks():
        for rows in args.rows:
            n = int(rows)
            idx = DeviceIndex.synthetic(n, 512, seed=2024, dtype=np.dtype(args.dtype))
            try:
                _lib.call("ssw_tune_prune", 1, 1, -1)
                t0 = time.perf_counter()
                idx.topk(query(0), args.k)
                first_ms = 1e3 * (time.perf_counter() - t0)
                res = {"rows": n, "dtype": args.dtype, "k": args.k, "first_call_ms_with_shadow_build": round(first_ms, 2),
                       "shadow_bytes": int(stats(idx)[5])}
                wall = {0: [], 1: []}
                ev = {0: [], 1: []}
                surv, same = [], True
                for i in range(-args.warmup_pairs, args.reps):
                    q = query(1 + args.warmup_pairs + i)
                    out = {}
                    for on in (0, 1):
                        _lib.call("ssw_tune_prune", on, 1, -1)
                        if i < 0:
                            idx.topk(q, args.k)
                            continue
                        idx.profile(True)
                        t0 = time.perf_counter()
                        out[on] = idx.topk(q, args.k)
                        wall[on].append(1e3 * (time.perf_counter() - t0))
                        ev[on].extend(idx.profile_read().tolist())
                        idx.profile(False)
                        if on:
                            surv.append(int(stats(idx)[2]))
                    if i < 0:
                        continue
                    same = same and all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
                                        for a, b in zip(out[0], out[1]))
                st = stats(idx)
                res.update({
                    "full_ms_wall_median": round(float(np.median(wall[0])), 3),
                    "full_ms_wall_min_max": [round(float(np.min(wall[0])), 3), round(float(np.max(wall[0])), 3)],
                    "pruned_ms_wall_median": round(float(np.median(wall[1])), 3),
                    "pruned_ms_wall_min_max": [round(float(np.min(wall[1])), 3), round(float(np.max(wall[1])), 3)],
                    "full_scan_phase_ms_median": round(float(np.median(ev[0])), 3),
                    "pruned_scan_phase_ms_median": round(float(np.median(ev[1])), 3),
                    "survivors": surv, "pruned_calls": int(st[3]), "fallbacks": int(st[4]),
                    "identical": bool(same),
                })
                print(json.dumps(res), flush=True)
            finally:
                _lib.call("ssw_tune_prune", 1, -1, -1)
                idx.close()


if __name__ == "__main__":
    main()
