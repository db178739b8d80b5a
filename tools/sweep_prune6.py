#!/usr/bin/env python3
"""Launch shapes of the 6-bit shadow scan (csrc/prune.hip, k_q6_bounds) on one index, the shapes taking turns.

    python tools/sweep_prune6.py [--rows 100e6] [--dim 512] [--dtype float32|float16] [--k 100] [--reps 6]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/sweep_prune6.py ...
    python tools/sweep_prune6.py --trace DIR        # the kernel times of such a run, per shape

One synthetic N x dim index; for every (four-wave blocks per CU, 16-row tiles a request) the lab build offers at that
dim (ssw_tune_prune6_scan; tiles * dim <= 1024) one warm-up round and `reps` rounds of pruned top-k calls, a call a shape
a round, so that drift hits all shapes alike.  Prints per shape the median and the spread (max - min) of the host wall ms
of a call; the first line is the product's shape.  Under rocprofv3 the same run gives the kernel's own time: --trace reads
the kernel trace and prints, per k_q6_bounds instance and grid size (= blocks), calls, median, min and max us with the
warm-up round's launch dropped."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_trace(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                m = re.search(r"k_q6_bounds(?:_mq)?<[^>]*>", r["Kernel_Name"])
                if not m:
                    continue
                grid, wg = r.get("Grid_Size_X") or r["Grid_Size"], r.get("Workgroup_Size_X") or r["Workgroup_Size"]
                blocks = int(grid) // max(1, int(wg))
                rows.setdefault((m.group(0), blocks), []).append(
                    (int(r["Start_Timestamp"]), 1e-3 * (int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))))
    for (name, blocks), v in sorted(rows.items()):
        us = np.asarray([d for _, d in sorted(v)][1:])  # without the warm-up round's launch
        if us.size:
            print(json.dumps({"kernel": name, "blocks": blocks, "calls": int(us.size),
                              "us_median": round(float(np.median(us)), 1), "us_min": round(float(us.min()), 1),
                              "us_max": round(float(us.max()), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=100e6)
    ap.add_argument("--dim", type=int, default=512, choices=(256, 512, 1024))
    ap.add_argument("--dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--trace", metavar="DIR")
    args = ap.parse_args()
    if args.trace:
        read_trace(args.trace)
        return
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex

    def query(i):
        q = np.random.default_rng(10_000 + i).standard_normal(args.dim).astype(np.float32)
        return (q / np.linalg.norm(q)).astype(np.float32)

    n = int(args.rows)
    shapes = [(-1, -1)] + [(b, t) for t in (1, 2, 4) if t * args.dim <= 1024 for b in args.blocks]
    with _lib.debug_hooks():
        idx = DeviceIndex.synthetic(n, args.dim, seed=2024, dtype=np.dtype(args.dtype))
        try:
            _lib.call("ssw_tune_prune", 1, 1, -1)
            _lib.call("ssw_tune_prune6", 1, 1)
            idx.topk(query(0), args.k)  # builds the shadow
            ms = {s: [] for s in shapes}
            surv = []
            for i in range(args.reps + 1):
                for s in shapes:
                    _lib.call("ssw_tune_prune6_scan", s[0], s[1])
                    t0 = time.perf_counter()
                    idx.topk(query(1 + i), args.k)
                    dt = 1e3 * (time.perf_counter() - t0)
                    if i:  # the first round warms every shape's code object
                        ms[s].append(dt)
                surv.append(idx.prune_stats()["last_survivors"])
            st = idx.prune_stats()
            for s in shapes:
                v = np.asarray(ms[s])
                print(json.dumps({"rows": n, "dim": args.dim, "dtype": args.dtype, "blocks_per_cu": s[0], "tiles": s[1],
                                  "call_ms_median": round(float(np.median(v)), 3),
                                  "spread": round(float(v.max() - v.min()), 3), "survivors": surv[-1],
                                  "fallbacks": st["fallbacks"], "shadow_bytes": st["shadow_bytes"]}), flush=True)
        finally:
            _lib.call("ssw_tune_prune6_scan", -1, -1)
            _lib.call("ssw_tune_prune", 1, -1, -1)
            _lib.call("ssw_tune_prune6", 1, -1)
            idx.close()


if __name__ == "__main__":
    main()
