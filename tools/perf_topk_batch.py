#!/usr/bin/env python3
"""Batched against single-query scan and top-k in one process (csrc/scan.hip: batch_scores_kernel; DESIGN.md section 4,
"Batched scan").

    python tools/perf_topk_batch.py --rows 12.5e6 --dtype float32 [--dim 768] [--blocks-per-cu 1 2] [--k 100] [--reps 7]
                                    [--pmc-only W]

One index size and row format per invocation (run each under its own `timeout`, chained with `&&`); one JSON line per
measurement, interleaved A/B, one warm-up round, medians:

  "scan"  for every chunk width W in 1, 2, 4, 8, 16 (the lab build's ssw_tune_scan_batch; 1 = the single-query kernel):
          HIP-event ms of ONE launch that scores W queries, ms per query, and the ratio to the single-query launch.
          Widths above the widest instance of the (dim, row format) are left out (the hook clamps them, so a request
          for them is more than one launch); with several --blocks-per-cu values every (W, blocks) pair is a variant
          of the same interleaved rounds.
  "topk"  for nq in 1, 2, 4, 8, 16: wall ms of one topk_batch(nq) at the product's width against nq topk calls as the
          product runs them (pruned where the index is eligible) and against nq full-scan topk calls; per query; and
          whether all three returned the same images, scores and rows.

SSW_TOPK_FULL_SCAN=1 in the environment makes the "as the product runs them" column a full scan too (a separate process).
--pmc-only W runs nothing but a few W-wide scan launches: the body for `rocprofv3 --pmc FETCH_SIZE -- ...` and, in a pass
of its own, `--pmc WRITE_SIZE` (both counters in one pass are refused by the profiler)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, required=True)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16"])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pmc-only", type=int, default=0)
    ap.add_argument("--dim", type=int, default=512, choices=[256, 512, 768, 1024])
    ap.add_argument("--blocks-per-cu", type=int, nargs="+", default=[-1],
                    help="of the multi-query kernel in the scan sweep (-1: the product's); several: all in one sweep")
    ap.add_argument("--scan-only", action="store_true")
    args = ap.parse_args()
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex

    n = int(args.rows)
    rng = np.random.default_rng(4242)
    Q = rng.standard_normal((max(WIDTHS), args.dim)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    qp = ctypes.c_void_p(Q.ctypes.data)
    tag = {"rows": n, "dim": args.dim, "dtype": args.dtype, "full_scan_env": bool(os.environ.get("SSW_TOPK_FULL_SCAN"))}

    with _lib.debug_hooks():
        idx = DeviceIndex.synthetic(n, args.dim, seed=2024, dtype=np.dtype(args.dtype))
        try:
            def scan(w, per_cu=args.blocks_per_cu[0]):
                _lib.call("ssw_tune_scan_batch", w, per_cu)
                if w == 1:
                    _lib.call("ssw_index_scan", idx._h, qp, None)
                else:
                    _lib.call("ssw_index_scan_batch", idx._h, qp, w, None)

            if args.pmc_only:
                for _ in range(5):
                    scan(args.pmc_only)
                print(json.dumps({**tag, "what": "pmc", "width": args.pmc_only, "launches": 5,
                                  "row_bytes_per_launch": n * args.dim * np.dtype(args.dtype).itemsize,
                                  "score_bytes_per_launch": n * 4 * args.pmc_only}), flush=True)
                return

            # (a) the kernels, by HIP events around each launch
            variants = [(1, -1)] + [(w, c) for w in WIDTHS[1:] for c in args.blocks_per_cu]
            ev = {v: [] for v in variants}
            for rep in range(args.reps + 1):
                for v in list(ev):
                    idx.profile(True)
                    scan(*v)
                    ms = idx.profile_read().tolist()
                    idx.profile(False)
                    if rep == 0 and len(ms) != 1:  # wider than the widest instance of this shape: clamped, not one launch
                        del ev[v]
                        continue
                    assert len(ms) == 1, (v, ms)  # one event pair per launch
                    if rep:
                        ev[v].append(ms[0])
            single = float(np.median(ev[(1, -1)]))
            row_bytes = n * args.dim * np.dtype(args.dtype).itemsize
            for (w, per_cu), t in ev.items():
                ms = float(np.median(t))
                print(json.dumps({**tag, "what": "scan", "width": w, "blocks_per_cu": per_cu, "launch_ms": round(ms, 4),
                                  "ms_per_query": round(ms / w, 4), "over_single_launch": round(ms / single, 4),
                                  "row_TBps": round(row_bytes / ms / 1e9, 3), "min_ms": round(min(t), 4),
                                  "max_ms": round(max(t), 4)}), flush=True)

            if args.scan_only:
                return
            # (b) the calls, by the host's clock
            _lib.call("ssw_tune_scan_batch", -1, -1)
            _lib.call("ssw_tune_prune", 1, -1, -1)
            idx.topk(Q[0], args.k)  # builds the shadow where the index is eligible
            st = np.zeros(6, dtype=np.int64)
            _lib.call("ssw_index_prune_stats", idx._h, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
            for nq in WIDTHS:
                wall = {"batch": [], "singles": [], "singles_full": []}
                same = True
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    a = idx.topk_batch(Q[:nq], args.k)
                    t1 = time.perf_counter()
                    b = [idx.topk(q, args.k) for q in Q[:nq]]
                    t2 = time.perf_counter()
                    _lib.call("ssw_tune_prune", 0, -1, -1)
                    t3 = time.perf_counter()
                    c = [idx.topk(q, args.k) for q in Q[:nq]]
                    t4 = time.perf_counter()
                    _lib.call("ssw_tune_prune", 1, -1, -1)
                    if rep:
                        wall["batch"].append(1e3 * (t1 - t0))
                        wall["singles"].append(1e3 * (t2 - t1))
                        wall["singles_full"].append(1e3 * (t4 - t3))
                    for x, y, z in zip(a, b, c):
                        same = same and all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) and
                                            np.array_equal(np.asarray(u).view(np.uint8), np.asarray(t).view(np.uint8))
                                            for u, v, t in zip(x, y, z))
                med = {key: float(np.median(v)) for key, v in wall.items()}
                print(json.dumps({**tag, "what": "topk", "nq": nq, "k": args.k, "singles_pruned": bool(st[1]) and not tag["full_scan_env"],
                                  "batch_ms": round(med["batch"], 3), "singles_ms": round(med["singles"], 3),
                                  "singles_full_ms": round(med["singles_full"], 3),
                                  "batch_ms_per_query": round(med["batch"] / nq, 3),
                                  "singles_ms_per_query": round(med["singles"] / nq, 3),
                                  "singles_full_ms_per_query": round(med["singles_full"] / nq, 3),
                                  "identical": bool(same)}), flush=True)
        finally:
            _lib.call("ssw_tune_scan_batch", -1, -1)
            _lib.call("ssw_tune_prune", 1, -1, -1)
            idx.close()


if __name__ == "__main__":
    main()
