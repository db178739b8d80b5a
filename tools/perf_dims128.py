#!/usr/bin/env python3
"""The scan at the dims that are multiples of 128 (384, 640, 896, 1152, 1280; csrc/scan.hip, scan_dims128.o) against its
yardsticks, in one process on one GPU ("Dims that are multiples of 128").

    python tools/perf_dims128.py [--rows 12500000] [--reps 15] [--nq 16] [--k 100]

Per row type (f32, f16) and new dim, one group: the new dim, dims 512 and 768 (the yardstick, resident throughout) and
the index a user had to zero-pad to before (dim 384 -> 512, 640 -> 768, 896 -> 1024; it scans that dim's bytes) take
turns in every round, in an order that rotates from round to round, after one untimed round.  One JSON line a case:

  scan_ms, scan_tbps   the single scan from the handle's event pairs (ssw_index_profile): median [interquartile range]
                       and the achieved rate over its row bytes (rows x dim x element size)
  batch_ms_per_query   host-to-host topk_batch at --nq queries, a query

and then the verdicts: each new dim's rate against the dim-512 / 768 yardsticks' of the same run (within their spread,
or the shortfall), and its scan time against the zero-padded index's (are the bytes saved time saved).  The rows are one
block of unit Gaussian rows repeated: the scan's time does not depend on the values."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW_DIMS, YARDSTICK_DIMS, PADDED_TO = (384, 640, 896, 1152, 1280), (512, 768), {384: 512, 640: 768, 896: 1024}


def resident(n, dim, dtype, block_rows=1 << 16):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex, _ptr
    idx = DeviceIndex(n, dim, dtype=dtype)
    block = np.random.default_rng(dim).standard_normal((block_rows, dim)).astype(np.float32)
    block /= np.linalg.norm(block, axis=1, keepdims=True)
    for r0 in range(0, n, block_rows):
        _lib.call("ssw_index_upload", idx._h, _ptr(block), r0, min(block_rows, n - r0))
    return idx


def quartiles(v):
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return float(med), float(q3 - q1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--nq", type=int, default=16)
    ap.add_argument("--k", type=int, default=100)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_dims128: no GPU (timings are not taken on a CPU)")
    for dtype in (np.float32, np.float16):
        yard = {d: resident(args.rows, d, dtype) for d in YARDSTICK_DIMS}  # resident throughout
        for d in NEW_DIMS:  # one group a new dim: it, the yardsticks and its zero-padded alternative take turns
            made = dict(yard)
            made[d] = resident(args.rows, d, dtype)
            if d in PADDED_TO and PADDED_TO[d] not in made:
                made[PADDED_TO[d]] = resident(args.rows, PADDED_TO[d], dtype)
            dims = sorted(made)
            scan, batch = {x: [] for x in dims}, {x: [] for x in dims}
            Q = {x: np.random.default_rng(1).standard_normal((args.nq, x)).astype(np.float32) for x in dims}
            for idx in made.values():
                idx.profile(True)
            for rep in range(args.reps + 1):
                for i in range(len(dims)):
                    x = dims[(i + rep) % len(dims)]
                    idx = made[x]
                    idx.profile_read()
                    idx.scan(Q[x][0])
                    idx.sync()
                    ms = idx.profile_read()
                    t0 = time.perf_counter()
                    idx.topk_batch(Q[x], args.k)
                    t = 1e3 * (time.perf_counter() - t0) / args.nq
                    if rep:
                        scan[x].append(float(ms[0]))
                        batch[x].append(t)
            res = {}
            for x in dims:
                med, iqr = quartiles(scan[x])
                bmed, biqr = quartiles(batch[x])
                tbps = args.rows * x * np.dtype(dtype).itemsize / med / 1e9
                res[x] = {"group": d, "dim": x, "dtype": np.dtype(dtype).name, "rows": args.rows, "reps": args.reps,
                          "scan_ms": round(med, 4), "scan_iqr": round(iqr, 4), "scan_tbps": round(tbps, 3),
                          "tbps_spread": round(tbps * iqr / med, 3), "nq": args.nq,
                          "batch_ms_per_query": round(bmed, 4), "batch_iqr": round(biqr, 4)}
                print(json.dumps(res[x]), flush=True)
            r = res[d]
            for y in YARDSTICK_DIMS:
                short = res[y]["scan_tbps"] - r["scan_tbps"]
                within = short <= res[y]["tbps_spread"] + r["tbps_spread"]
                print("%s dim %d vs dim %d: %.3f vs %.3f TB/s -- %s" % (
                    r["dtype"], d, y, r["scan_tbps"], res[y]["scan_tbps"],
                    "within the run's spread" if within else "short by %.1f %%" % (100 * short / res[y]["scan_tbps"])), flush=True)
            if d in PADDED_TO:
                rp = res[PADDED_TO[d]]
                print("%s dim %d vs zero-padded to %d: scan %.4f vs %.4f ms (%.3f of the padded time; the bytes are %.3f)" % (
                    r["dtype"], d, PADDED_TO[d], r["scan_ms"], rp["scan_ms"], r["scan_ms"] / rp["scan_ms"], d / PADDED_TO[d]),
                    flush=True)
            for x in dims:
                made[x].profile(False)
                if x not in yard:
                    made[x].close()
        for idx in yard.values():
            idx.close()


if __name__ == "__main__":
    main()
