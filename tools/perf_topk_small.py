#!/usr/bin/env python3
"""Host-to-host time of one top-k call on a small index (1 000 images x 13 rows x 512: the one-launch form of
csrc/index_topk.hip), call by call.

    python tools/perf_topk_small.py [--calls 5000] [--k 50]

A call costs tens of microseconds, nearly all of it host code and launch latency, so this is where host-side overhead in
the top-k path shows.  Three loops after 200 untimed calls each: topk(q), topk(q) with 25 excluded images, and topk(None)
over the resident scores.  One JSON line: per loop the median, the 10th and 90th percentile and the mean, in us."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--k", type=int, default=50)
    args = ap.parse_args()
    from seesaw_amd.device_index import DeviceIndex

    n_images, tiles, dim = 1000, 13, 512
    idx = DeviceIndex.synthetic(n_images * tiles, dim, seed=4)
    idx.set_row2image(np.repeat(np.arange(n_images), tiles).astype(np.int32))
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((64, dim)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    excluded = np.sort(rng.choice(n_images, 25, replace=False)).tolist()
    out = {"rows": n_images * tiles, "images": n_images, "dim": dim, "k": args.k, "calls": args.calls}
    try:
        for tag, call in (("topk_q", lambda i: idx.topk(Q[i % 64], args.k)),
                          ("topk_q_excluded_25", lambda i: idx.topk(Q[i % 64], args.k, excluded=excluded)),
                          ("topk_resident", lambda i: idx.topk(None, args.k))):
            for i in range(200):
                call(i)
            us = np.empty(args.calls)
            for i in range(args.calls):
                t0 = time.perf_counter()
                call(i)
                us[i] = 1e6 * (time.perf_counter() - t0)
            out[tag + "_us"] = {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2),
                                "p90": round(float(np.percentile(us, 90)), 2), "mean": round(float(us.mean()), 2)}
    finally:
        idx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
