#!/usr/bin/env python3
"""Launch shapes of the shadow scan (csrc/prune.hip, k_q8_bounds) on one index, interleaved.

    python tools/sweep_prune.py [--rows 100e6] [--k 100] [--reps 6]

One synthetic N x 512 f32 index; for every (four-wave blocks per CU, 16-byte loads a lane per group) the lab build
offers (ssw_tune_prune_scan) `reps` pruned top-k calls, the shapes taking turns so that drift hits all alike.  Prints
per shape the median and the spread of the HIP-event ms of the scan phase (shadow scan + threshold selection +
survivors + rescoring) and the shadow scan's share of it as TB/s over N x 520 B.  The first line is the product's."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2, 8), (1, 8), (3, 8), (4, 8), (1, 16), (2, 16), (2, 4), (4, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=100e6)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=6)
    args = ap.parse_args()
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex

    def query(i):
        q = np.random.default_rng(10_000 + i).standard_normal(512).astype(np.float32)
        return (q / np.linalg.norm(q)).astype(np.float32)

    n = int(args.rows)
    with _lib.debug_hooks():
        idx = DeviceIndex.synthetic(n, 512, seed=2024)
        try:
            _lib.call("ssw_tune_prune", 1, -1, -1)
            idx.topk(query(0), args.k)  # builds the shadow
            ms = {s: [] for s in SHAPES}
            for i in range(args.reps + 1):
                for s in SHAPES:
                    _lib.call("ssw_tune_prune_scan", s[0], s[1])
                    idx.profile(True)
                    idx.topk(query(1 + i), args.k)
                    t = idx.profile_read().tolist()
                    idx.profile(False)
                    if i:  # the first round warms every shape's code object
                        ms[s].extend(t)
            for s in SHAPES:
                v = np.asarray(ms[s])
                print(json.dumps({"rows": n, "blocks_per_cu": s[0], "group_loads": s[1],
                                  "scan_phase_ms_median": round(float(np.median(v)), 3),
                                  "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
                                  "phase_TBps": round(n * 520 / float(np.median(v)) * 1e-9, 3)}), flush=True)
        finally:
            _lib.call("ssw_tune_prune_scan", -1, -1)
            idx.close()


if __name__ == "__main__":
    main()
