#!/usr/bin/env python3
"""Top-k across S views of one parent in one call (DeviceIndex.views_topk_batch; csrc/scan.hip: views_small_kernel /
views_stream_kernel) against the loop of `view.topk` it stands in for, in one process on one GPU (DESIGN.md section 4,
"Top-k across views of one parent").  SessionGroup.MIN_VIEW_GROUP is read from this tool's output.

    python tools/perf_views_batch.py [--reps 31] [--k 50] [--dtypes float32 float16] [--chunk-select]

Parent: 120 000 images x 13 tiles = 1.56 M rows at dim 512.  Views: sixteen seeded random sets of 1 109 images
(14 417 rows: an LVIS category); `mixed` replaces the first of them by a view of 96 154 images (1.25 M rows, the
streaming form).  Per case and S in 2, 4, 8, 16, one JSON line with the host-to-host microseconds A SLOT of

  views_batch  DeviceIndex.views_topk_batch(views[:S], Q[:S], k)     the one call
  view_loop    [v.topk(q, k) for v, q in zip(views[:S], Q[:S])]      what S sessions on S views do today

each as median [interquartile range] over --reps rounds after one untimed round; both run in every round, in
alternating order.  `ahead`: the call's median is below the loop's by more than both interquartile ranges.
`scan_us_per_slot`: the call's scan launches alone, between events on the parent's stream, from a pass of their own
(the events cost host time, so that pass is not the one timed above); the rest of a slot is selections and the wait.
`identical`: both returned the same images, score bits and rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOTS = (2, 4, 8, 16)


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2]) and
               np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def case(tag, parent, views, args):
    from seesaw_amd.device_index import DeviceIndex
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((max(SLOTS), parent.dim)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    paths = {"views_batch": lambda s: DeviceIndex.views_topk_batch(views[:s], Q[:s], args.k),
             "view_loop": lambda s: [v.topk(q, args.k) for v, q in zip(views[:s], Q[:s])]}
    names = list(paths)
    for s in SLOTS:
        us = {name: [] for name in names}
        identical = True
        for rep in range(args.reps + 1):
            got = {}
            for i in range(len(names)):
                name = names[(i + rep) % len(names)]
                t0 = time.perf_counter()
                got[name] = paths[name](s)
                t = 1e6 * (time.perf_counter() - t0) / s
                if rep:
                    us[name].append(t)
            identical = identical and same(got["views_batch"], got["view_loop"])
        parent.profile(True)
        for _ in range(args.reps):
            paths["views_batch"](s)
        scan_ms = parent.profile_read()
        parent.profile(False)
        out = {"case": tag, "parent_rows": parent.n_rows, "view_rows": [int(v.n_rows) for v in views[:2]], "dim": parent.dim,
               "dtype": parent.dtype.name, "k": args.k, "slots": s, "reps": args.reps, "chunk_select": bool(parent.chunk_select)}
        stat = {}
        for name in names:
            q1, med, q3 = np.percentile(us[name], [25, 50, 75])
            stat[name] = (med, q3 - q1)
            out[name + "_us_per_slot"] = round(float(med), 2)
            out[name + "_iqr"] = round(float(q3 - q1), 2)
        out["scan_us_per_slot"] = round(float(np.median(scan_ms)) * 1e3 / s, 2)
        out["ahead"] = bool(stat["view_loop"][0] - stat["views_batch"][0] > max(stat["view_loop"][1], stat["views_batch"][1]))
        out["identical"] = bool(identical)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float16"])
    ap.add_argument("--chunk-select", action="store_true",
                    help="the parent's chunk selection on (DeviceIndex.chunk_select): the call selects its slots together")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_views_batch: no GPU (timings are not taken on a CPU)")
    from seesaw_amd.device_index import DeviceIndex
    n_images, tiles = 120_000, 13
    for name in args.dtypes:
        parent = DeviceIndex.synthetic(n_images * tiles, 512, seed=4, dtype=np.dtype(name))
        parent.set_row2image(np.repeat(np.arange(n_images), tiles).astype(np.int32))
        parent.chunk_select = args.chunk_select
        rng = np.random.default_rng(11)
        small = [parent.view(np.sort(rng.choice(n_images, 1109, replace=False))) for _ in range(max(SLOTS))]
        large = parent.view(np.sort(rng.choice(n_images, 96_154, replace=False)))
        try:
            case("category_%s" % name, parent, small, args)
            case("mixed_%s" % name, parent, [large] + small[1:], args)
        finally:
            for v in small + [large]:
                v.close()
            parent.close()


if __name__ == "__main__":
    main()
