#!/usr/bin/env python3
"""The batched top-k of a subset view (DeviceIndex.view_topk_batch; csrc/scan.hip: view_batch_kernel) against the path
it replaces and against its yardstick, in one process on one GPU ("Batched scan of a view").

    python tools/perf_view_batch.py [--reps 21] [--k 100] [--skip-large]

Views of every tenth image of a parent at dim 512, f32 and f16 rows: 16 384 images x 8 tiles = 2^17 rows of a 1.31 M-row
parent, and 96 154 images x 13 tiles = 1.25 M rows of a 12.5 M-row parent (the large case of tools/perf_subset_view.py).
Per case and nq in 2, 4, 8, 16, one JSON line with the host-to-host ms A QUERY of

  view_batch   view.view_topk_batch(Q[:nq], k)                  the new path
  view_loop    [view.topk(q, k) for q in Q[:nq]]                what query_batch on a view index did before
  copy_batch   copy.topk_batch(Q[:nq], k)                       the copied subset of the same members: the yardstick

each as median [interquartile range] over --reps rounds after one untimed round; the three run in every round, in an
order that rotates from round to round.  `identical`: the three returned the same images, score bits and rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NQS = (2, 4, 8, 16)


def gather_host(parent, rows, chunk=1 << 17):
    out = np.empty((rows.shape[0], parent.dim), dtype=np.float32)
    for r0 in range(0, rows.shape[0], chunk):
        out[r0:r0 + chunk] = parent.gather_rows(rows[r0:r0 + chunk])
    return out


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2]) and
               np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def case(tag, n_images, tiles, dtype, args):
    from seesaw_amd.device_index import DeviceIndex, view_rows
    dim = 512
    n = n_images * tiles
    parent = DeviceIndex.synthetic(n, dim, seed=4, dtype=dtype)
    parent.set_row2image(np.repeat(np.arange(n_images), tiles).astype(np.int32))
    members = np.arange(0, n_images, 10, dtype=np.int64)
    rows, _ = view_rows(np.arange(n_images + 1, dtype=np.int64) * tiles, members)
    compact = np.repeat(np.arange(members.shape[0]), tiles).astype(np.int32)
    view = parent.view(members)
    copy = DeviceIndex.from_numpy(gather_host(parent, rows), row2image=compact, dtype=dtype)  # (f16: rounds to the same bits)
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((max(NQS), dim)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    paths = {"view_batch": lambda nq: view.view_topk_batch(Q[:nq], args.k),
             "view_loop": lambda nq: [view.topk(q, args.k) for q in Q[:nq]],
             "copy_batch": lambda nq: copy.topk_batch(Q[:nq], args.k)}
    names = list(paths)
    try:
        for nq in NQS:
            ms = {name: [] for name in names}
            identical = True
            for rep in range(args.reps + 1):
                got = {}
                for i in range(len(names)):
                    name = names[(i + rep) % len(names)]
                    t0 = time.perf_counter()
                    got[name] = paths[name](nq)
                    t = 1e3 * (time.perf_counter() - t0) / nq
                    if rep:
                        ms[name].append(t)
                identical = identical and same(got["view_batch"], got["view_loop"]) and same(got["view_batch"], got["copy_batch"])
            out = {"case": tag, "parent_rows": n, "view_rows": int(rows.shape[0]), "view_images": int(members.shape[0]),
                   "dim": dim, "dtype": np.dtype(dtype).name, "k": args.k, "nq": nq, "reps": args.reps}
            for name in names:
                q1, med, q3 = np.percentile(ms[name], [25, 50, 75])
                out[name + "_ms_per_query"] = round(float(med), 4)
                out[name + "_iqr"] = round(float(q3 - q1), 4)
            out["batch_over_loop"] = round(out["view_batch_ms_per_query"] / out["view_loop_ms_per_query"], 3)
            out["batch_over_copy"] = round(out["view_batch_ms_per_query"] / out["copy_batch_ms_per_query"], 3)
            out["identical"] = bool(identical)
            print(json.dumps(out), flush=True)
    finally:
        view.close()
        copy.close()
        parent.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_view_batch: no GPU (timings are not taken on a CPU)")
    for dtype in (np.float32, np.float16):
        case("2^17_%s" % np.dtype(dtype).name, 163_840, 8, dtype, args)
    if not args.skip_large:
        for dtype in (np.float32, np.float16):
            case("1.25M_%s" % np.dtype(dtype).name, 12_500_000 // 13, 13, dtype, args)


if __name__ == "__main__":
    main()
