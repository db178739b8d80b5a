#!/usr/bin/env python3
"""A zero-copy view of a resident index (DeviceIndex.view) against the copied subset index (from_numpy(X[rows]): what
`subset()` builds, the parent commit's only way), in one process on one GPU.

    python tools/perf_subset_view.py [--calls 2000] [--repeats 5] [--k 50] [--skip-large]

Cases: 1 109 images x 13 tiles (an LVIS-category subset, 14 417 rows) of a 120 000-image parent at dim 512, f32 and
f16 rows; every tenth image of a 12.5 M-row f32 parent (961 538 images x 13 tiles -> 1.25 M rows).  The member images
of the first case are drawn at random (sorted), so the view's rows lie in runs of one image's 13 tiles.

Per case, one JSON line:
  create_ms       view creation against from_numpy of the member rows that are already gathered on the host (the host
                  gather `vectors[mask]` that precedes it in subset() is reported apart, as gather_ms of the D2H gather
                  this tool uses to get the rows; neither is in copy create_ms) -- median of --create-repeats
  device_bytes    device memory taken by each after its first top-k: a difference of hipMemGetInfo, which moves in 2 MiB
                  steps and counts what the allocator had cached from the creations before -- the footprint a process
                  sees, not the sum of the handle's buffers; for an f16 copy it includes the 32 MiB upload staging
  alloc_bytes     the buffers a handle allocates at creation, computed from its shape: the rows (copy: rows x dim x 2 or 4
                  bytes) or the row table (view: 4 bytes a row), the score buffer (4 bytes a row + 256), the query
                  (4 dim) and the image map (8 bytes an image + 8).  The selection workspace and the staging blocks of
                  the first top-k come on top and are the same for both
  topk_us         host-to-host time of topk(q, k) per query: after 200 untimed calls each, --repeats alternating blocks
                  of --calls calls on the view and on the copy; the per-block medians, their median, and the copy's own
                  block-to-block spread (max - min of its block medians over their median)
  ratio           view / copy of the medians;  identical: the two return the same images, score bits and rows for 16
                  queries at this size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info(0)[0])


def gather_host(parent, rows, chunk=1 << 17):
    out = np.empty((rows.shape[0], parent.dim), dtype=np.float32)
    for r0 in range(0, rows.shape[0], chunk):
        out[r0:r0 + chunk] = parent.gather_rows(rows[r0:r0 + chunk])
    return out


def block(idx, Q, k, calls, first):
    us = np.empty(calls)
    for i in range(calls):
        q = Q[(first + i) % Q.shape[0]]
        t0 = time.perf_counter()
        idx.topk(q, k)
        us[i] = 1e6 * (time.perf_counter() - t0)
    return float(np.median(us)), float(np.percentile(us, 10)), float(np.percentile(us, 90))


def case(tag, n_images, tiles, dim, dtype, members, args, calls):
    from seesaw_amd.device_index import DeviceIndex, view_rows
    n = n_images * tiles
    parent = DeviceIndex.synthetic(n, dim, seed=4, dtype=dtype)
    parent.set_row2image(np.repeat(np.arange(n_images), tiles).astype(np.int32))
    rows, start = view_rows(np.arange(n_images + 1, dtype=np.int64) * tiles, members)
    compact = np.repeat(np.arange(members.shape[0]), tiles).astype(np.int32)
    t0 = time.perf_counter()
    X_sub = gather_host(parent, rows)  # (an f16 parent's rows come back widened: from_numpy rounds them to the same bits)
    gather_ms = 1e3 * (time.perf_counter() - t0)
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((64, dim)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    out = {"case": tag, "parent_rows": n, "view_rows": int(rows.shape[0]), "view_images": int(members.shape[0]), "dim": dim,
           "dtype": np.dtype(dtype).name, "k": args.k, "calls": calls, "repeats": args.repeats, "gather_ms": round(gather_ms, 2)}
    make = {"view": lambda: parent.view(members),
            "copy": lambda: DeviceIndex.from_numpy(X_sub, row2image=compact, dtype=dtype)}
    create, mem, live = {}, {}, {}
    for name in ("view", "copy"):
        ms = []
        for _ in range(args.create_repeats):  # (the first creation also warms the allocator)
            t0 = time.perf_counter()
            d = make[name]()
            d.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
            d.close()
        create[name] = round(float(np.median(ms)), 3)
        before = free_bytes()
        live[name] = make[name]()
        live[name].topk(Q[0], args.k)
        mem[name] = before - free_bytes()
    out["create_ms"], out["device_bytes"] = create, mem
    shared = (rows.shape[0] + 64) * 4 + dim * 4 + (members.shape[0] + 1) * 8
    out["alloc_bytes"] = {"view": int(rows.shape[0] * 4 + shared),
                          "copy": int(rows.shape[0] * dim * np.dtype(dtype).itemsize + shared)}
    v, c = live["view"], live["copy"]
    try:
        same = True
        for i in range(16):
            a, b = v.topk(Q[i], args.k), c.topk(Q[i], args.k)
            same = same and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and \
                np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        out["identical"] = bool(same)
        for d in (v, c):
            for i in range(200):
                d.topk(Q[i % 64], args.k)
        meds = {"view": [], "copy": []}
        for r in range(args.repeats):
            for name, d in (("view", v), ("copy", c)) if r % 2 == 0 else (("copy", c), ("view", v)):
                meds[name].append(block(d, Q, args.k, calls, r * calls))
        topk = {}
        for name in ("view", "copy"):
            m = np.array([x[0] for x in meds[name]])
            topk[name] = {"block_medians": [round(x, 2) for x in m.tolist()], "median": round(float(np.median(m)), 2),
                          "p10": round(float(np.median([x[1] for x in meds[name]])), 2),
                          "p90": round(float(np.median([x[2] for x in meds[name]])), 2),
                          "spread": round(float((m.max() - m.min()) / np.median(m)), 4)}
        out["topk_us"] = topk
        out["ratio"] = round(topk["view"]["median"] / topk["copy"]["median"], 4)
    finally:
        v.close()
        c.close()
        parent.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--create-repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_subset_view: no GPU (timings are not taken on a CPU)")
    rng = np.random.default_rng(11)
    lvis = np.sort(rng.choice(120_000, 1109, replace=False)).astype(np.int64)
    case("lvis_f32", 120_000, 13, 512, np.float32, lvis, args, args.calls)
    case("lvis_f16", 120_000, 13, 512, np.float16, lvis, args, args.calls)
    if not args.skip_large:
        n_images = 12_500_000 // 13
        case("tenth_of_12.5M_f32", n_images, 13, 512, np.float32, np.arange(0, n_images, 10, dtype=np.int64), args,
             max(50, args.calls // 10))


if __name__ == "__main__":
    main()
