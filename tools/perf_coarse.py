#!/usr/bin/env python3
"""The coarse index's rows out of a resident multiscale index (ssw_index_coarse_mean, csrc/coarse.hip) against the host
expression of the reference (mask, per-image f32 mean, normalise) on rows that are already in host memory, in one
process on one GPU.

    python tools/perf_coarse.py [--calls 20] [--host-max-gb 8] [--skip-large] [--out profiles/coarse_mean_ab.txt]

Shapes: 120 000 images x 13 tiles (1.56 M rows) and 961 538 images x 13 tiles (12.5 M rows) at dim 512, f32 and f16 rows,
one kept row in thirteen (the tile at the image's max_zoom_level: the last of its thirteen).

Per case, one JSON line:
  call_ms        host-to-host time of ssw_index_coarse_mean into an existing destination index (staging of the mask and
                 the positions, the kernel, the wait): one untimed call, then the median of --calls, with min and max
  kernel_ms      the kernel alone, from the event pair ssw_index_profile records around it, same calls
  bytes          the bytes the algorithm needs: kept rows x row bytes + n mask bytes read + m x dim x 4 written
  kernel_GBps    bytes / kernel_ms, and its share of the 8 TB/s HBM peak (the kernel is bound by HBM, not by arithmetic)
  pcie_bytes     what crosses PCIe: device path = n mask bytes + 8 m up and m x dim x 4 down once (from_fine_grained);
                 host path = 0 when the rows are in host memory and the result stays there, m x dim x 4 up to make the
                 result resident, and n x row bytes down first when the rows are only on the device
  host_ms        the host expression on the rows in host memory (numpy, one thread of this process): median of 3; the
                 rows are downloaded once for it (an f16 index's rows widened to f32), `null` where they exceed
                 --host-max-gb
  max_abs_diff   device result against the host expression (f32 against float64-accumulated f32: a few 1e-8)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
TILES = 13


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_expression(X, keep, tiles):
    """infer_coarse_embedding on host rows: every image has `tiles` rows"""
    lev1 = X[keep != 0]                                     # the mask (a copy of the kept rows)
    kept_per_image = int(keep[:tiles].sum())
    res = lev1.reshape(-1, kept_per_image, X.shape[1]).mean(axis=1, dtype=np.float32)
    return res / np.maximum(np.linalg.norm(res, axis=1, keepdims=True), np.float32(1e-6))


def download_chunked(idx, chunk=1 << 18):
    out = np.empty((idx.n_rows, idx.dim), dtype=np.float32)
    for r0 in range(0, idx.n_rows, chunk):
        n = min(chunk, idx.n_rows - r0)
        out[r0:r0 + n] = idx.download(r0, n)
    return out


def case(n_images, dim, dtype, args):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    n = n_images * TILES
    elem = np.dtype(dtype).itemsize
    src = DeviceIndex.synthetic(n, dim, seed=4, dtype=dtype)
    src.set_row2image(np.repeat(np.arange(n_images, dtype=np.int32), TILES))
    keep = np.zeros(n, dtype=np.uint8)
    keep[TILES - 1::TILES] = 1
    images = np.arange(n_images, dtype=np.int64)
    dst = DeviceIndex(n_images, dim)
    out = {"images": n_images, "rows": n, "dim": dim, "dtype": np.dtype(dtype).name, "kept_rows": int(keep.sum()),
           "calls": args.calls}

    def call():
        _lib.call("ssw_index_coarse_mean", src._h, _p(keep), _p(images), n_images, dst._h)

    call()  # warm-up: the code object, the allocator
    src.profile(True)
    ms = np.empty(args.calls)
    for i in range(args.calls):
        t0 = time.perf_counter()
        call()
        ms[i] = 1e3 * (time.perf_counter() - t0)
    kernel = src.profile_read()
    src.profile(False)
    assert kernel.shape[0] == args.calls, kernel.shape
    algo = int(keep.sum()) * dim * elem + n + n_images * dim * 4
    k_med = float(np.median(kernel))
    out.update(call_ms={"median": round(float(np.median(ms)), 3), "min": round(float(ms.min()), 3), "max": round(float(ms.max()), 3)},
               kernel_ms={"median": round(k_med, 4), "min": round(float(kernel.min()), 4), "max": round(float(kernel.max()), 4)},
               bytes=algo, kernel_GBps=round(algo / (k_med * 1e-3) / 1e9, 1),
               share_of_hbm_peak=round(algo / (k_med * 1e-3) / HBM_PEAK, 3),
               pcie_bytes={"device_path_up": n + 8 * n_images, "device_path_down": n_images * dim * 4,
                           "host_path_rows_on_host": 0, "host_path_result_up": n_images * dim * 4,
                           "host_path_rows_down_first": n * dim * elem})
    result = dst.download()
    if n * dim * 4 <= args.host_max_gb * 1e9:
        X = download_chunked(src)
        host_expression(X[:TILES * 64], keep[:TILES * 64], TILES)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = host_expression(X, keep, TILES)
            hs.append(1e3 * (time.perf_counter() - t0))
        out["host_ms"] = round(float(np.median(hs)), 1)
        out["host_over_call"] = round(out["host_ms"] / out["call_ms"]["median"], 1)
        out["max_abs_diff"] = float(np.abs(result - ref).max())
        del X
    else:
        out["host_ms"] = None
    dst.close()
    src.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-max-gb", type=float, default=8.0)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("perf_coarse.py measures on a GPU and found none")
    lines = []
    for n_images in (120_000,) + (() if args.skip_large else (961_538,)):
        for dtype in (np.float32, np.float16):
            line = json.dumps(case(n_images, 512, dtype, args))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/perf_coarse.py --calls %d --host-max-gb %g%s\n" % (args.calls, args.host_max_gb,
                                                                             " --skip-large" if args.skip_large else ""))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
