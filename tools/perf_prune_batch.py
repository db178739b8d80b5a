#!/usr/bin/env python3
"""The pruned batch -- on the int8 shadow, on the packed 6-bit shadow, or both in turn -- against the plain batch and
against pruned single calls, in one process (csrc/prune.hip k_q8_bounds_mq / k_q6_bounds_mq, DESIGN.md section 4,
"Pruned batch" and "Pruned batch on the 6-bit shadow").

    python tools/perf_prune_batch.py [--rows 4194304 ... 100e6] [--nq 2 4 8 16 64] [--k 100] [--reps 7]
                                     [--dtype float32|float16] [--warmup-rounds 2] [--shadow int8|six|both]
                                     [--tiles T] [--blocks B] [--tiles6 T] [--blocks6 B] [--dim 512]

For each index size: a synthetic N x 512 index, one first pruned call per form (builds its shadow), then per nq
`warmup-rounds` untimed rounds and `reps` timed rounds; a round runs the variants in turn on the same handle with fresh
queries -- topk_batch(prune=True) on each shadow asked for (ssw_tune_prune6 switches between them as tools/perf_prune.py
does: with `both`, the two shadows are resident side by side), topk_batch (plain), nq pruned single topk calls (on the
last form's shadow).  The lab build lowers the thresholds to 1 row so that every size is pruned (ssw_tune_prune,
ssw_tune_prune6, ssw_tune_prune6_batch).  Prints one JSON line per (size, nq): host wall ms PER QUERY of each variant (median, min, max and
the max - min spread), the HIP-event ms per chunk of each pruned batch's replacement of the scan, survivors per query,
fallbacks, whether all variants returned the same bits, and the shadow bytes resident; a form whose shadow was refused
for memory ran the plain batch and is reported as `"resident": false`.

--dim D (default 512): the width of the index.  --dim 768 (how MIN_ROWS (6-bit batch, dim 768, f32 and f16) are chosen): that
dim has the 6-bit shadow alone, so --shadow is taken as `six` whatever was given, the comparison is the 6-bit batch
against the plain batch and the pruned singles, there is no int8 column, and the
JSON line carries "dim".  Every other dim prints what it printed before the option existed."""
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
    ap.add_argument("--rows", type=float, nargs="+", default=[1 << 22, 1 << 23, 12.5e6, 1 << 24, 25e6, 50e6, 100e6])
    ap.add_argument("--nq", type=int, nargs="+", default=[2, 4, 8, 16, 64])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--warmup-rounds", type=int, default=2)
    ap.add_argument("--shadow", choices=("int8", "six", "both"), default="both")
    ap.add_argument("--tiles", type=int, default=-1)
    ap.add_argument("--blocks", type=int, default=-1)
    ap.add_argument("--tiles6", type=int, default=-1)
    ap.add_argument("--blocks6", type=int, default=-1)
    ap.add_argument("--dim", type=int, choices=(256, 512, 768, 1024), default=512)
    args = ap.parse_args()
    dim = args.dim
    if dim == 768:
        args.shadow = "six"
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    forms = {"int8": ["int8"], "six": ["six"], "both": ["int8", "six"]}[args.shadow]

    def stats(idx):
        out = np.zeros(6, dtype=np.int64)
        _lib.call("ssw_index_prune_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return out

    def use(form):  # the shadow the next pruned call scans, single or batch
        _lib.call("ssw_tune_prune6", 1 if form == "six" else 0, 1)

    def queries(seed, nq):
        Q = np.random.default_rng(10_000 + seed).standard_normal((nq, dim)).astype(np.float32)
        return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)

    def same(a, b):
        return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
                   for ra, rb in zip(a, b) for x, y in zip(ra, rb))

    def summary(v):
        return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3),
                round(float(np.max(v) - np.min(v)), 3)]

    with _lib.debug_hooks():
        _lib.call("ssw_tune_prune_scan_mq", args.blocks, args.tiles)
        _lib.call("ssw_tune_prune6_scan_mq", args.blocks6, args.tiles6)
        for rows in args.rows:
            n = int(rows)
            idx = DeviceIndex.synthetic(n, dim, seed=2024, dtype=np.dtype(args.dtype))
            try:
                _lib.call("ssw_tune_prune", 1, 1, -1)
                _lib.call("ssw_tune_prune6_batch", 1)
                resident, bytes_before = {}, 0
                for form in forms:  # the first pruned call of each form builds its shadow, if it fits
                    use(form)
                    idx.topk_batch(queries(0, 2), args.k, prune=True)
                    now = int(stats(idx)[5])
                    resident[form] = now > bytes_before
                    bytes_before = now
                seed = 1
                for nq in args.nq:
                    names = ["pruned_batch_" + f for f in forms] + ["plain_batch", "pruned_singles"]
                    wall = {name: [] for name in names}
                    ev = {f: [] for f in forms}
                    surv = {f: [] for f in forms}
                    identical = True
                    st0 = stats(idx)
                    for r in range(-args.warmup_rounds, args.reps):
                        Q = queries(seed, nq)
                        seed += 1
                        out, dt, chunk_ms, last = {}, {}, {}, {}
                        for form in forms:
                            use(form)
                            idx.profile(True)
                            t0 = time.perf_counter()
                            out["pruned_batch_" + form] = idx.topk_batch(Q, args.k, prune=True)
                            dt["pruned_batch_" + form] = time.perf_counter() - t0
                            chunk_ms[form] = idx.profile_read().tolist()
                            idx.profile(False)
                            last[form] = int(stats(idx)[2])
                        t2 = time.perf_counter()
                        out["plain_batch"] = idx.topk_batch(Q, args.k)
                        t3 = time.perf_counter()
                        out["pruned_singles"] = [idx.topk(q, args.k) for q in Q]
                        t4 = time.perf_counter()
                        dt["plain_batch"], dt["pruned_singles"] = t3 - t2, t4 - t3
                        if r < 0:
                            continue
                        for name in names:
                            wall[name].append(1e3 * dt[name] / nq)
                            identical = identical and same(out[name], out["plain_batch"])
                        for form in forms:
                            ev[form].extend(chunk_ms[form])
                            surv[form].append(last[form])
                    st = stats(idx)
                    res = {"rows": n, "dtype": args.dtype, "k": args.k, "nq": nq, "shadow": args.shadow,
                           "resident": resident, "shadow_bytes": int(st[5])}
                    if dim != 512:
                        res = {"dim": dim, **res}
                    for name, v in wall.items():
                        res[name + "_ms_per_query"] = summary(v)
                    for form in forms:
                        res["pruned_batch_" + form + "_chunk_event_ms_median"] = \
                            round(float(np.median(ev[form])), 3) if ev[form] else None
                        res["last_query_survivors_" + form] = surv[form]
                    res.update({"pruned_queries": int(st[3] - st0[3]), "fallbacks": int(st[4] - st0[4]),
                                "identical": bool(identical)})
                    print(json.dumps(res), flush=True)
            finally:
                _lib.call("ssw_tune_prune", 1, -1, -1)
                _lib.call("ssw_tune_prune6", 1, -1)
                _lib.call("ssw_tune_prune6_batch", -1)
                idx.close()
        _lib.call("ssw_tune_prune_scan_mq", -1, -1)
        _lib.call("ssw_tune_prune6_scan_mq", -1, -1)


if __name__ == "__main__":
    main()
