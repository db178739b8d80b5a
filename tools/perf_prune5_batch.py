#!/usr/bin/env python3
"""The pruned batch on the packed 5-bit shadow against the pruned batch on the 6-bit shadow, the plain batch and a loop of
pruned single calls, in one process on one handle (csrc/prune.hip k_q5_bounds_mq; DESIGN.md section 4, "Pruned batch on
the 5-bit shadow").

    python tools/perf_prune5_batch.py [--rows 25e6 50e6 100e6] [--nq 2 4 8 16] [--k 100] [--reps 9] [--warmup-rounds 2]
                                      [--dim 512] [--forms five six] [--reserve-gib 4]

For each size: a synthetic N x dim f32 index without an image map; the first pruned batch of each form builds its shadow
(with both forms the two shadows are resident side by side, if the reserve lets them: a form whose shadow was refused
reports `"resident": false` and its column is the form the batch fell to).  Per nq, `warmup-rounds` untimed and `reps`
timed rounds; a round runs the variants in turn with fresh queries: topk_batch(prune=True) on the 5-bit shadow, on the
6-bit shadow, topk_batch, and nq pruned single calls (5-bit).  The lab build picks the batch's shadow: ssw_tune_prune6
off sends a pruned batch to the 5-bit shadow, on to the 6-bit one the index holds; the row counts are lowered to one row
and the two-stage shadow of single queries is off.  One JSON line per (size, nq): host wall ms PER QUERY of each variant
as [median, q25, q75, q75 - q25], the last slot's survivors of each pruned batch, fallbacks, whether every variant
returned the plain batch's bits, and the shadow bytes held."""
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
    ap.add_argument("--rows", type=float, nargs="+", default=[25e6, 50e6, 100e6])
    ap.add_argument("--nq", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup-rounds", type=int, default=2)
    ap.add_argument("--dim", type=int, choices=(512, 1024), default=512)
    ap.add_argument("--forms", nargs="+", choices=("five", "six"), default=["five", "six"])
    ap.add_argument("--reserve-gib", type=float, default=4.0)
    args = ap.parse_args()
    dim = args.dim
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex

    def stats(idx):
        out = np.zeros(6, dtype=np.int64)
        _lib.call("ssw_index_prune_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return out

    def use(form):  # the shadow the next pruned batch scans; single queries stay on the 5-bit one
        _lib.call("ssw_tune_prune6", 1 if form == "six" else 0, 1)
        _lib.call("ssw_tune_prune5", 0 if form == "six" else 1, 1)

    def queries(seed, nq):
        Q = np.random.default_rng(10_000 + seed).standard_normal((nq, dim)).astype(np.float32)
        return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)

    def same(a, b):
        return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
                   for ra, rb in zip(a, b) for x, y in zip(ra, rb))

    def summary(v):
        q25, med, q75 = (float(x) for x in np.percentile(v, [25, 50, 75]))
        return [round(med, 3), round(q25, 3), round(q75, 3), round(q75 - q25, 3)]

    with _lib.debug_hooks():
        for rows in args.rows:
            n = int(rows)
            idx = DeviceIndex.synthetic(n, dim, seed=2024)
            try:
                _lib.call("ssw_tune_prune", 1, 1, int(args.reserve_gib * (1 << 30)))
                _lib.call("ssw_tune_prune6_batch", 1)
                _lib.call("ssw_tune_prune5_batch", 1)
                _lib.call("ssw_tune_prune41", 0, -1, -1)
                resident, held = {}, 0
                for form in args.forms:  # the first pruned batch of each form builds its shadow, if it fits
                    use(form)
                    idx.topk_batch(queries(0, 2), args.k, prune=True)
                    now = int(stats(idx)[5])
                    resident[form] = now > held
                    held = now
                seed = 1
                for nq in args.nq:
                    names = ["pruned_batch_" + f for f in args.forms] + ["plain_batch", "pruned_singles"]
                    wall = {name: [] for name in names}
                    surv = {f: [] for f in args.forms}
                    identical = True
                    st0 = stats(idx)
                    for r in range(-args.warmup_rounds, args.reps):
                        Q = queries(seed, nq)
                        seed += 1
                        out, dt, last = {}, {}, {}
                        for form in args.forms:
                            use(form)
                            t0 = time.perf_counter()
                            out["pruned_batch_" + form] = idx.topk_batch(Q, args.k, prune=True)
                            dt["pruned_batch_" + form] = time.perf_counter() - t0
                            last[form] = int(stats(idx)[2])
                        use("five")
                        t2 = time.perf_counter()
                        out["plain_batch"] = idx.topk_batch(Q, args.k)
                        t3 = time.perf_counter()
                        out["pruned_singles"] = [idx.topk(q, args.k) for q in Q]
                        dt["plain_batch"], dt["pruned_singles"] = t3 - t2, time.perf_counter() - t3
                        if r < 0:
                            continue
                        for name in names:
                            wall[name].append(1e3 * dt[name] / nq)
                            identical = identical and same(out[name], out["plain_batch"])
                        for form in args.forms:
                            surv[form].append(last[form])
                    st = stats(idx)
                    res = {"rows": n, "dim": dim, "k": args.k, "nq": nq, "resident": resident, "shadow_bytes": int(st[5])}
                    for name, v in wall.items():
                        res[name + "_ms_per_query"] = summary(v)
                    for form in args.forms:
                        res["last_slot_survivors_" + form] = surv[form]
                    res.update({"pruned_queries": int(st[3] - st0[3]), "fallbacks": int(st[4] - st0[4]),
                                "identical": bool(identical)})
                    print(json.dumps(res), flush=True)
            finally:
                _lib.call("ssw_tune_prune", 1, -1, -1)
                _lib.call("ssw_tune_prune6", 1, -1)
                _lib.call("ssw_tune_prune5", 1, -1)
                _lib.call("ssw_tune_prune6_batch", -1)
                _lib.call("ssw_tune_prune5_batch", -1)
                _lib.call("ssw_tune_prune41", 1, -1, -1)
                idx.close()


if __name__ == "__main__":
    main()
