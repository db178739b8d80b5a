#!/usr/bin/env python3
"""Pruned against full-scan top-k in one process (csrc/prune.hip).

    python tools/perf_prune.py [--rows 12.5e6 25e6 50e6 100e6] [--k 100] [--reps 10] [--dtype float32|float16]
                               [--warmup-pairs 2]
    python tools/perf_prune.py --three-way [--rows ...] [--k 100] [--dtype float32|float16]
    python tools/perf_prune.py --dim 768 [--rows ...] [--k 100] [--dtype float32|float16]
    python tools/perf_prune.py --two-stage [--rows ...] [--k 100] [--dim 512|1024] [--scan41 BLOCKS TILES]

For each index size: a synthetic N x 512 index of f32 or binary16 rows, one first top-k (builds the int8 shadow, timed
on its own), `warmup-pairs` untimed pairs, then `reps` pairs of top-k calls with the pruning switched off and on in turn
(the lab build's ssw_tune_prune; the threshold is lowered to 1 row so that every size is pruned), each a different
query.  Prints per size: host wall ms per call (median, and the spread min .. max), the HIP-event ms of the scan phase
(the full scan, or shadow scan + threshold selection + survivors + rescoring), survivors and fallbacks, and whether
both forms returned the same images, scores and best rows.  This mode keeps every index on the int8 shadow at every size
(ssw_tune_prune6(0)).

--three-way (how MIN_ROWS (6-bit single call, f32), MIN_ROWS_Q5 and, with --dtype float16, MIN_ROWS (6-bit single call, f16) of
csrc/index_prune.hip are chosen):
full scan / int8 shadow / packed 6-bit shadow and, on f32 rows of dim 512 or 1024, a fourth column, the packed 5-bit
shadow with its exact threshold, in turn in one process, two warm-up rounds, then 20 rounds, each a
different query; per size one JSON line with the median and the spread (max - min) of the host wall ms of each form, the
6-bit and the 5-bit survivors, whether all forms returned the same bytes, and under "shadows" which shadow each form's first call
built, from the growth of prune_stats' shadow_bytes ("none", "int8", "6-bit" or "5-bit"; a form that built another shadow than
its name says ends the run).  Where the shadows do not fit beside the rows together, the int8 rounds and the 6-bit (and
5-bit) rounds run one after the other on two indexes of the same rows, each alternating with the full scan; the 6-bit and
the 5-bit call always alternate on one index.

--two-stage (how MIN_ROWS_Q41 of csrc/index_prune.hip is chosen; f32 rows of dim 512 or 1024): full scan / packed 5-bit
shadow / two-stage 4 + 1-bit shadow in turn on one index, the rounds and the JSON line of --three-way with the columns
"q5" and "q41", and beside them the first stage's survivors of the two-stage calls (min, median, max) and the dense
refines.  --scan41 sets k_q4_bounds' launch shape (four-wave blocks a CU, 16-row tiles a request) for the run and the
line carries it.

--dim D (default 512): the width of the index.  --dim 768 (how MIN_ROWS (6-bit single call, dim 768, f32) and MIN_ROWS (6-bit single call, dim 768, f16) are
chosen): that dim has the 6-bit shadow alone, so the run is always the rounds of --three-way with two forms, full scan /
packed 6-bit shadow, and the JSON line has no int8 column; it carries "dim".  Every other dim prints what it printed
before the option existed."""
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
    ap.add_argument("--rows", type=float, nargs="+", default=[12.5e6, 25e6, 50e6, 100e6])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--warmup-pairs", type=int, default=2)
    ap.add_argument("--three-way", action="store_true")
    ap.add_argument("--dim", type=int, choices=(256, 512, 768, 1024), default=512)
    ap.add_argument("--two-stage", action="store_true")
    ap.add_argument("--scan41", type=int, nargs=2, metavar=("BLOCKS", "TILES"))
    args = ap.parse_args()
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    dim = args.dim

    def stats(idx):
        out = np.zeros(6, dtype=np.int64)
        _lib.call("ssw_index_prune_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return out

    def query(i):
        q = np.random.default_rng(10_000 + i).standard_normal(dim).astype(np.float32)
        return (q / np.linalg.norm(q)).astype(np.float32)

    def set_form(form):
        _lib.call("ssw_tune_prune", 0 if form == "full" else 1, 1, -1)
        _lib.call("ssw_tune_prune6", 1 if form == "q6" else 0, 1)
        _lib.call("ssw_tune_prune5", 1 if form == "q5" else 0, 1)
        _lib.call("ssw_tune_prune41", 1 if form == "q41" else 0, 1, -1)

    dtype = np.dtype(args.dtype)
    six_only = dim == 768  # no int8 shadow at this dim
    five = dim in (512, 1024) and dtype == np.float32  # the fourth column
    built_by = {"full": "none", "int8": "int8", "q6": "6-bit", "q5": "5-bit", "q41": "two-stage"}
    coarse = []  # the first stage's survivors of the timed two-stage calls

    def coarse_stats(idx):
        out = np.zeros(3, dtype=np.int64)
        _lib.call("ssw_index_prune_coarse_stats", idx._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        return out

    def rounds(n, forms, wall, surv, shadows):
        """warm-up and timed rounds over `forms` on a fresh index; -> all forms returned the same bytes"""
        idx = DeviceIndex.synthetic(n, dim, seed=2024, dtype=dtype)
        grows = {0: "none", n * (dim + 8): "int8", (n + 15) // 16 * 16 * (dim * 3 // 4 + 8): "6-bit",
                 (n + 15) // 16 * 16 * (dim * 5 // 8 + 8): "5-bit", (n + 15) // 16 * 16 * (dim * 5 // 8 + 16): "two-stage"}
        same = True
        try:
            for form in forms:  # builds the shadows, untimed
                set_form(form)
                before = idx.prune_stats()["shadow_bytes"]
                idx.topk(query(0), args.k)
                grew = idx.prune_stats()["shadow_bytes"] - before
                shadows[form] = grows.get(grew, f"{grew} bytes")
                if shadows[form] != built_by[form]:
                    raise SystemExit(f"{n} rows: the {form} form built {shadows[form]!r}, not {built_by[form]!r}")
            for i in range(-2, 20):
                q, out = query(3 + i), {}
                for form in forms:
                    set_form(form)
                    t0 = time.perf_counter()
                    out[form] = idx.topk(q, args.k)
                    if i >= 0:
                        wall.setdefault(form, []).append(1e3 * (time.perf_counter() - t0))
                        if form in ("q6", "q5", "q41"):
                            surv.setdefault(form, []).append(int(stats(idx)[2]))
                        if form == "q41":
                            coarse.append(int(coarse_stats(idx)[0]))
                for form in forms[1:]:
                    same = same and all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
                                        for a, b in zip(out[forms[0]], out[form]))
            if "q41" in forms:
                shadows["dense_refines"] = int(coarse_stats(idx)[1])
            return same, int(stats(idx)[4])
        finally:
            idx.close()

    def three_way(n):
        import torch
        total = torch.cuda.mem_get_info(0)[1]
        q5_bytes = dim * 5 // 8 + 8 if five else 0
        together = six_only or n * (dim * dtype.itemsize + (dim + 8) + (dim * 3 // 4 + 8) + q5_bytes + 8) + (5 << 30) < total
        wall, surv, shadows = {}, {}, {}
        packed = ["q6", "q5"] if five else ["q6"]
        if args.two_stage:
            same, fallbacks = rounds(n, ["full", "q5", "q41"], wall, surv, shadows)
        elif six_only:
            same, fallbacks = rounds(n, ["full", "q6"], wall, surv, shadows)
        elif together:
            same, fallbacks = rounds(n, ["full", "int8"] + packed, wall, surv, shadows)
        else:
            wall_b = {}
            same_a, fa = rounds(n, ["full", "int8"], wall, surv, shadows)
            same_b, fb = rounds(n, ["full"] + packed, wall_b, surv, shadows)
            wall["full_beside_q6"] = wall_b.pop("full")
            wall.update(wall_b)
            same, fallbacks = same_a and same_b, fa + fb
        res = {"rows": n, "dtype": args.dtype, "k": args.k, "one_index": bool(together), "shadows": shadows}
        if dim != 512:
            res = {"dim": dim, **res}
        for form, v in wall.items():
            res[form + "_ms_median"] = round(float(np.median(v)), 3)
            res[form + "_ms_spread"] = round(float(np.max(v) - np.min(v)), 3)
        for form, v in surv.items():
            res[form + "_survivors_min_median_max"] = [int(np.min(v)), int(np.median(v)), int(np.max(v))]
        if args.two_stage:
            res["q41_first_stage_min_median_max"] = [int(np.min(coarse)), int(np.median(coarse)), int(np.max(coarse))]
            res["dense_refines"] = shadows.pop("dense_refines")
            if args.scan41:
                res["scan41_blocks_tiles"] = list(args.scan41)
            coarse.clear()
        res.update({"fallbacks": fallbacks, "identical": bool(same)})
        print(json.dumps(res), flush=True)

    with _lib.debug_hooks():
        if args.two_stage and not five:
            raise SystemExit("--two-stage: f32 rows of dim 512 or 1024 only")
        if args.three_way or six_only or args.two_stage:
            try:
                if args.scan41:
                    _lib.call("ssw_tune_prune41_scan", args.scan41[0], args.scan41[1])
                for rows in args.rows:
                    three_way(int(rows))
            finally:
                _lib.call("ssw_tune_prune", 1, -1, -1)
                _lib.call("ssw_tune_prune6", 1, -1)
                _lib.call("ssw_tune_prune5", 1, -1)
                _lib.call("ssw_tune_prune41", 1, -1, -1)
                _lib.call("ssw_tune_prune41_scan", 0, 0)
            return
        _lib.call("ssw_tune_prune6", 0, -1)
        _lib.call("ssw_tune_prune5", 0, -1)
        _lib.call("ssw_tune_prune41", 0, -1, -1)
        for rows in args.rows:
            n = int(rows)
            idx = DeviceIndex.synthetic(n, dim, seed=2024, dtype=np.dtype(args.dtype))
            try:
                _lib.call("ssw_tune_prune", 1, 1, -1)
                t0 = time.perf_counter()
                idx.topk(query(0), args.k)
                first_ms = 1e3 * (time.perf_counter() - t0)
                res = {"rows": n, "dtype": args.dtype, "k": args.k, "first_call_ms_with_shadow_build": round(first_ms, 2),
                       "shadow_bytes": int(stats(idx)[5])}
                if dim != 512:
                    res = {"dim": dim, **res}
                wall = {0: [], 1: []}
                ev = {0: [], 1: []}
                surv, same = [], True
                for i in range(-args.warmup_pairs, args.reps):
                    q = query(1 + args.warmup_pairs + i)
                    out = {}
                    for on in (0, 1):
                        _lib.call("ssw_tune_prune", on, 1, -1)
                        if i < 0:
                            idx.topk(q, args.k)
                            continue
                        idx.profile(True)
                        t0 = time.perf_counter()
                        out[on] = idx.topk(q, args.k)
                        wall[on].append(1e3 * (time.perf_counter() - t0))
                        ev[on].extend(idx.profile_read().tolist())
                        idx.profile(False)
                        if on:
                            surv.append(int(stats(idx)[2]))
                    if i < 0:
                        continue
                    same = same and all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
                                        for a, b in zip(out[0], out[1]))
                st = stats(idx)
                res.update({
                    "full_ms_wall_median": round(float(np.median(wall[0])), 3),
                    "full_ms_wall_min_max": [round(float(np.min(wall[0])), 3), round(float(np.max(wall[0])), 3)],
                    "pruned_ms_wall_median": round(float(np.median(wall[1])), 3),
                    "pruned_ms_wall_min_max": [round(float(np.min(wall[1])), 3), round(float(np.max(wall[1])), 3)],
                    "full_scan_phase_ms_median": round(float(np.median(ev[0])), 3),
                    "pruned_scan_phase_ms_median": round(float(np.median(ev[1])), 3),
                    "survivors": surv, "pruned_calls": int(st[3]), "fallbacks": int(st[4]),
                    "identical": bool(same),
                })
                print(json.dumps(res), flush=True)
            finally:
                _lib.call("ssw_tune_prune", 1, -1, -1)
                idx.close()
        _lib.call("ssw_tune_prune6", 1, -1)
        _lib.call("ssw_tune_prune5", 1, -1)
        _lib.call("ssw_tune_prune41", 1, -1, -1)


if __name__ == "__main__":
    main()
