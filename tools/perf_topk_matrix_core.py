#!/usr/bin/env python3
"""Large-batch top-k on the matrix cores against the two existing batches, in one process (csrc/index_mc.hip; DESIGN.md
section 4, "Large-batch top-k on the matrix cores").

    python tools/perf_topk_matrix_core.py [--rows 1.56e6 12.5e6 100e6] [--nq 16 64 256 1024] [--k 100] [--reps 5]
                                          [--dtype float32 float16] [--dim 512] [--step-limit 120] [--out FILE]

For each dtype and index size: a synthetic N x dim index (DeviceIndex.synthetic), one untimed call of each variant (the
pruned one builds its shadow there), then per nq `reps` timed rounds; a round runs topk_batch(matrix_core=True),
topk_batch() and topk_batch(prune=True) in turn on the same handle with fresh unit queries.  Each call ends in the
library's own device waits, so the host clock around it is the call's time.  Every GPU step runs under --step-limit
seconds (SIGALRM): a step that exceeds it ends the tool with status 124 and nothing more is started.
Prints, and with --out appends to FILE, one line per (dtype, size, nq): ms PER QUERY of each variant as median
[quartile 1, quartile 3], the share of queries the new path sent to the plain batch, and the new path's arithmetic and
row-byte rates over the WHOLE CALL (2 n nq dim flop, n dim bytes-per-element a group of 1024 queries: the candidate
kernel's own rates are at least these), and whether the three variants returned the same bits in the last round."""
import argparse
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, nargs="+", default=[1.56e6, 12.5e6, 100e6])
    ap.add_argument("--nq", type=int, nargs="+", default=[16, 64, 256, 1024])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", nargs="+", choices=("float32", "float16"), default=["float32", "float16"])
    ap.add_argument("--dim", type=int, choices=(256, 512, 768, 1024), default=512)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from seesaw_amd.device_index import DeviceIndex

    def on_alarm(signum, frame):
        print("a GPU step exceeded its time limit; nothing more is started", flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, on_alarm)

    def step(f):
        signal.alarm(args.step_limit)
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        signal.alarm(0)
        return r, dt

    def queries(seed, nq):
        Q = np.random.default_rng(10_000 + seed).standard_normal((nq, args.dim)).astype(np.float32)
        return np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)

    def same(a, b):
        return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
                   for ra, rb in zip(a, b) for x, y in zip(ra, rb))

    def quart(v, nq):
        q1, med, q3 = np.percentile(np.asarray(v) * 1e3 / nq, [25, 50, 75])
        return f"{med:9.4f} [{q1:9.4f}, {q3:9.4f}]"

    variants = (("matrix_core", dict(matrix_core=True)), ("plain", dict()), ("pruned", dict(prune=True)))
    lines = [f"# dim {args.dim}, k {args.k}, {args.reps} rounds; ms a query: median [q1, q3]",
             f"# {'dtype':8s} {'rows':>10s} {'nq':>5s}  {'matrix_core':>31s}  {'plain':>31s}  {'pruned':>31s}  "
             f"{'fallback':>8s} {'TFLOP/s':>8s} {'TB/s':>6s} same"]
    print("\n".join(lines), flush=True)
    for dtype in args.dtype:
        for rows in args.rows:
            n = int(rows)
            idx, _ = step(lambda: DeviceIndex.synthetic(n, args.dim, seed=2024, dtype=np.dtype(dtype)))
            for _, kw in variants:  # untimed: workspaces, the shadow, code objects
                step(lambda: idx.topk_batch(queries(0, 16), args.k, **kw))
            for nq in args.nq:
                t = {name: [] for name, _ in variants}
                before = idx.matrix_core_stats()
                for r in range(args.reps):
                    Q = queries(1 + r, nq)
                    res = {}
                    for name, kw in variants:
                        res[name], dt = step(lambda: idx.topk_batch(Q, args.k, **kw))
                        t[name].append(dt)
                after = idx.matrix_core_stats()
                sent = after["uncertified"] + after["overflowed"] - before["uncertified"] - before["overflowed"]
                med = float(np.median(t["matrix_core"]))
                groups = -(-nq // 1024)
                line = (f"  {dtype:8s} {n:10d} {nq:5d}  {quart(t['matrix_core'], nq)}  {quart(t['plain'], nq)}  "
                        f"{quart(t['pruned'], nq)}  {sent / (args.reps * nq):8.4f} "
                        f"{2.0 * n * nq * args.dim / med / 1e12:8.1f} "
                        f"{groups * n * args.dim * np.dtype(dtype).itemsize / med / 1e12:6.2f} "
                        f"{same(res['matrix_core'], res['plain']) and same(res['plain'], res['pruned'])}")
                print(line, flush=True)
                lines.append(line)
            idx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
