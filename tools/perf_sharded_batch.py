#!/usr/bin/env python3
"""The batched sharded top-k against the loop of single sharded queries, in one process ("Sharded
batch"; ssw_index_topk_batch_dev, ssw_topk_merge_msgs_batch_dev).

    python tools/perf_sharded_batch.py [--rows 12.5e6] [--dtype float32] [--k 100] [--reps 9] [--prune] [--out FILE]

World 1 with `force_collective` over RCCL: one rank's share of the 8-GPU configuration (12.5 M x 512 rows), with the
all-gather really issued.  One row format per invocation (run each under its own `timeout`, chained with `&&`).  For
nq = 2 / 4 / 8 / 16, k = 100:

  A  `ShardedSyntheticIndex.topk_batch_async(Q[:nq], k)` + one synchronisation: one scan launch per chunk, nq
     selections, ONE all-gather, ONE merge launch;
  B  nq x `topk_async(q, k)` + one synchronisation: nq scans, selections, all-gathers and merges -- the only way to do
     this without the batched path, as the product runs it: on an index the single query prunes (own rows, >= 2^22
     of them) every topk_async is the certified pre-scan with its host wait inside, while A always scans in full.

  C  (--prune) `topk_batch_async(Q[:nq], k, prune=True)` + one synchronisation: ONE pass over the int8 shadow per
     chunk, nq threshold selections and survivor lists, ONE rescoring launch sized by the device, nq selections, ONE
     all-gather, ONE merge launch, no host wait inside (ssw_index_topk_batch_dev_pruned).

A, B (and C) alternate after two warm-up rounds; one JSON line per nq with the median, the minimum, the quartiles and
the max - min spread of the wall ms per query of every form, the ratios of the medians, and whether all returned the
same keys; with --prune also the survivors and the failure bits of the last pruned chunk, read back from the device
(ssw_index_prune_batch_dev_read), and whether C is ahead of A and of B by more than the two spreads together.  The raw
lines are appended to --out (profiles/sharded_batch_ab.txt; with --prune profiles/sharded_batch_pruned_ab.txt)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NQS = (2, 4, 8, 16)


def spread(ms):
    a = np.sort(np.asarray(ms))
    return {"median": float(np.median(a)), "min": float(a[0]), "q1": float(np.percentile(a, 25)),
            "q3": float(np.percentile(a, 75)), "max": float(a[-1]), "spread": float(a[-1] - a[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=12.5e6)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float16"])
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--prune", action="store_true", help="a third column: the pruned batch (topk_batch_async(prune=True))")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sharded_batch_pruned_ab.txt" if args.prune else "sharded_batch_ab.txt")
    import torch
    import torch.distributed as dist
    from seesaw_amd.sharded import ShardedSyntheticIndex

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    n = int(args.rows)
    idx = ShardedSyntheticIndex(n, 512, seed=2024, rank=0, world=1, local_device=0, k_max=128, force_collective=True,
                                vector_dtype=args.dtype)
    rng = np.random.default_rng(4242)
    Q = rng.standard_normal((max(NQS), 512)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    Qd = torch.from_numpy(Q).to(idx.device)
    qptrs = [Qd[b].data_ptr() for b in range(Q.shape[0])]
    k = args.k

    def batch(nq, prune=False):
        t0 = time.perf_counter()
        if prune:
            keys, counts = idx.topk_batch_async(Q[:nq], k, prune=True)
        else:
            keys, counts = idx.topk_batch_async(Q[:nq], k)
        torch.cuda.synchronize(idx.device)
        return (time.perf_counter() - t0) * 1e3 / nq, keys[:, :k].clone()

    def loop(nq):
        got = []
        t0 = time.perf_counter()
        for b in range(nq):
            keys, _ = idx.topk_async(qptrs[b], k)
            got.append(keys[:k].clone())  # (a 800-byte device copy per query, enqueued: what a caller that keeps them pays)
        torch.cuda.synchronize(idx.device)
        return (time.perf_counter() - t0) * 1e3 / nq, torch.stack(got)

    lines = []
    try:
        for nq in NQS:
            for _ in range(2):  # warm-up rounds: the side buffer, the batch target, the shadow, RCCL's first call
                batch(nq)
                loop(nq)
                if args.prune:
                    batch(nq, prune=True)
            a_ms, b_ms, c_ms, same = [], [], [], True
            for _ in range(args.reps):
                ta, ka = batch(nq)
                tb, kb = loop(nq)
                a_ms.append(ta)
                b_ms.append(tb)
                same = same and bool(torch.equal(ka, kb))
                if args.prune:
                    tc, kc = batch(nq, prune=True)
                    c_ms.append(tc)
                    same = same and bool(torch.equal(kc, kb))
            idx.xchg.assert_no_overflow_seen()
            a, b = spread(a_ms), spread(b_ms)
            line = {"rows": n, "dtype": args.dtype, "k": k, "nq": nq, "reps": args.reps, "batch_ms_per_query": a,
                    "loop_ms_per_query": b, "ratio_of_medians": a["median"] / b["median"], "same_keys": same}
            if args.prune:
                c = spread(c_ms)
                surv, why = idx.local.prune_batch_dev_counts()  # of the last pruned chunk
                line.update({"pruned_batch_ms_per_query": c, "pruned_over_batch": c["median"] / a["median"],
                             "pruned_over_loop": c["median"] / b["median"],
                             # a win counts only where the gap exceeds the two spreads together
                             "pruned_beats_batch": bool(a["median"] - c["median"] > a["spread"] + c["spread"]),
                             "pruned_beats_loop": bool(b["median"] - c["median"] > b["spread"] + c["spread"]),
                             "survivors": surv.tolist(), "fail_bits": why.tolist(),
                             "loop_is_pruned": bool(idx.local.prune_stats()["eligible"])})
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
    finally:
        idx.close()
        dist.destroy_process_group()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
