#!/usr/bin/env python3
"""One call of each kind that reaches the index's selection, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/trace_topk_paths.py

Host top-k with the full scan and pruned, the one-launch top-k of a small index, the device form with an exchange
target, a batch of 5 (a chunk of 4 and a single query) plain, pruned and with the second stage, score_rows and
rescore_avg, on the lab build (the pruning is forced on at this size).  Two builds launch the same kernels when their
*_kernel_stats.csv agree in names and calls (profiles/topk_paths_kernel_stats_*.txt and index_split_kernel_stats_*.txt:
tools/trace_topk_paths.py --summary OUT/.../*_kernel_stats.csv)."""
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(path):
    rows = sorted((r["Name"], int(r["Calls"])) for r in csv.DictReader(open(path)))
    print("rocprofv3 --kernel-trace --stats --output-format csv -- python tools/trace_topk_paths.py: calls, kernel")
    for name, calls in rows:
        print(f"{calls:6d}  {name}")


def main():
    import torch
    from oracle import seesaw_oracle as orc
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.sharded import ShardedTopK
    n_images, dim, k = 35000, 512, 50
    row2image = np.repeat(np.arange(n_images), 2).astype(np.int32)
    n = row2image.shape[0]
    Q = np.stack([orc.synth_query(i, dim) for i in range(6)])
    with _lib.debug_hooks():
        idx = DeviceIndex.synthetic(n, dim, seed=3)
        idx.set_row2image(row2image)
        idx.set_tile_meta(np.tile(np.array([[0, 0, 1, 1], [0, 0, .5, .5]], np.float32), (n_images, 1)),
                          np.tile(np.array([0, 1], np.int32), n_images))
        small = DeviceIndex.synthetic(13000, dim, seed=4)
        small.set_row2image(np.repeat(np.arange(1000), 13).astype(np.int32))
        _lib.call("ssw_tune_prune", 0, -1, -1)
        idx.topk(Q[0], k, excluded=[1, 2, 3])
        _lib.call("ssw_tune_prune", 1, 1, -1)
        idx.topk(Q[0], k, excluded=[1, 2, 3])
        small.topk(Q[1], k, excluded=[4])
        dev = torch.device("cuda", 0)
        q_dev = torch.from_numpy(Q[2]).to(dev)
        x = ShardedTopK(rank=0, world=1, device=dev, image_offset=0, k_max=64, with_best=True).attach(idx)
        torch.cuda.synchronize()
        idx.topk_dev(q_dev.data_ptr(), k)
        idx.sync()
        _lib.call("ssw_index_set_exchange_target", idx._h, None, 0, 0, 0, 0)
        idx.topk_batch(Q[:5], k, excluded=[[1], None, [2, 3], None, [5]])
        idx.topk_batch(Q[:5], k, excluded=[[1], None, [2, 3], None, [5]], prune=True)
        idx.topk_batch_avg(Q[:5], k, "greater")
        idx.score_rows(Q[5], np.arange(0, n, 101))
        idx.rescore_avg(np.arange(0, n_images, 301), "greater")
        _lib.call("ssw_tune_prune", 1, -1, -1)
        del x
        idx.close()
        small.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        main()
