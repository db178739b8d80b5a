#!/usr/bin/env python3
"""Chunk selection (DeviceIndex.chunk_select; csrc/select.hip: k_chunk_*) against the per-slot selections, in one
process on one GPU: every call once with the setting off and once with it on, in alternating order, a warm-up pair
first, the result bits of both compared on every call ("Chunk selection").
SessionGroup.CHUNK_SELECT is read from this tool's output.

    python tools/perf_chunk_select.py [--reps 31] [--k 50] [--cases a b c d] [--rounds 33]

  a  topk_batch, nq = 2 / 4 / 8 / 16: 120 000 images x 13 tiles at dim 512, f32
  b  the same rows without an image map (row = image)
  c  views_topk_batch on the category views of tools/perf_views_batch.py (1 109 images each), S = 2 / 16
  d  LabelPropagation.round_batch as in tools/perf_round_batch.py (1.56 M nodes, knn_k = 10 graph, shortlist 50),
     S = 2 / 3 / 4 / 8 / 16: two sets of S graph handles on one index are fed the same scripted sessions, one set's
     call with the setting off, the other's with it on, --rounds rounds of which the first two (the prior ranking, the
     first full propagation) are left out

One JSON line a case and size: the host-to-host microseconds A SLOT of `off` and `on` as median and interquartile range
over --reps calls (d: over the steady rounds); `ahead`: on's median is below off's by more than both interquartile
ranges; `identical`: same images, score bits and rows every call; `stats`: chunk_select_stats() of one on call (d: of
the whole run).  The kernel times of the on side come from a run of their own, under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perf_chunk_select.py --on-only --cases a c
read with --kernel-stats DIR (profiles/chunk_select_kernel_stats.txt)."""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2]) and
                                    np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def report(tag, s, reps, us, identical, stats):
    out = {"case": tag, "slots": s, "reps": reps, "identical": bool(identical), "stats": stats}
    stat = {}
    for on, name in ((False, "off"), (True, "on")):
        if not us[on]:
            continue
        q1, med, q3 = np.percentile(us[on], [25, 50, 75])
        stat[name] = (med, q3 - q1)
        out[name + "_us_per_slot"] = round(float(med), 2)
        out[name + "_iqr"] = round(float(q3 - q1), 2)
    if len(stat) == 2:
        out["ahead"] = bool(stat["off"][0] - stat["on"][0] > max(stat["off"][1], stat["on"][1]))
    print(json.dumps(out), flush=True)


def measure(tag, owner, sizes, call, reps, on_only=False):
    for s in sizes:
        us = {False: [], True: []}
        identical, stats = True, None
        for rep in range(reps + 1):
            got = {}
            for i in range(2):
                on = bool((i + rep) % 2)
                if on_only and not on:
                    continue
                owner.chunk_select = on
                before = owner.chunk_select_stats()
                t0 = time.perf_counter()
                got[on] = call(s)
                t = 1e6 * (time.perf_counter() - t0) / s
                if rep:
                    us[on].append(t)
                if on:
                    after = owner.chunk_select_stats()
                    stats = {key: after[key] - before[key] for key in after}
            identical = identical and (on_only or same(got[False], got[True]))
        report(tag, s, reps, us, identical, stats)
    owner.chunk_select = False


def graph_round(args):
    """case d: tools/perf_round_batch.py's index, graph and scripted sessions; set `off` and set `on` both take
    round_batch, the index's setting switched before each call, alternating which goes first"""
    from scipy.special import expit
    from seesaw_amd.label_propagation import LabelPropagation
    from seesaw_amd.loops.graph_based import _locality_order_of, get_weight_matrix_from_index
    from seesaw_amd.synthetic import make_dataset
    matrix = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
    ds = make_dataset("lvis", n_images=120000, tiles_per_image=13, n_categories=2, positive_frac=0.05, seed=11, knn_k=10)
    ds.embedding.noise = 1.2
    index = ds.load_index("multiscale", options={"use_vec_index": False})
    dev = index._dev
    W = get_weight_matrix_from_index(index, matrix)
    order = _locality_order_of(W)
    n, n_images = W.shape[0], dev.n_images
    priors = [expit(10.0 * (np.asarray(index.score(index.string2vec(string=f"a c{c}")), dtype=np.float64) - 0.4)) for c in (0, 1)]
    sides = [True] if args.on_only else [False, True]
    sets = {on: [LabelPropagation(W, reg_lambda=1.0, max_iter=300, node_order=order, device=dev.device) for _ in range(16)]
            for on in sides}
    for S in (2, 3, 4, 8, 16):
        for hs in sets.values():
            for j, lp in enumerate(hs[:S]):
                lp.set_prior(priors[j % 2])  # (a fresh session: the kept iterates are dropped)
        scripts = [np.random.default_rng(1000 + j) for j in range(S)]
        labels, excluded = [dict() for _ in range(S)], [[] for _ in range(S)]
        us = {False: [], True: []}
        identical, before = True, dev.chunk_select_stats()
        for rnd in range(args.rounds):
            prop, ids, vals, exs = [], [], [], []
            for j in range(S):
                rng = scripts[j]
                for v in rng.choice(n, size=int(rng.integers(1, 14)), replace=False):
                    labels[j][int(v)] = float(rng.integers(0, 2))
                if rnd == 1:
                    labels[j][int(rng.integers(0, n))] = 0.0  # every session propagates from its second round on
                excluded[j].append(int(rng.integers(0, n_images)))
                i = np.array(sorted(labels[j]), dtype=np.int64)
                v = np.array([labels[j][int(x)] for x in i], dtype=np.float64)
                p = rnd >= 1 and bool((v == 0).any())
                prop.append(p), ids.append(i), vals.append(v if p else np.zeros(i.shape[0]))
                exs.append(np.array(sorted(set(excluded[j])), dtype=np.int64))
            got = {}
            for i in range(len(sides)):
                on = sides[(i + rnd) % len(sides)]
                dev.chunk_select = on
                with contextlib.redirect_stdout(io.StringIO()):
                    t0 = time.perf_counter()
                    got[on] = LabelPropagation.round_batch(sets[on][:S], dev, propagate=prop, label_ids=ids, label_values=vals,
                                                           mask_labeled=True, excluded=exs, k=args.k)
                    t = 1e6 * (time.perf_counter() - t0) / S
                if rnd >= 2:
                    us[on].append(t)
            identical = identical and (args.on_only or same(got[False], got[True]))
        after = dev.chunk_select_stats()
        report("d_round_batch", S, args.rounds - 2, us, identical, {key: after[key] - before[key] for key in after})
    dev.chunk_select = False


def kernel_stats(directory):
    """the selection's kernels out of a rocprofv3 --stats run: name, calls, total us, mean us"""
    import re
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            m = re.search(r"\bk_[a-z0-9_]+|[a-z_]*scores?_kernel|views_[a-z_]+", r.get("Name", ""))
            if m:
                rows.append((m.group(0), int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3, float(r["AverageNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--cases", nargs="+", default=["a", "b", "c", "d"])
    ap.add_argument("--rounds", type=int, default=33, help="case d: rounds a session (the first two are not timed)")
    ap.add_argument("--on-only", action="store_true", help="the setting-on side alone (the profiled run)")
    ap.add_argument("--kernel-stats", default=None, help="print the kernels out of a rocprofv3 --stats directory and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        for name, calls, total, mean in kernel_stats(args.kernel_stats):
            print(f"{name:40s} calls {calls:6d}  total {total:10.1f} us  mean {mean:7.2f} us")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_chunk_select: no GPU (timings are not taken on a CPU)")
    from seesaw_amd.device_index import DeviceIndex
    n_images, tiles = 120_000, 13
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((16, 512)).astype(np.float32)
    Q = np.ascontiguousarray(Q / np.linalg.norm(Q, axis=1, keepdims=True), dtype=np.float32)
    excluded = [rng.choice(n_images, 60, replace=False).tolist() for _ in range(16)]
    idx = DeviceIndex.synthetic(n_images * tiles, 512, seed=4)
    try:
        if "b" in args.cases:
            measure("b_topk_batch_no_map", idx, (2, 4, 8, 16), lambda s: idx.topk_batch(Q[:s], args.k, excluded=excluded[:s]),
                    args.reps, args.on_only)
        idx.set_row2image(np.repeat(np.arange(n_images), tiles).astype(np.int32))
        if "a" in args.cases:
            measure("a_topk_batch", idx, (2, 4, 8, 16), lambda s: idx.topk_batch(Q[:s], args.k, excluded=excluded[:s]),
                    args.reps, args.on_only)
        if "c" in args.cases:
            vr = np.random.default_rng(11)
            views = [idx.view(np.sort(vr.choice(n_images, 1109, replace=False))) for _ in range(16)]
            try:
                measure("c_views_topk_batch", idx, (2, 16),
                        lambda s: DeviceIndex.views_topk_batch(views[:s], Q[:s], args.k), args.reps, args.on_only)
            finally:
                for v in views:
                    v.close()
    finally:
        idx.close()
    if "d" in args.cases:
        graph_round(args)


if __name__ == "__main__":
    main()
