"""A/B of the batched graph round (LabelPropagation.round_batch -> ssw_labelprop_round_batch) against the loop of single
rounds (LabelPropagation.round) it replaces, at the bench's feedback shape: 120 000 images x 13 tiles = 1.56 M nodes, the
knn_k = 10 graph, the index's selection over per-image maxima, shortlist 50.

Two sets of S graph handles over ONE index are fed the same scripted sessions -- 30 rounds, 1-13 new labels a round, one
more excluded image a round -- in one process, round by round, alternating which set goes first: set A takes S `round`
calls, set B one `round_batch`.  Reported for S = 2, 3, 4, 8, 16: the median time per session-round of each and its spread
(interquartile range) over the steady rounds (the first two rounds of a session -- the prior ranking, the first full
propagation -- are left out), and the batched call's stats (slots in the batched pass, its launches, host waits).
The kernel time of the batched pass comes from a second run of its own, under
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/perf_round_batch.py --sizes 16 --batched-only
whose per-kernel table is read with --kernel-stats DIR (the *_b kernels are the pass).

    python tools/perf_round_batch.py [--sizes 2,3,4,8,16] [--rounds 30] [--out profiles/round_batch_ab.txt]"""
import argparse
import contextlib
import csv
import glob
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy.special import expit


def kernel_stats(directory):
    """the *_b kernels (and the selection's, for scale) out of a rocprofv3 --stats run: name, calls, total us, mean us"""
    import re
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            m = re.search(r"\bk_[a-z0-9_]+", r.get("Name", ""))
            if m and re.match(r"k_(inc_|lp_|select|image_max|excl|final)", m.group(0)):
                rows.append((m.group(0), int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3, float(r["AverageNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,3,4,8,16")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--images", type=int, default=120000)
    ap.add_argument("--batched-only", action="store_true", help="set B alone (the profiled run)")
    ap.add_argument("--kernel-stats", default=None, help="print the pass's kernels out of a rocprofv3 --stats directory and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        for name, calls, total, mean in kernel_stats(args.kernel_stats):
            print(f"{name:40s} calls {calls:6d}  total {total:10.1f} us  mean {mean:7.2f} us")
        return
    from seesaw_amd.label_propagation import LabelPropagation
    from seesaw_amd.loops.graph_based import _locality_order_of, get_weight_matrix_from_index
    from seesaw_amd.synthetic import make_dataset
    sizes = [int(s) for s in args.sizes.split(",")]
    matrix = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
    ds = make_dataset("lvis", n_images=args.images, tiles_per_image=13, n_categories=2, positive_frac=0.05, seed=11, knn_k=10)
    ds.embedding.noise = 1.2
    index = ds.load_index("multiscale", options={"use_vec_index": False})
    dev = index._dev
    W = get_weight_matrix_from_index(index, matrix)
    order = _locality_order_of(W)
    n, n_images = W.shape[0], dev.n_images
    # the prior of a knn_prop2 session: the calibrated scan scores of its text query
    priors = [expit(10.0 * (np.asarray(index.score(index.string2vec(string=f"a c{c}")), dtype=np.float64) - 0.4)) for c in (0, 1)]
    S_max = max(sizes)
    sets = {}
    for name in ("single", "batched"):
        if name == "single" and args.batched_only:
            continue
        sets[name] = [LabelPropagation(W, reg_lambda=1.0, max_iter=300, node_order=order, device=dev.device) for _ in range(S_max)]
    lines = [f"# tools/perf_round_batch.py: {n} nodes ({n_images} images x 13 tiles), knn_k = 10 graph, node order "
             f"{'on' if order is not None else 'off'}, shortlist 50, {args.rounds} rounds a session, 1-13 labels a round",
             "# per session-round, steady rounds (round >= 2): median [interquartile range], microseconds",
             f"# {'S':>2s} {'loop of round':>22s} {'round_batch':>22s} {'ratio':>6s}   batched slots / launches / waits of a steady call (median)"]
    print("\n".join(lines))
    for S in sizes:
        for hs in sets.values():
            for j, lp in enumerate(hs[:S]):
                lp.set_prior(priors[j % 2])  # (a fresh session: the kept iterates are dropped)
        scripts = [np.random.default_rng(1000 + j) for j in range(S)]
        labels = [dict() for _ in range(S)]
        excluded = [[] for _ in range(S)]
        t_single, t_batch, stats = [], [], []
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

            def run_single():
                t0 = time.perf_counter()
                out = [lp.round(dev, propagate=prop[j], label_ids=ids[j], label_values=vals[j], mask_labeled=True, excluded=exs[j],
                                k=50) for j, lp in enumerate(sets["single"][:S])]
                return time.perf_counter() - t0, out

            def run_batch():
                t0 = time.perf_counter()
                out = LabelPropagation.round_batch(sets["batched"][:S], dev, propagate=prop, label_ids=ids, label_values=vals,
                                                   mask_labeled=True, excluded=exs, k=50)
                return time.perf_counter() - t0, out

            with contextlib.redirect_stdout(io.StringIO()):
                if args.batched_only:
                    tb, ob = run_batch()
                    ts, os_ = tb, ob
                elif rnd % 2 == 0:
                    ts, os_ = run_single()
                    tb, ob = run_batch()
                else:
                    tb, ob = run_batch()
                    ts, os_ = run_single()
            for a, b in zip(os_, ob):  # faster and different is not faster
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), (S, rnd)
            if rnd >= 2:
                t_single.append(ts / S), t_batch.append(tb / S), stats.append(LabelPropagation.last_batch_stats)
        q = lambda t: np.percentile(np.asarray(t) * 1e6, [25, 50, 75])  # noqa: E731
        (s25, s50, s75), (b25, b50, b75) = q(t_single), q(t_batch)
        st = np.median(np.asarray(stats), axis=0)
        line = (f"  {S:2d} {s50:9.1f} [{s75 - s25:6.1f}]      {b50:9.1f} [{b75 - b25:6.1f}]      {b50 / s50:6.2f}   "
                f"{st[0]:.0f} / {st[1]:.0f} / {st[2]:.0f}  (single-path slots {st[3]:.0f})")
        print(line)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
