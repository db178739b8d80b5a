"""S sessions' multi_reg fits: one FeedbackEngine.fit_batch (one launch of k_fb_fit_wg_batch, one host wait) against the
loop of S single `fit` calls (S launches of k_fb_fit_wg, S host waits), host wall time, one MI355X, one process.
Every session's labelled set is 390 rows (30 rounds x 13 tiles) of dim 512 gathered from a resident synthetic index;
the objective is the `multi_reg` loop's (CE, balanced positives, norm regulariser 100, max_iter 200).  The two sides
alternate inside each repetition; the figures are medians of `--reps` after `--warmup`, with min / max.
One JSON line per S.   python tools/perf_fit_batch.py [--sessions 1,2,4,8,16,64,256]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from seesaw_amd import _lib
from seesaw_amd.device_index import DeviceIndex
from seesaw_amd.feedback import FeedbackEngine

TILES, ROUNDS, DIM = 13, 30, 512


def unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,2,4,8,16,64,256")
    ap.add_argument("--images", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=200)
    args = ap.parse_args()
    rng = np.random.default_rng(11)
    n_rows = args.images * TILES
    X = rng.standard_normal((n_rows, DIM)).astype(np.float32)
    hidden = unit(rng.standard_normal((8, DIM)))
    pos_images = [rng.choice(args.images, size=args.images // 20, replace=False) for _ in range(hidden.shape[0])]
    for c, imgs in enumerate(pos_images):  # a positive image: one tile pulled towards its category's direction
        rows = imgs * TILES + rng.integers(0, TILES - 1, size=imgs.shape[0])
        X[rows] = unit(X[rows]) * 0.45 + hidden[c] * 0.55
    X = unit(X)
    index = DeviceIndex.from_numpy(X, row2image=(np.arange(n_rows) // TILES).astype(np.int32), device=0)
    obj = _lib.FbObjective(kind=_lib.SSW_FB_MULTIREG, loss_type=_lib.SSW_FB_LOSS_CE, fit_intercept=0, reg_kind=0,
                           pos_weight=-1.0, reg_weight=0.0, margin=0.2, reg_norm_lambda=100.0, reg_data_lambda=0.0,
                           reg_query_lambda=0.0)
    s_max = max(int(s) for s in args.sessions.split(","))
    engines, w0s = [], []
    for s in range(s_max):  # a session 30 rounds in: 30 shown images, a third of them of its category
        c = s % hidden.shape[0]
        pos = rng.choice(pos_images[c], size=ROUNDS // 3, replace=False)
        neg = rng.choice(np.setdiff1d(np.arange(args.images), pos), size=ROUNDS - pos.shape[0], replace=False)
        images = np.sort(np.concatenate([pos, neg]))
        rows = (images[:, None] * TILES + np.arange(TILES)[None, :]).reshape(-1)
        y = (X[rows] @ hidden[c] > 0.4).astype(np.float64)
        q = unit(hidden[c] + 0.35 * unit(rng.standard_normal(DIM)))
        eng = FeedbackEngine(DIM)
        eng.set_query(q)
        eng.set_data_from_index(index, rows, center=True)
        eng.set_targets(y, np.full(rows.shape[0], 1.0 / TILES))
        engines.append(eng)
        w0s.append(q)
    for S in (int(s) for s in args.sessions.split(",")):
        eng, w0 = engines[:S], w0s[:S]
        objs, mi, lr = [obj] * S, [args.max_iter] * S, [1.0] * S
        t_batch, t_loop = [], []
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            got = FeedbackEngine.fit_batch(eng, objs, w0, mi, lr)
            t1 = time.perf_counter()
            want = [e.fit(obj, w, args.max_iter, 1.0) for e, w in zip(eng, w0)]
            t2 = time.perf_counter()
            if rep >= args.warmup:
                t_batch.append(1e3 * (t1 - t0))
                t_loop.append(1e3 * (t2 - t1))
        identical = all(np.array_equal(g[0].view(np.uint32), w[0].view(np.uint32)) and g[1] == w[1]
                        for g, w in zip(got, want))
        evals = [w[1]["func_evals"] for w in want]
        stat = lambda t: [round(float(np.median(t)), 4), round(float(np.min(t)), 4), round(float(np.max(t)), 4)]  # noqa: E731
        print(json.dumps({"sessions": S, "rows": int(engines[0].n), "dim": DIM, "reps": args.reps,
                          "fit_batch_ms_median_min_max": stat(t_batch), "loop_of_fits_ms_median_min_max": stat(t_loop),
                          "batch_over_loop": round(float(np.median(t_batch) / np.median(t_loop)), 3),
                          "batch_us_per_fit": round(1e3 * float(np.median(t_batch)) / S, 1),
                          "loop_us_per_fit": round(1e3 * float(np.median(t_loop)) / S, 1),
                          "func_evals_min_median_max": [int(min(evals)), int(np.median(evals)), int(max(evals))],
                          "identical": bool(identical)}), flush=True)
    for e in engines:
        e.close()
    index.close()


if __name__ == "__main__":
    main()
