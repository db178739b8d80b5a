"""The two-output (multi_reg_neg) fit, host wall time, one MI355X, one process:
  * per shape -- the golden cases of tests/golden/multiregneg.npz and a 390-row set (30 rounds x 13 tiles) of dim 512 --
    `fit2` (ssw_fb_fit2: host-driven, the O(dim) tail on the host; unchanged from the parent commit) against `fit2_dev`
    (ssw_fb_fit2_batch with one slot: k_fb_fit2_wg, the whole fit in one launch) against the host-driven fit over the
    device evaluation (SSW_FB_HOST_DRIVER);
  * per S -- a loop of S single device fits against ONE `fit2_batch` over S engines, 390 rows each.
The sides alternate inside each repetition, after `--warmup` unrecorded repetitions of the whole round; the figures are
medians of `--reps` with min / max.  One JSON line per shape and per S.
    python tools/perf_fit2.py [--sessions 4,16,64]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from seesaw_amd.feedback import FeedbackEngine

TILES, ROUNDS, DIM = 13, 30, 512
L_NORM, L_QUERY = 100.0, 10.0


def unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def synthetic(rng, n_images=ROUNDS):
    """a session 30 rounds in: 13 tiles an image, a third of the images of the target class (one tile pulled towards
    it), a sixth of the confusion class"""
    n = n_images * TILES
    target, confusion = unit(rng.standard_normal(DIM)), unit(rng.standard_normal(DIM))
    X = unit(rng.standard_normal((n, DIM)))
    ys = np.zeros((n, 2), np.float32)
    for im in range(n_images):
        row = im * TILES + int(rng.integers(0, TILES))
        if im % 3 == 0:
            X[row] = unit(0.45 * X[row] + 0.55 * target)
            ys[row, 0] = 1
        elif im % 6 == 1:
            X[row] = unit(0.45 * X[row] + 0.55 * confusion)
            ys[row, 1] = 1
    q = unit(target + 0.35 * unit(rng.standard_normal(DIM)))
    w0 = (rng.uniform(-1, 1, (2, DIM)) / np.sqrt(DIM)).astype(np.float32)
    return dict(name=f"synthetic n={n}", X=X, ys=ys, sw=np.full(n, 1.0 / TILES, np.float32), q=q, w0=w0, l_norm=L_NORM,
                l_query=L_QUERY)


def golden():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "multiregneg.npz")
    g = np.load(path)
    for c in range(int(g["n_cases"])):
        _, inv, cnt = np.unique(g[f"c{c}_img"], return_inverse=True, return_counts=True)
        yield dict(name=f"golden c{c} n={g[f'c{c}_X'].shape[0]}", X=g[f"c{c}_X"], ys=g[f"c{c}_ys"], sw=1.0 / cnt[inv],
                   q=g[f"c{c}_q"], w0=g[f"c{c}_w0"], l_norm=float(g[f"c{c}_l_norm"]), l_query=float(g[f"c{c}_l_query"]))


def engine(s):
    eng = FeedbackEngine(s["X"].shape[1])
    eng.set_data(s["X"], center=True)
    eng.set_targets2(s["ys"], s["sw"])
    eng.set_query(s["q"])
    return eng


def stat(t):
    return [round(float(np.median(t)), 4), round(float(np.min(t)), 4), round(float(np.max(t)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="4,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=100)
    args = ap.parse_args()
    assert "SSW_FB_HOST_DRIVER" not in os.environ
    rng = np.random.default_rng(11)
    for s in list(golden()) + [synthetic(rng)]:
        eng = engine(s)
        a = (s["w0"], s["l_norm"], s["l_query"], args.max_iter, 1.0)
        t_host, t_dev, t_hostdev = [], [], []
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            _, i_host = eng.fit2(*a)
            t1 = time.perf_counter()
            W_dev, i_dev = eng.fit2_dev(*a)
            t2 = time.perf_counter()
            os.environ["SSW_FB_HOST_DRIVER"] = "1"
            try:
                t3 = time.perf_counter()
                W_hd, i_hd = eng.fit2_dev(*a)
                t4 = time.perf_counter()
            finally:
                del os.environ["SSW_FB_HOST_DRIVER"]
            if rep >= args.warmup:
                t_host.append(1e3 * (t1 - t0))
                t_dev.append(1e3 * (t2 - t1))
                t_hostdev.append(1e3 * (t4 - t3))
        assert i_dev["on_device"] and not i_hd["on_device"]
        print(json.dumps({"shape": s["name"], "dim": int(s["X"].shape[1]), "reps": args.reps,
                          "fit2_host_tail_ms_median_min_max": stat(t_host), "fit2_host_tail_evals": i_host["func_evals"],
                          "fit2_dev_one_launch_ms_median_min_max": stat(t_dev), "fit2_dev_evals": i_dev["func_evals"],
                          "fit2_dev_host_driven_ms_median_min_max": stat(t_hostdev),
                          "host_tail_us_per_eval": round(1e3 * float(np.median(t_host)) / i_host["func_evals"], 1),
                          "one_launch_us_per_eval": round(1e3 * float(np.median(t_dev)) / i_dev["func_evals"], 1),
                          "host_driven_dev_us_per_eval": round(1e3 * float(np.median(t_hostdev)) / i_hd["func_evals"], 1),
                          "one_launch_over_host_tail": round(float(np.median(t_dev) / np.median(t_host)), 3),
                          "drivers_identical": bool(np.array_equal(W_dev.view(np.uint32), W_hd.view(np.uint32))
                                                    and i_dev["func_evals"] == i_hd["func_evals"])}), flush=True)
        eng.close()
    sessions = [int(x) for x in args.sessions.split(",")]
    slots = [synthetic(rng) for _ in range(max(sessions))]
    engines = [engine(s) for s in slots]
    for S in sessions:
        eng, sl = engines[:S], slots[:S]
        ba = ([s["w0"] for s in sl], [L_NORM] * S, [L_QUERY] * S, [args.max_iter] * S, [1.0] * S)
        t_batch, t_loop = [], []
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            got = FeedbackEngine.fit2_batch(eng, *ba)
            t1 = time.perf_counter()
            want = [e.fit2_dev(s["w0"], L_NORM, L_QUERY, args.max_iter, 1.0) for e, s in zip(eng, sl)]
            t2 = time.perf_counter()
            if rep >= args.warmup:
                t_batch.append(1e3 * (t1 - t0))
                t_loop.append(1e3 * (t2 - t1))
        identical = all(np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1] == b[1] for a, b in zip(got, want))
        evals = [w[1]["func_evals"] for w in want]
        print(json.dumps({"sessions": S, "rows": int(engines[0].n), "dim": DIM, "reps": args.reps,
                          "fit2_batch_ms_median_min_max": stat(t_batch), "loop_of_fits_ms_median_min_max": stat(t_loop),
                          "batch_over_loop": round(float(np.median(t_batch) / np.median(t_loop)), 3),
                          "batch_us_per_fit": round(1e3 * float(np.median(t_batch)) / S, 1),
                          "loop_us_per_fit": round(1e3 * float(np.median(t_loop)) / S, 1),
                          "func_evals_min_median_max": [int(min(evals)), int(np.median(evals)), int(max(evals))],
                          "identical": bool(identical)}), flush=True)
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
