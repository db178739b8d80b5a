"""A/B of the batched L-KNN step against the loop of single calls, in one process, on the tree it is run from: S
device-resident models (DeviceLKNNModel) over one directed 10-NN graph (uniformly random neighbours: gathers without any
locality) of 3000, 50 000, 200 000 and 1.56 M nodes, priors 0.1 +- 1e-6 of their own, S in {2, 3, 4, 8, 16}:

  lknn           the S calls  m.top_k_remaining(1)        against  DeviceLKNNModel.top_k_remaining_batch(models, [1] * S)
  active_search  the S calls  m.step(K=4, lookahead=2)    against  DeviceLKNNModel.step_batch(models, [4] * S, [2] * S)
                 (reward_horizon 5)

Both read the same state, so a round times the two one after the other -- which one first alternates from round to round --
checks that they picked the same nodes, and then answers every model's pick (the same answers for both, whoever ran
first).  One warm-up round, then --rounds timed rounds.  Reported: median [interquartile range] in us per session-step
(the call's host time / S; every call ends in its host wait), and the device-event times of the selection and look-ahead
phases: of one single step (model 0's) and of the whole batched pass (all S slots).

    python tools/perf_lknn_batch.py [--sizes 3000,50000,200000,1560000] [--sessions 2,3,4,8,16] [--rounds 30]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

from seesaw_amd import _lib
from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
from seesaw_amd.research.active_search.common import Dataset

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="3000,50000,200000,1560000")
ap.add_argument("--sessions", default="2,3,4,8,16")
ap.add_argument("--rounds", type=int, default=30)
args = ap.parse_args()
SIZES = [int(x) for x in args.sizes.split(",")]
SESSIONS = [int(x) for x in args.sessions.split(",")]
D, K = 10, 4

import ctypes

count = _lib.c_i32(0)
_lib.call("ssw_device_count", ctypes.byref(count))
if count.value < 1:
    sys.exit("perf_lknn_batch: no GPU")


def graph(n):
    rng = np.random.default_rng(n)
    nbr = rng.integers(0, n, size=(n, D), dtype=np.int32)
    return sp.csr_array((np.ones(n * D), nbr.reshape(-1), np.arange(0, n * D + 1, D)), shape=(n, n))


def spread(x):
    q1, med, q3 = np.percentile(np.asarray(x, dtype=np.float64), [25, 50, 75])
    return f"{med:8.1f} [{q3 - q1:6.1f}]"


def single_lknn(models):
    return [int(m.top_k_remaining(1)[0][0]) for m in models]


def batch_lknn(models):
    return [int(e[0][0]) for e in DeviceLKNNModel.top_k_remaining_batch(models, [1] * len(models))]


def single_active(models):
    return [m.step(K, 2)[0] for m in models]


def batch_active(models):
    return [e[0] for e in DeviceLKNNModel.step_batch(models, [K] * len(models), [2] * len(models))]


MODES = {"lknn": (single_lknn, batch_lknn), "active_search": (single_active, batch_active)}

print(f"# directed {D}-NN graphs with random neighbours; lknn: top_remaining k = 1; active_search: K = {K}, lookahead 2; 1 warm-up "
      f"round + {args.rounds} timed rounds, loop / batch alternating over the same answers")
print("# us per session-step: median [interquartile range]; device events in us: one single step | the whole batched pass")
verdict = {}
for n in SIZES:
    W = graph(n)
    every = [DeviceLKNNModel.from_dataset(Dataset.from_vectors(np.zeros((n, 1))), weight_matrix=W,
                                          gamma=np.random.default_rng(1000 + j).normal(0.1, 1e-6, n)) for j in range(max(SESSIONS))]
    every[0].step_times(True)
    for S in SESSIONS:
        for mode, (single, batch) in MODES.items():
            models = every[:S]  # (they keep the answers of the sweeps before: a few hundred of n nodes)
            t = {"loop": [], "batch": []}
            ev = {"loop": [], "batch": []}
            for r in range(args.rounds + 1):
                picks = {}
                for which in (("loop", "batch") if r % 2 else ("batch", "loop")):
                    fn = single if which == "loop" else batch
                    t0 = time.perf_counter()
                    picks[which] = fn(models)
                    dt = time.perf_counter() - t0
                    ms = models[0].step_times(True)
                    if r:
                        t[which].append(dt / S * 1e6)
                        if ms is not None:
                            ev[which].append(ms)
                assert picks["loop"] == picks["batch"], (n, S, mode, r, picks)
                for m, i in zip(models, picks["loop"]):
                    m.condition_(i, r % 2)
            lo, ba = np.asarray(t["loop"]), np.asarray(t["batch"])
            iqr = lambda x: np.subtract(*np.percentile(x, [75, 25]))
            ahead = np.median(lo) - np.median(ba) > max(iqr(lo), iqr(ba))
            verdict.setdefault(mode, {}).setdefault(S, []).append(bool(ahead))
            line = (f"n={n:8d} S={S:2d} {mode:13s} loop {spread(lo)}  batch {spread(ba)}  "
                    f"{'batch ahead by more than both IQRs' if ahead else 'not ahead'}")
            for name, col in (("selection", 0), ("look-ahead", 1)):
                a, b = (np.asarray(ev[w], dtype=np.float64).reshape(-1, 2)[:, col] * 1e3 for w in ("loop", "batch"))
                if a.shape[0] and (a >= 0).all() and b.shape[0] and (b >= 0).all():
                    line += f"  {name} {np.median(a):8.1f} | {np.median(b):8.1f} ({np.median(b) / np.median(a) / S:4.2f} x S singles)"
            print(line, flush=True)
    for m in every:
        m.close()
print("# smallest S at which the batch is ahead at every measured size (and at every larger S measured):")
for mode, by_s in verdict.items():
    good = [S for S in sorted(by_s) if all(all(by_s[T]) for T in by_s if T >= S)]
    print(f"#   {mode}: {good[0] if good else None}   " + "  ".join(f"S={S}: {sum(v)}/{len(v)} sizes" for S, v in sorted(by_s.items())))
