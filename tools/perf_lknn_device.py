"""A/B of interactive_options["model_on_device"] for the two active-search loops, in one process: sessions of the
`active_search` loop (reward_horizon 5) and of the `lknn` loop on a synthetic 1.56 M-vector dataset made like the one of the
README's loop numbers, over its directed (regular) k-NN graph -- but as 1.56 M images of one tile, not 120 000 x 13: both
loops show the image of the node they pick, and two tiles of one image picked in one session end it ("returned a
repeated dbidx", on either path).  The option alternates off / on over the
same scripted answers: one warm-up pair, then --pairs timed pairs.  Per round: median and interquartile range of
next_batch, refine and set_text_vec, each on its own (host clock; next_batch ends in a host wait on either path, refine
on the device path only enqueues -- its kernel is waited for by the next next_batch), and the device-event times of the
selection pass and the look-ahead kernel.  The images shown must agree between the two paths, round by round.

    python tools/perf_lknn_device.py [--images 1560000] [--tiles 1] [--batches 30] [--pairs 3]"""
import argparse
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from seesaw_amd.basic_types import BenchParams, IndexSpec, SessionParams
from seesaw_amd.bitmap import BitMap
from seesaw_amd.loops.active_search import ActiveSearch, LKNNSearch
from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
from seesaw_amd.seesaw_bench import benchmark_loop
from seesaw_amd.seesaw_session import make_session
from seesaw_amd.synthetic import GlobalDataManager, make_dataset

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=1560000)
ap.add_argument("--tiles", type=int, default=1)
ap.add_argument("--batches", type=int, default=30)
ap.add_argument("--pairs", type=int, default=3)
args = ap.parse_args()
assert args.pairs >= 3, "at least three timed pairs"

ds = make_dataset("lvis", n_images=args.images, tiles_per_image=args.tiles, n_categories=2, positive_frac=0.05, seed=11, knn_k=10)
ds.embedding.noise = 1.2
gdm = GlobalDataManager().add(ds)
boxes, _ = ds.load_ground_truth()
subset = BitMap(ds.file_meta.index.values)
matrix = dict(knn_path="nndescent60", symmetric=False, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
lp = dict(matrix_options=matrix, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0, calib_b=-0.4, prior_weight=1.0)
LOOPS = {
    "active_search": dict(gamma=dict(mode="clip", calibration="sigmoid", a=10.0, b=-0.2), reward_horizon=5, adjust_horizon=False,
                          max_steps=10 ** 6, pruning_on=False, implementation="vectorized", **lp),
    "lknn": dict(gamma=0.1, use_clip_as_gamma=False, **lp),
}

rec = {}  # method name -> seconds of every call of the running session; "kernel" -> (selection ms, look-ahead ms) a round


def timed(cls, name):
    inner = getattr(cls, name)

    def wrapper(self, *a, **k):
        t0 = time.perf_counter()
        out = inner(self, *a, **k)
        rec.setdefault(name, []).append(time.perf_counter() - t0)
        if isinstance(self.prob_model, DeviceLKNNModel):  # outside the timed window: the last call's events, and keep timing
            ms = self.prob_model.step_times(True)
            if name == "next_batch" and ms is not None:
                rec.setdefault("kernel", []).append(ms)
        return out

    setattr(cls, name, wrapper)


for cls in (ActiveSearch, LKNNSearch):
    for name in ("next_batch", "refine", "set_text_vec"):
        timed(cls, name)


def session(loop, on_device):
    rec.clear()
    opts = dict(LOOPS[loop], model_on_device=on_device) if on_device else dict(LOOPS[loop])
    p = SessionParams(index_spec=IndexSpec(d_name="lvis", i_name="coarse" if args.tiles == 1 else "multiscale"), interactive=loop, interactive_options=opts,
                      batch_size=1, shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                      start_policy="from_start", index_options={"use_vec_index": False})
    b = BenchParams(name=loop, ground_truth_category="c1", qstr="a c1", n_batches=args.batches, max_results=10 ** 6)
    ret = make_session(gdm, p, b=b)
    with contextlib.redirect_stdout(io.StringIO()):
        benchmark_loop(session=ret["session"], box_data=boxes, subset=subset, b=b, p=p)
    shown = [int(a[0]) for a in ret["session"].acc_indices]
    times = {k: list(v) for k, v in rec.items()}
    times["round"] = [a + b for a, b in zip(times["next_batch"], times["refine"])]  # a round = next_batch + the refine after it
    return shown, times


def spread(x, scale=1e3):
    x = np.asarray(x, dtype=np.float64) * scale
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return f"median {med:9.3f} ms  IQR {q1:9.3f} .. {q3:9.3f}  (n = {x.shape[0]})"


n_vectors = args.images * args.tiles
print(f"# {n_vectors} vectors ({args.images} images x {args.tiles} tiles), {args.batches} rounds a session, "
      f"1 warm-up pair + {args.pairs} timed pairs, option off / on alternating")
for loop in LOOPS:
    acc = {False: {}, True: {}}
    for pair in range(args.pairs + 1):
        shown = {}
        for on_device in (False, True):
            shown[on_device], times = session(loop, on_device)
            if pair:
                for k, v in times.items():
                    acc[on_device].setdefault(k, []).extend(v)
        assert shown[False] == shown[True], (loop, pair, shown)
    print(f"{loop}: the {args.batches} images shown agree in all {args.pairs + 1} pairs")
    for on_device in (False, True):
        tag = "model_on_device" if on_device else "host model     "
        for name in ("next_batch", "refine", "set_text_vec"):
            print(f"  {loop:13s} {tag} {name:12s} {spread(acc[on_device][name])}")
        print(f"  {loop:13s} {tag} {'round':12s} {spread(acc[on_device]['round'])}")
    kernel = np.asarray(acc[True].get("kernel", []), dtype=np.float64).reshape(-1, 2)
    if kernel.shape[0]:
        print(f"  {loop:13s} device events   selection    {spread(kernel[:, 0], 1.0)}")
        if (kernel[:, 1] >= 0).all():
            print(f"  {loop:13s} device events   look-ahead   {spread(kernel[:, 1], 1.0)}")
        state_bytes, operand_bytes = 25 * n_vectors, 16 * n_vectors
        med = np.median(kernel[:, 0]) * 1e-3
        print(f"  {loop:13s} selection reads {state_bytes / 1e6:.1f} MB of state and writes {operand_bytes / 1e6:.1f} MB of operands: "
              f"{(state_bytes + operand_bytes) / med / 1e12:.2f} TB/s over the median (merge levels included)")
