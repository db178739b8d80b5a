"""GPU: whole feedback sessions on an f16 index.  A session whose index holds binary16 rows
(SessionParams.index_options={"vector_dtype": "float16"} -> SyntheticDataset.load_index -> MultiscaleIndex) must show
the same images, round by round, as the same session over the dataset whose vectors were rounded to binary16 up front
and kept f32: the host mirror (`index.vectors[rows]`), the k-NN graph of the rounded rows, X'LX and the feedback gathers
all see the numbers the device scans.  The C5-small parameters of tests/test_c5_sequence_gpu.py; then the row-sharded
multiscale index with two ranks on one GPU."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

from conftest import free_port  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MATRIX = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
LP = dict(matrix_options=MATRIX, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0, calib_b=-0.4,
          prior_weight=1.0)
LOGREG = dict(class_weights=1.0, scale="centered", reg_lambda=1.0, max_iter=200.0, lr=1, fit_intercept=False)
OPTIONS = {
    "plain": None,
    "knn_prop2": LP,
    "multi_reg": dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=0.0,
                      reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=200, pos_weight="balanced",
                      lr=1.0, matrix_options=MATRIX),
    "pseudo_lr": dict(switch_over=True, real_sample_weight=1.0, sample_size=10000, log_reg_params=LOGREG,
                      label_prop_params=LP),
}


def widen(X):
    return np.asarray(X).astype(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def c5_pair():
    """(the C5-small dataset, the same dataset with its vectors rounded to binary16 and kept f32)"""
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    g = np.load(os.path.join(GOLDEN, "c5_sequence.npz"))
    out = []
    for rounded in (False, True):
        ds = make_dataset("lvis", knn_k=10, **json.loads(str(g["make"])))
        ds.embedding.noise = float(g["noise"])
        if rounded:
            ds.vectors = widen(ds.vectors)
        out.append((GlobalDataManager().add(ds), ds))
    return out


def _session(gdm, ds, name, vector_dtype):
    import torch
    from seesaw_amd.basic_types import BenchParams, IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.seesaw_bench import benchmark_loop
    from seesaw_amd.seesaw_session import make_session
    p = SessionParams(index_spec=IndexSpec(d_name="lvis", i_name="multiscale", c_name=None), interactive=name,
                      interactive_options=OPTIONS[name], shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                      batch_size=1, start_policy="from_start" if name == "knn_prop2" else "after_first_batch",
                      index_options={"use_vec_index": False, "vector_dtype": vector_dtype})
    b = BenchParams(name=name, ground_truth_category="c1", qstr="a c1", n_batches=30, max_results=10 ** 6)
    np.random.seed(0)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        ret = make_session(gdm, p, b=b)
        boxes, _ = ds.load_ground_truth()
        out = benchmark_loop(session=ret["session"], box_data=boxes, subset=BitMap(ds.file_meta.index.values), b=b, p=p)
    shown = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in ret["session"].acc_indices])
    return shown, out["nfound"], ret["session"]


@pytest.mark.parametrize("name", ["plain", "multi_reg", "knn_prop2", "pseudo_lr"])
def test_f16_session_equals_the_session_over_prerounded_f32_rows(c5_pair, name):
    (gdm16, ds16), (gdm32, ds32) = c5_pair
    shown16, nfound16, s16 = _session(gdm16, ds16, name, "float16")
    shown32, nfound32, s32 = _session(gdm32, ds32, name, "float32")
    idx16, idx32 = ds16.load_index(options={"vector_dtype": "float16"}), ds32.load_index(options={"vector_dtype": "float32"})
    assert idx16._dev.dtype == np.float16 and idx32._dev.dtype == np.float32  # the sessions ran on those indexes
    assert np.array_equal(idx16.vectors, ds32.vectors)                        # the host mirror is the rounded rows
    assert len(shown16) == 30
    assert np.array_equal(shown16, shown32), (shown16.tolist(), shown32.tolist())
    assert nfound16 == nfound32


def _sharded_worker(rank, world, port, tmpdir):
    """the same sessions over a two-rank sharded index: f16 shards built from the original rows against f32 shards of the
    rounded rows; no rank holds the matrix (the fitting loops gather rows from the shards)"""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from seesaw_amd.basic_types import BenchParams, IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.multiscale.sharded_index import ShardedMultiscaleIndex
    from seesaw_amd.seesaw_bench import benchmark_loop
    from seesaw_amd.seesaw_session import Session
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    g = np.load(os.path.join(GOLDEN, "bench_loop.npz"))
    spec = json.loads(str(g["datasets"]))["A"]
    ds = make_dataset("lvis", knn_k=10, **spec["make"])
    ds.embedding.noise = spec["noise"]
    X = ds.vectors
    ds.vectors = widen(X)  # the graph and the ground truth of the rounded rows
    gdm = GlobalDataManager().add(ds)
    boxes, _ = ds.load_ground_truth()
    graph = ds.knn_graph()
    options = {
        "plain": None,
        "multi_reg_data": dict(label_loss_type="pairwise_rank_loss", rank_loss_margin=0.2, use_qvec_norm=None,
                               reg_data_lambda=1000.0, reg_norm_lambda=100.0, reg_query_lambda=10.0, verbose=False,
                               max_iter=100, pos_weight="balanced", lr=1.0, matrix_options=MATRIX),
        "knn_prop2": LP,
    }
    lo, hi = ShardedMultiscaleIndex.row_range(ds.vector_meta, world, rank)
    out = {}
    for dtype, local in (("float16", X[lo:hi]), ("float32", ds.vectors[lo:hi])):
        for name, opts in options.items():
            index = ShardedMultiscaleIndex(embedding=ds.embedding, vectors=None, local_vectors=local,
                                           vector_meta=ds.vector_meta, rank=rank, world=world, device=0,
                                           comm_device="cpu", k_max=128, vector_dtype=dtype)
            index.knng = {n_: graph for n_ in ("exact", "nndescent60", "")}
            interactive = "multi_reg" if name.startswith("multi_reg") else name
            p = SessionParams(index_spec=IndexSpec(d_name="lvis", i_name="multiscale", c_name=None),
                              interactive=interactive, interactive_options=opts, shortlist_size=50,
                              agg_method="plain_score", aug_larger="greater", batch_size=1,
                              start_policy="from_start" if name == "knn_prop2" else "after_first_batch",
                              index_options={"use_vec_index": False})
            b = BenchParams(name=name, ground_truth_category="c1", qstr="a c1", n_batches=25, max_results=10)
            np.random.seed(0)
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                session = Session(gdm, ds, index, p)
                benchmark_loop(session=session, box_data=boxes, subset=BitMap(ds.file_meta.index.values), b=b, p=p)
            out[f"{dtype}_{name}"] = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1)
                                                     for a in session.acc_indices])
            if dtype == "float16":
                out[f"{name}_dev_dtype"] = np.asarray(str(index._shard.index.dtype))
            index.close()
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_f16_sharded_sessions_equal_the_prerounded_f32_sharded_sessions(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_sharded_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    for k in range(2):
        r = np.load(tmp_path / f"rank{k}.npz")
        for name in ("plain", "multi_reg_data", "knn_prop2"):
            assert str(r[f"{name}_dev_dtype"]) == "float16"
            assert len(r[f"float16_{name}"]) > 0
            assert np.array_equal(r[f"float16_{name}"], r[f"float32_{name}"]), (k, name)
