"""GPU: the pruned sharded batch through the two index classes, against their per-query loops entry by entry.  Two ranks
share the box's one GPU over gloo with the messages staged through the host (`comm_device="cpu"`), as in
tests/test_sharded_batch_index_gpu.py; each rank is a fresh process on the lab build with the pruning threshold at one
row, and the pair runs under one deadline.  ShardedMultiscaleIndex.query_batch(prune=True, agg_method="plain_score"):
six vectors, one of them with an exclusion set that leaves rank 0 five images -- fewer than the shortlist, so rank 0's
certificate fails for that query and the repair runs there and only there.  ShardedSyntheticIndex.topk_batch(prune=True):
nine queries in groups of four against topk()."""
import os
import sys
import time

import numpy as np
import pandas as pd
import pytest

from conftest import free_port  # noqa: E402
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEADLINE_S = 240


def _meta(m):
    return pd.DataFrame({"dbidx": m[:, 0].astype(np.int64), "zoom_level": m[:, 1].astype(np.int16),
                         "x1": m[:, 2].astype(np.float32), "y1": m[:, 3].astype(np.float32),
                         "x2": m[:, 4].astype(np.float32), "y2": m[:, 5].astype(np.float32)})


def _flat(results):
    """a list of query results as arrays that np.savez takes and np.array_equal compares bit for bit"""
    out = {}
    for i, res in enumerate(results):
        out[f"e{i}_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
        acts = [a[["x1", "y1", "x2", "y2", "dbidx", "score"]].values[0].astype(np.float64) for a in res["activations"]]
        out[f"e{i}_acts"] = np.stack(acts) if acts else np.zeros((0, 6))
    return out


def _multiscale(rank, world, vector_dtype, out):
    from oracle import seesaw_oracle as orc
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.sharded_index import ShardedMultiscaleIndex
    from seesaw_amd.sharded import shard_bounds_by_image
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["pyr_meta"]), int(g["pyr_seed"])
    X = orc.synth_rows(seed, 0, meta.shape[0], 512)
    lo, hi = ShardedMultiscaleIndex.row_range(meta, world, rank)
    index = ShardedMultiscaleIndex(embedding=None, vectors=None, local_vectors=X[lo:hi], vector_meta=meta, rank=rank,
                                   world=world, device=0, comm_device="cpu", k_max=128, vector_dtype=vector_dtype, n_slots=4)
    ids = index._dbidx
    _, hi0, _, _ = shard_bounds_by_image(index._row_start, world, 0)
    queries = [orc.synth_query(seed + i) for i in range(6)]
    excludes = [None, BitMap(ids[:40].tolist()), BitMap(ids[5:hi0].tolist()), BitMap(ids.tolist()),
                BitMap(ids[10:25].tolist()), BitMap()]
    kw = dict(topk=10, shortlist_size=50, force_exact=True, agg_method="plain_score", aug_larger="all", rescore_method=None)
    repaired = []
    deep = index._shard.select_slot_deep
    index._shard.select_slot_deep = lambda q, k, ex, slot: (repaired.append(int(slot)), deep(q, k, ex, slot))[1]
    got = index.query_batch(vectors=queries, excludes=excludes, prune=True, **kw)
    out["ms_repaired"] = np.asarray(repaired, dtype=np.int64)
    out["ms_pruned_queries"] = np.asarray(index._shard.index.prune_stats()["queries"])
    out["ms_resident_ok"] = np.asarray(np.array_equal(index._resident_q, np.asarray(queries[5], np.float32).reshape(-1)))
    want = AccessMethod.query_batch(index, vectors=queries, excludes=excludes, **kw)
    out.update({f"got_ms_{k}": v for k, v in _flat(got).items()})
    out.update({f"want_ms_{k}": v for k, v in _flat(want).items()})
    # a route the batch does not serve runs its loop and ignores the flag
    kw2 = dict(kw, agg_method="avg_score")
    a = index.query_batch(vectors=queries[:2], excludes=excludes[:2], prune=True, **kw2)
    b = AccessMethod.query_batch(index, vectors=queries[:2], excludes=excludes[:2], **kw2)
    out.update({f"got_avg_{k}": v for k, v in _flat(a).items()})
    out.update({f"want_avg_{k}": v for k, v in _flat(b).items()})
    index.close()


def _synthetic(rank, world, vector_dtype, out):
    import torch
    from seesaw_amd.sharded import ShardedSyntheticIndex
    idx = ShardedSyntheticIndex(40_000, 512, seed=9, rank=rank, world=world, local_device=0, k_max=32, comm_device="cpu",
                                vector_dtype=vector_dtype, n_slots=4)
    rng = np.random.default_rng(10)
    Q = rng.standard_normal((9, 512)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    got = idx.topk_batch(Q, 10, prune=True)
    out["syn_pruned_queries"] = np.asarray(idx.local.prune_stats()["queries"])
    surv, why = idx.local.prune_batch_dev_counts()
    out["syn_last_chunk"] = np.stack([surv, why.astype(np.int64)])
    for b in range(9):
        qd = torch.from_numpy(Q[b]).to(idx.device)
        imgs, scores = idx.topk(qd.data_ptr(), 10)
        out[f"got_syn_{b}_imgs"], out[f"want_syn_{b}_imgs"] = got[b][0], imgs
        out[f"got_syn_{b}_scores"], out[f"want_syn_{b}_scores"] = got[b][1].view(np.uint32), scores.view(np.uint32)
    idx.close()


def _worker(rank, world, port, tmpdir, vector_dtype):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch
    torch.cuda.set_device(0)
    from seesaw_amd import _lib
    out = {}
    with _lib.debug_hooks():
        _lib.call("ssw_tune_prune", 1, 1, -1)  # every shard is pruned, from one row on
        try:
            _multiscale(rank, world, vector_dtype, out)
            _synthetic(rank, world, vector_dtype, out)
        finally:
            _lib.call("ssw_tune_prune", 1, -1, -1)
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(world, args):
    """fresh processes, joined under one deadline: a rank that does not come back is ended, never waited for"""
    ctx = mp.spawn(_worker, args=args, nprocs=world, join=False)
    t0 = time.monotonic()
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() - t0 < DEADLINE_S, "the ranks did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()


@pytest.mark.parametrize("vector_dtype", ["float32", "float16"])
def test_two_ranks_pruned_batch_equals_the_loop(tmp_path, vector_dtype):
    _run_ranks(2, (2, free_port(), str(tmp_path), vector_dtype))
    for k in range(2):
        r = np.load(tmp_path / f"rank{k}.npz")
        assert bool(r["ms_resident_ok"])
        names = [n[len("got_"):] for n in r.files if n.startswith("got_")]
        assert len(names) == 2 * 6 + 2 * 2 + 2 * 9
        for n in names:
            assert np.array_equal(r[f"got_{n}"], r[f"want_{n}"]), (k, n)
        assert r["got_ms_e3_dbidxs"].shape[0] == 0                      # the covering exclusion set
        assert all(r[f"got_ms_e{i}_dbidxs"].shape[0] == 10 for i in (0, 1, 2, 4, 5))
        # five entries went through the pruned chunks (the covering set goes through `query`), on both ranks
        assert int(r["ms_pruned_queries"]) >= 5 and int(r["syn_pruned_queries"]) >= 9
        assert r["syn_last_chunk"].shape == (2, 1) and int(r["syn_last_chunk"][1, 0]) == 0  # the remainder of one
    a, b = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    # entry 2 left rank 0 five images, fewer than the shortlist: slot 2 of the first group failed there, only there
    assert a["ms_repaired"].tolist() == [2] and b["ms_repaired"].tolist() == []
    for n in a.files:
        if n not in ("ms_repaired", "ms_pruned_queries", "syn_pruned_queries", "syn_last_chunk"):
            assert np.array_equal(a[n], b[n]), n  # every rank returns the same answer
