"""GPU: ShardedMultiscaleIndex.query_batch, the rows read once per chunk of queries and one exchange per group, against
the per-query loop `AccessMethod.query_batch(index, ...)` on the same ranks, entry by entry.  Two ranks share the box's
one GPU over gloo with the messages staged through the host (`comm_device="cpu"`), as in tests/test_sharded_index_gpu.py;
each rank is a fresh process and the pair runs under one deadline.  Six vectors: one None (ranks the scores that are
resident, so the same query is run right before either form), one exclusion set that covers the index, different
exclusion sets elsewhere; f32 and f16 rows.  And the world of one rank, in-process, against the unsharded
MultiscaleIndex.query_batch."""
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


def _entries(index_ids, queries):
    """six vectors and their exclusion sets over an index whose image ids are `index_ids`"""
    from seesaw_amd.bitmap import BitMap
    vectors = [None] + [q for q in queries[:5]]
    excludes = [BitMap(index_ids[:3].tolist()), None, BitMap(index_ids[:40].tolist()), BitMap(index_ids.tolist()),
                BitMap(index_ids[10:25].tolist()), BitMap()]
    return vectors, excludes


def _worker(rank, world, port, tmpdir, vector_dtype):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch
    torch.cuda.set_device(0)
    from oracle import seesaw_oracle as orc
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.sharded_index import ShardedMultiscaleIndex
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["pyr_meta"]), int(g["pyr_seed"])
    X = orc.synth_rows(seed, 0, meta.shape[0], 512)
    lo, hi = ShardedMultiscaleIndex.row_range(meta, world, rank)
    # n_slots = 2: the four batched entries make two groups, so two exchanges
    index = ShardedMultiscaleIndex(embedding=None, vectors=None, local_vectors=X[lo:hi], vector_meta=meta, rank=rank,
                                   world=world, device=0, comm_device="cpu", k_max=128, vector_dtype=vector_dtype, n_slots=2)
    queries = [orc.synth_query(seed + i) for i in range(6)]
    vectors, excludes = _entries(index._dbidx, queries)
    kw = dict(topk=10, shortlist_size=50, force_exact=True, agg_method="plain_score", aug_larger="all", rescore_method=None)
    out = {}
    index.query(vector=queries[5], exclude=None, **kw)  # what the entry without a vector ranks
    got = index.query_batch(vectors=vectors, excludes=excludes, **kw)
    out["resident_ok"] = np.asarray(np.array_equal(index._resident_q, np.asarray(vectors[5], np.float32).reshape(-1)))
    index.query(vector=queries[5], exclude=None, **kw)
    want = AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw)
    out.update({f"got_{k}": v for k, v in _flat(got).items()})
    out.update({f"want_{k}": v for k, v in _flat(want).items()})
    # whatever it does not serve is the loop itself
    kw2 = dict(kw, agg_method="avg_score")
    a = index.query_batch(vectors=vectors[1:3], excludes=excludes[1:3], **kw2)
    b = AccessMethod.query_batch(index, vectors=vectors[1:3], excludes=excludes[1:3], **kw2)
    out.update({f"got_avg_{k}": v for k, v in _flat(a).items()})
    out.update({f"want_avg_{k}": v for k, v in _flat(b).items()})
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), **out)
    index.close()
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
def test_two_ranks_batched_equals_the_loop(tmp_path, vector_dtype):
    _run_ranks(2, (2, free_port(), str(tmp_path), vector_dtype))
    for k in range(2):
        r = np.load(tmp_path / f"rank{k}.npz")
        assert bool(r["resident_ok"])
        names = [n[len("got_"):] for n in r.files if n.startswith("got_")]
        assert len(names) == 2 * 6 + 2 * 2
        for n in names:
            assert np.array_equal(r[f"got_{n}"], r[f"want_{n}"]), (k, n)
        assert r["got_e3_dbidxs"].shape[0] == 0                      # the covering exclusion set
        assert all(r[f"got_e{i}_dbidxs"].shape[0] == 10 for i in (0, 1, 2, 4, 5))
    a, b = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    for n in a.files:
        assert np.array_equal(a[n], b[n]), n  # every rank returns the same answer


def test_world_size_1_equals_the_unsharded_batch(oracle):
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from seesaw_amd.indices.multiscale.sharded_index import ShardedMultiscaleIndex
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["pyr_meta"]), int(g["pyr_seed"])
    X = oracle.synth_rows(seed, 0, meta.shape[0], 512)
    a = MultiscaleIndex(embedding=None, vectors=X, vector_meta=meta)
    b = ShardedMultiscaleIndex(embedding=None, vectors=X, vector_meta=meta, rank=0, world=1, k_max=256, n_slots=3)
    try:
        queries = [oracle.synth_query(seed + i) for i in range(6)]
        vectors, excludes = _entries(a._dbidx, queries)
        vectors, excludes = vectors[1:], excludes[1:]  # (the unsharded index ranks other resident scores for a None)
        kw = dict(topk=10, shortlist_size=60, agg_method="plain_score", aug_larger="all", rescore_method=None)
        ra = a.query_batch(vectors=vectors, excludes=excludes, **kw)
        rb = b.query_batch(vectors=vectors, excludes=excludes, **kw)
        fa, fb = _flat(ra), _flat(rb)
        assert fa.keys() == fb.keys()
        for n in fa:
            assert np.array_equal(fa[n], fb[n]), n
        assert np.array_equal(b._resident_q, a._resident_q)
    finally:
        b.close()
        a._dev.close()
