"""GPU: ShardedMultiscaleIndex.query_batch with agg_method="avg_score" -- the first stage per chunk, then ONE stage-2
launch on every owner and ONE more exchange a group -- against the per-query loop `AccessMethod.query_batch(index, ...)`
on the same ranks, entry by entry and bit for bit.  The harness is tests/test_sharded_batch_index_gpu.py's: two ranks
share the box's one GPU over gloo with the messages staged through the host (`comm_device="cpu"`), each rank a fresh
process, the pair under one deadline; `n_slots=2`, so four served entries make two groups.
The shard factory is a DeviceShard subclass that counts calls: for the served entries `select` (the single query's scan)
is never called and `stage2_batch` is called once per group -- the route, not only the result."""
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
COUNTED = ("select", "select_batch", "stage2_batch")


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
    from seesaw_amd.indices.multiscale.sharded_index import DeviceShard, ShardedMultiscaleIndex

    calls = dict.fromkeys(COUNTED, 0)

    class CountingShard(DeviceShard):
        def select(self, *a, **k):
            calls["select"] += 1
            return super().select(*a, **k)

        def select_batch(self, *a, **k):
            calls["select_batch"] += 1
            return super().select_batch(*a, **k)

        def stage2_batch(self, *a, **k):
            calls["stage2_batch"] += 1
            return super().stage2_batch(*a, **k)

    def counted(fn):
        for name in COUNTED:
            calls[name] = 0
        res = fn()
        return res, np.array([calls[name] for name in COUNTED], dtype=np.int64)

    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["pyr_meta"]), int(g["pyr_seed"])
    X = orc.synth_rows(seed, 0, meta.shape[0], 512)
    lo, hi = ShardedMultiscaleIndex.row_range(meta, world, rank)
    # n_slots = 2: four batched entries make two groups, so two first exchanges, two stage-2 launches, two more exchanges
    index = ShardedMultiscaleIndex(embedding=None, vectors=None, local_vectors=X[lo:hi], vector_meta=meta, rank=rank,
                                   world=world, device=0, comm_device="cpu", k_max=128, vector_dtype=vector_dtype, n_slots=2,
                                   shard_factory=CountingShard)
    queries = [orc.synth_query(seed + i) for i in range(6)]
    vectors, excludes = _entries(index._dbidx, queries)
    served = [1, 2, 4, 5]  # entry 0 has no vector, entry 3's exclusion set covers the index
    base = dict(topk=10, shortlist_size=50, force_exact=True, agg_method="avg_score", rescore_method=None)
    out = {}

    def compare(tag, kw, which):
        vs, es = [vectors[i] for i in which], [excludes[i] for i in which]
        index.query(vector=queries[5], exclude=None, **kw)  # what an entry without a vector ranks
        got, n_got = counted(lambda: index.query_batch(vectors=vs, excludes=es, **kw))
        index.query(vector=queries[5], exclude=None, **kw)
        want, n_want = counted(lambda: AccessMethod.query_batch(index, vectors=vs, excludes=es, **kw))
        out.update({f"got_{tag}_{k}": v for k, v in _flat(got).items()})
        out.update({f"want_{tag}_{k}": v for k, v in _flat(want).items()})
        out[f"calls_{tag}"], out[f"loopcalls_{tag}"] = n_got, n_want

    compare("six", dict(base, aug_larger="greater"), range(6))
    out["resident_ok"] = np.asarray(np.array_equal(index._resident_q, np.asarray(vectors[5], np.float32).reshape(-1)))
    compare("greater", dict(base, aug_larger="greater"), served)
    compare("all", dict(base, aug_larger="all"), served)
    compare("cont", dict(base, aug_larger="greater", aug_weight="cont_weighted"), served)
    compare("v2", dict(base, aug_larger="greater", vector2=queries[0]), served[:2])
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
def test_two_ranks_avg_score_batched_equals_the_loop(tmp_path, vector_dtype):
    _run_ranks(2, (2, free_port(), str(tmp_path), vector_dtype))
    for k in range(2):
        r = np.load(tmp_path / f"rank{k}.npz")
        assert bool(r["resident_ok"])
        names = [n[len("got_"):] for n in r.files if n.startswith("got_")]
        assert len(names) == 2 * (6 + 4 + 4 + 4 + 2)
        for n in names:
            assert np.array_equal(r[f"got_{n}"], r[f"want_{n}"]), (k, n)
        assert r["got_six_e3_dbidxs"].shape[0] == 0  # the covering exclusion set
        assert all(r[f"got_six_e{i}_dbidxs"].shape[0] == 10 for i in (0, 1, 2, 4, 5))
        # the route (select, select_batch, stage2_batch): four served entries in groups of two
        for tag in ("greater", "all", "cont"):
            assert r[f"calls_{tag}"].tolist() == [0, 2, 2], (k, tag)
            assert r[f"loopcalls_{tag}"].tolist() == [4, 0, 0], (k, tag)
        assert r["calls_six"].tolist() == [1, 2, 2], k  # the entry without a vector is a single query
        assert r["calls_v2"].tolist() == [2, 0, 0], k   # vector2 is the loop, because it is the loop
    a, b = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    for n in a.files:
        assert np.array_equal(a[n], b[n]), n  # every rank returns the same answer
