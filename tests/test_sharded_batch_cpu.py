"""CPU: the batched sharded top-k's interface (include/seesaw_hip.h: ssw_index_set_exchange_target_batch,
ssw_index_topk_batch_dev, ssw_index_topk_slot_deep_dev, ssw_topk_merge_msgs_batch_dev) -- declared, exported and bound;
the argument errors detected before the device is touched; ShardedMultiscaleIndex.query_batch over a shard factory
without `select_batch` (the CPU oracle shard) is the per-query loop; the numpy layout of a chunk's message block."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = {"ssw_index_set_exchange_target_batch": 7, "ssw_index_topk_batch_dev": 7, "ssw_index_topk_slot_deep_dev": 6,
       "ssw_topk_merge_msgs_batch_dev": 13}


def test_the_entries_are_declared_exported_and_bound():
    from seesaw_amd import _lib
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name, n_args in NEW.items():
        assert name in declared, name
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][1]) == n_args, name
        assert getattr(lib, name).restype is ctypes.c_int32
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r" T %s$" % name, nm, re.M), (path, name)
    assert lib.ssw_abi_version() == 1  # additive: the ABI version stays
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integration, name


def test_null_arguments_are_invalid_before_the_device_is_touched():
    from seesaw_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 512), dtype=np.float32)
    qp = ctypes.c_void_p(q.ctypes.data)
    assert lib.ssw_index_set_exchange_target_batch(None, None, 4, 16, 1, 0, 0) == _lib.SSW_ERR_INVALID
    assert lib.ssw_index_topk_batch_dev(None, qp, 2, None, None, 10, 0) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert lib.ssw_index_topk_batch_dev(None, qp, 0, None, None, 10, 0) == _lib.SSW_ERR_INVALID
    assert "nq=0" in _lib.last_error()
    assert lib.ssw_index_topk_slot_deep_dev(None, qp, None, 0, 10, 0) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert lib.ssw_topk_merge_msgs_batch_dev(0, None, None, 2, 66, 2, 16, 1, 10, None, None, None, None) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()


def test_message_block_round_trips():
    from seesaw_amd.sharded import pack_message_block, unpack_message_block
    rng = np.random.default_rng(5)
    k_max, world, nq = 7, 3, 4
    for with_best in (False, True):
        lists = []
        for r in range(world):
            row = []
            for b in range(nq):
                c = int(rng.integers(0, k_max + 1)) if (r, b) != (1, 2) else 0  # one empty list
                keys = np.sort(rng.integers(1, 2 ** 63, size=c, dtype=np.int64).astype(np.uint64) * np.uint64(2))[::-1]
                best = rng.integers(0, 2 ** 40, size=c, dtype=np.int64) if with_best else None
                row.append((keys, best, int((r + b) % 3 == 0)))
            lists.append(row)
        block = pack_message_block(lists, k_max, with_best)
        msg_len = (2 if with_best else 1) * k_max + 1
        assert block.shape == (world, nq, msg_len) and block.dtype == np.uint64
        # the layout ssw_index_set_exchange_target documents, at the place one all-gather of nq * msg_len words puts it
        flat = block.reshape(-1)
        for r in range(world):
            for b in range(nq):
                keys, best, flag = lists[r][b]
                at = r * nq * msg_len + b * msg_len
                assert np.array_equal(flat[at:at + len(keys)], keys)
                assert int(flat[at + msg_len - 1]) == len(keys) | (flag << 32)
                if with_best:
                    assert np.array_equal(flat[at + k_max:at + k_max + len(keys)].view(np.int64), best)
        back = unpack_message_block(block.view(np.int64), k_max, with_best)  # torch hands the block over as int64
        for r in range(world):
            for b in range(nq):
                keys, best, flag = lists[r][b]
                k2, b2, f2 = back[r][b]
                assert np.array_equal(k2, keys) and f2 == flag
                assert (b2 is None) if not with_best else np.array_equal(b2, best)


def _meta(m):
    return pd.DataFrame({"dbidx": m[:, 0].astype(np.int64), "zoom_level": m[:, 1].astype(np.int16),
                         "x1": m[:, 2].astype(np.float32), "y1": m[:, 3].astype(np.float32),
                         "x2": m[:, 4].astype(np.float32), "y2": m[:, 5].astype(np.float32)})


def _same(a, b):
    assert np.array_equal(a["dbidxs"], b["dbidxs"])
    assert len(a["activations"]) == len(b["activations"])
    for x, y in zip(a["activations"], b["activations"]):
        assert np.array_equal(x.values, y.values)


def test_query_batch_over_a_factory_without_select_batch_is_the_loop(oracle):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _oracle_shard import OracleShard, merge_on_cpu
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.sharded_index import DeviceShard, ShardedMultiscaleIndex
    assert hasattr(DeviceShard, "select_batch") and not hasattr(OracleShard, "select_batch")
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["meta"]), int(g["seed"])
    X = oracle.synth_rows(seed, 0, meta.shape[0], 512)
    index = ShardedMultiscaleIndex(embedding=None, vectors=X, vector_meta=meta, rank=0, world=1, shard_factory=OracleShard,
                                   merge=merge_on_cpu, k_max=128)
    all_ids = np.unique(meta.dbidx.values)
    vectors = [oracle.synth_query(seed), oracle.synth_query(seed + 3), oracle.synth_query(seed + 1), oracle.synth_query(seed + 2)]
    excludes = [None, None, BitMap(all_ids[:9]), BitMap(all_ids)]
    kw = dict(topk=5, shortlist_size=50, force_exact=True, agg_method="plain_score", aug_larger="all", rescore_method=None)
    got = index.query_batch(vectors=vectors, excludes=excludes, **kw)
    want = AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw)
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        _same(a, b)
    assert len(got[3]["dbidxs"]) == 0 and len(got[0]["dbidxs"]) == 5
