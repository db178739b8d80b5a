"""CPU: the interface of the pruned sharded batch (include/seesaw_hip.h: ssw_index_topk_batch_dev_pruned,
ssw_index_prune_batch_dev_read; include/seesaw_hip_debug.h: ssw_tune_surv_cap, ssw_debug_rescore_survivors) -- declared,
exported by the libraries they belong to, bound and documented; the argument errors detected before the device is
touched, with the plain entry's messages; ShardedMultiscaleIndex.query_batch(prune=True) over a shard factory without
`select_batch` (the CPU oracle shard) is the per-query loop."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRODUCT = {"ssw_index_topk_batch_dev_pruned": 7, "ssw_index_prune_batch_dev_read": 3}
LAB = {"ssw_tune_surv_cap": 1, "ssw_debug_rescore_survivors": 8}


def _exported(path):
    return subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout


def test_the_product_entries_are_declared_exported_bound_and_documented():
    from seesaw_amd import _lib
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name, n_args in PRODUCT.items():
        assert name in declared, name
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][1]) == n_args, name
        assert getattr(lib, name).restype is ctypes.c_int32
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        nm = _exported(path)
        for name in PRODUCT:
            assert re.search(r" T %s$" % name, nm, re.M), (path, name)
    assert lib.ssw_abi_version() == 1  # additive: the ABI version stays
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in PRODUCT:
        assert name in integration, name
    # the plain entry keeps its signature, the pruned one has the same
    assert _lib._SIGNATURES["ssw_index_topk_batch_dev_pruned"] == _lib._SIGNATURES["ssw_index_topk_batch_dev"]


def test_the_lab_entries_are_in_the_lab_library_only():
    from seesaw_amd import _lib
    declared = _lib.declared_symbols(_lib.DEBUG_HEADER_PATH)
    product, lab = _exported(_lib.LIB_PATH), _exported(_lib.DEBUG_LIB_PATH)
    for name, n_args in LAB.items():
        assert name in declared and name not in _lib.declared_symbols(), name
        assert name in _lib._DEBUG_SIGNATURES and len(_lib._DEBUG_SIGNATURES[name][1]) == n_args, name
        assert re.search(r" T %s$" % name, lab, re.M), name
        assert not re.search(r"\b%s\b" % name, product), name


def test_null_arguments_are_invalid_before_the_device_is_touched():
    from seesaw_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 512), dtype=np.float32)
    qp = ctypes.c_void_p(q.ctypes.data)
    messages = []
    for entry in (lib.ssw_index_topk_batch_dev, lib.ssw_index_topk_batch_dev_pruned):
        assert entry(None, qp, 2, None, None, 10, 0) == _lib.SSW_ERR_INVALID
        null = _lib.last_error()
        assert entry(None, None, 2, None, None, 10, 0) == _lib.SSW_ERR_INVALID
        assert _lib.last_error() == null
        assert entry(None, qp, 0, None, None, 10, 0) == _lib.SSW_ERR_INVALID
        messages.append((null, _lib.last_error()))
    assert messages[0] == messages[1]  # the plain entry's messages
    assert "NULL" in messages[1][0] and "nq=0" in messages[1][1]
    out, w = np.zeros(32, dtype=np.int32), ctypes.c_int32(7)
    assert lib.ssw_index_prune_batch_dev_read(None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                              ctypes.byref(w)) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()


def test_the_python_layers_take_the_keyword_and_default_to_the_plain_path():
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.indices.multiscale.sharded_index import DeviceShard, ShardedMultiscaleIndex
    from seesaw_amd.sharded import ShardedSyntheticIndex
    for fn in (DeviceIndex.topk_batch_dev, DeviceShard.select_batch, ShardedSyntheticIndex.topk_batch_async,
               ShardedSyntheticIndex.topk_batch, ShardedMultiscaleIndex._query_batch_sharded):
        p = inspect.signature(fn).parameters
        assert "prune" in p and p["prune"].default is False, fn
    assert hasattr(DeviceIndex, "prune_batch_dev_counts")


def _meta(m):
    return pd.DataFrame({"dbidx": m[:, 0].astype(np.int64), "zoom_level": m[:, 1].astype(np.int16),
                         "x1": m[:, 2].astype(np.float32), "y1": m[:, 3].astype(np.float32),
                         "x2": m[:, 4].astype(np.float32), "y2": m[:, 5].astype(np.float32)})


def _same(a, b):
    assert np.array_equal(a["dbidxs"], b["dbidxs"])
    assert len(a["activations"]) == len(b["activations"])
    for x, y in zip(a["activations"], b["activations"]):
        assert np.array_equal(x.values, y.values)


def test_query_batch_prune_over_a_factory_without_select_batch_is_the_loop(oracle):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _oracle_shard import OracleShard, merge_on_cpu
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.sharded_index import ShardedMultiscaleIndex
    assert not hasattr(OracleShard, "select_batch")
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["meta"]), int(g["seed"])
    X = oracle.synth_rows(seed, 0, meta.shape[0], 512)
    index = ShardedMultiscaleIndex(embedding=None, vectors=X, vector_meta=meta, rank=0, world=1, shard_factory=OracleShard,
                                   merge=merge_on_cpu, k_max=128)
    all_ids = np.unique(meta.dbidx.values)
    vectors = [oracle.synth_query(seed), oracle.synth_query(seed + 3), oracle.synth_query(seed + 1), oracle.synth_query(seed + 2)]
    excludes = [None, None, BitMap(all_ids[:9]), BitMap(all_ids)]
    kw = dict(topk=5, shortlist_size=50, force_exact=True, agg_method="plain_score", aug_larger="all", rescore_method=None)
    got = index.query_batch(vectors=vectors, excludes=excludes, prune=True, **kw)
    want = AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw)
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        _same(a, b)
    assert len(got[3]["dbidxs"]) == 0 and len(got[0]["dbidxs"]) == 5
    # a route the batch does not serve ignores the flag the same way
    kw2 = dict(kw, agg_method="avg_score")
    for a, b in zip(index.query_batch(vectors=vectors[:2], excludes=excludes[:2], prune=True, **kw2),
                    AccessMethod.query_batch(index, vectors=vectors[:2], excludes=excludes[:2], **kw2)):
        _same(a, b)
