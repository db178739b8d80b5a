"""CPU: the interface of the sharded batch's second stage (include/seesaw_hip.h: ssw_index_stage2_avg_batch_dev) --
declared, exported by both libraries and bound; the argument errors detected before the device is touched; the host
combine of the stage-2 blocks (seesaw_amd.sharded.combine_stage2_block); ShardedMultiscaleIndex.query_batch with
agg_method="avg_score" over a shard factory without `stage2_batch` (the CPU oracle shard) is still the per-query loop."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAME, N_ARGS = "ssw_index_stage2_avg_batch_dev", 11


def test_the_entry_is_declared_exported_and_bound():
    from seesaw_amd import _lib
    lib = _lib.load()
    assert NAME in _lib.declared_symbols()
    assert NAME in _lib._SIGNATURES and len(_lib._SIGNATURES[NAME][1]) == N_ARGS
    assert getattr(lib, NAME).restype is ctypes.c_int32
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NAME, nm, re.M), path
    assert lib.ssw_abi_version() == 1  # additive: the ABI version stays
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_argument_errors_are_invalid_before_the_device_is_touched():
    from seesaw_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 512), dtype=np.float32)
    words = np.zeros(64, dtype=np.uint64)
    qp, wp = ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(words.ctypes.data)
    entry = lib.ssw_index_stage2_avg_batch_dev
    assert entry(None, qp, 2, wp, wp, 16, 10, 1, 0, 0, wp) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert entry(None, qp, 0, wp, wp, 16, 10, 1, 0, 0, wp) == _lib.SSW_ERR_INVALID
    assert "nq=0" in _lib.last_error()
    assert entry(None, qp, 2, wp, wp, 16, 17, 1, 0, 0, wp) == _lib.SSW_ERR_INVALID
    assert "k=17" in _lib.last_error()
    assert entry(None, qp, 2, wp, wp, 16, 0, 1, 0, 0, wp) == _lib.SSW_ERR_INVALID
    assert entry(None, qp, 2, wp, wp, _lib.SSW_MAX_TOPK + 1, 10, 1, 0, 0, wp) == _lib.SSW_ERR_INVALID
    for aug in (3, 7, 8, -1):
        assert entry(None, qp, 2, wp, wp, 16, 10, aug, 0, 0, wp) == _lib.SSW_ERR_INVALID
        assert "aug_larger=%d" % aug in _lib.last_error()


def _block(rng, world, nq, k_max, counts):
    """a stage-2 block with one random owner for every (b, c < counts[b]); rubbish without the owned bit elsewhere"""
    block = np.zeros((world, nq, 2, k_max), dtype=np.uint64)
    scores = rng.standard_normal((nq, k_max)).astype(np.float32)
    rows = rng.integers(0, 2 ** 40, size=(nq, k_max), dtype=np.int64)
    owner = rng.integers(0, world, size=(nq, k_max))
    for b in range(nq):
        for c in range(k_max):
            r = int(owner[b, c])
            if c < counts[b]:
                block[r, b, 0, c] = (np.uint64(1) << np.uint64(32)) | np.uint64(scores[b, c:c + 1].view(np.uint32)[0])
                block[r, b, 1, c] = np.uint64(rows[b, c])
    return block, scores, rows, owner


def test_combine_round_trip_nan_and_ignored_entries():
    from seesaw_amd.sharded import combine_stage2_block
    rng = np.random.default_rng(7)
    world, nq, k_max = 3, 4, 7
    counts = np.array([7, 0, 3, 5], dtype=np.int32)
    block, scores, rows, owner = _block(rng, world, nq, k_max, counts)
    nan_bits = np.float32(np.nan).view(np.uint32)
    block[int(owner[0, 2]), 0, 0, 2] = (np.uint64(1) << np.uint64(32)) | np.uint64(nan_bits)  # owned, and NaN
    # past a query's count anything may stand there: no owner, two owners
    block[0, 2, 0, 5] = block[1, 2, 0, 5] = (np.uint64(1) << np.uint64(32)) | np.uint64(5)
    block[:, 1, :, :] = np.uint64(0xA5A5A5A5A5A5A5A5)
    got_s, got_r = combine_stage2_block(block.view(np.int64), counts, k_max)  # torch hands the block over as int64
    assert got_s.dtype == np.float32 and got_s.shape == (nq, k_max) and got_r.dtype == np.int64 and got_r.shape == (nq, k_max)
    for b in range(nq):
        c = int(counts[b])
        want = scores[b, :c].copy()
        if b == 0:
            assert np.isnan(got_s[0, 2])
            want[2] = np.nan
        assert np.array_equal(got_s[b, :c].view(np.uint32), want.view(np.uint32)), b
        assert np.array_equal(got_r[b, :c], rows[b, :c]), b


@pytest.mark.parametrize("owners", [0, 2])
def test_combine_raises_without_exactly_one_owner(owners):
    from seesaw_amd.sharded import combine_stage2_block
    rng = np.random.default_rng(8)
    counts = np.array([7, 7, 7, 7], dtype=np.int32)
    block, _, _, owner = _block(rng, 3, 4, 7, counts)
    r = int(owner[2, 4])
    if owners == 0:
        block[r, 2, :, 4] = 0
    else:
        block[(r + 1) % 3, 2, :, 4] = block[r, 2, :, 4]
    with pytest.raises(ValueError, match="candidate 4 of query 2 has %d owners" % owners):
        combine_stage2_block(block, counts, 7)


def _meta(m):
    return pd.DataFrame({"dbidx": m[:, 0].astype(np.int64), "zoom_level": m[:, 1].astype(np.int16),
                         "x1": m[:, 2].astype(np.float32), "y1": m[:, 3].astype(np.float32),
                         "x2": m[:, 4].astype(np.float32), "y2": m[:, 5].astype(np.float32)})


def test_avg_score_over_a_factory_without_stage2_batch_is_the_loop(oracle, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _oracle_shard import OracleShard, merge_on_cpu
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.sharded_index import DeviceShard, ShardedMultiscaleIndex
    assert hasattr(DeviceShard, "stage2_batch") and not hasattr(OracleShard, "stage2_batch")
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    meta, seed = _meta(g["pyr_meta"]), int(g["pyr_seed"])
    X = oracle.synth_rows(seed, 0, meta.shape[0], 512)
    index = ShardedMultiscaleIndex(embedding=None, vectors=X, vector_meta=meta, rank=0, world=1, shard_factory=OracleShard,
                                   merge=merge_on_cpu, k_max=128)
    vectors = [oracle.synth_query(seed), oracle.synth_query(seed + 3)]
    kw = dict(topk=5, shortlist_size=30, force_exact=True, agg_method="avg_score", aug_larger="greater", rescore_method=None)
    calls = []
    loop = AccessMethod.query_batch
    monkeypatch.setattr(AccessMethod, "query_batch", lambda self, **k: calls.append(1) or loop(self, **k))
    got = index.query_batch(vectors=vectors, excludes=None, **kw)
    assert calls == [1]  # it went through the loop
    want = [index.query(vector=v, exclude=None, **kw) for v in vectors]
    for a, b in zip(got, want):
        assert np.array_equal(a["dbidxs"], b["dbidxs"]) and len(a["dbidxs"]) == 5
        for x, y in zip(a["activations"], b["activations"]):
            assert np.array_equal(x.values, y.values)
