"""CPU: the batched scan / top-k's interface (include/seesaw_hip.h: ssw_index_scan_batch, ssw_index_topk_batch) --
declared, exported and bound; the argument errors that are detected before the device is touched; the Python layers'
handling of the per-query exclusion lists and the default `AccessMethod.query_batch`."""
import ctypes

import numpy as np
import pytest

NEW = ("ssw_index_scan_batch", "ssw_index_topk_batch")


def test_symbols_are_declared_exported_and_bound():
    from seesaw_amd import _lib
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib._SIGNATURES, name
        assert getattr(lib, name).restype is ctypes.c_int32
    assert _lib.load().ssw_abi_version() == 1  # additive: the ABI version stays
    # the batch-width switch belongs to the lab build alone
    assert "ssw_tune_scan_batch" in _lib.declared_symbols(_lib.DEBUG_HEADER_PATH)
    assert "ssw_tune_scan_batch" in _lib._DEBUG_SIGNATURES and "ssw_tune_scan_batch" not in _lib._SIGNATURES
    assert not hasattr(lib, "ssw_tune_scan_batch")
    assert hasattr(_lib.load_debug(), "ssw_tune_scan_batch")


def test_null_handle_and_empty_batch_are_invalid():
    from seesaw_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 512), dtype=np.float32)
    cnt = np.zeros(2, dtype=np.int32)
    qp, cp = ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(cnt.ctypes.data)
    assert lib.ssw_index_topk_batch(None, qp, 2, None, None, 10, None, None, None, cp) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert lib.ssw_index_topk_batch(None, qp, 0, None, None, 10, None, None, None, cp) == _lib.SSW_ERR_INVALID
    assert "nq=0" in _lib.last_error()
    assert lib.ssw_index_topk_batch(None, qp, -3, None, None, 10, None, None, None, cp) == _lib.SSW_ERR_INVALID
    assert "nq=-3" in _lib.last_error()
    assert lib.ssw_index_scan_batch(None, qp, 2, None) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert lib.ssw_index_scan_batch(None, qp, 0, None) == _lib.SSW_ERR_INVALID
    assert "nq=0" in _lib.last_error()


def test_excluded_argument_none_ragged_and_wrong_length():
    from seesaw_amd.device_index import DeviceIndex
    pack = DeviceIndex._excluded_batch
    assert pack(None, 3) == (None, None)
    ids, off = pack([[5, 1, 5], None, range(3), [], np.array([7])], 5)
    assert ids.dtype == np.int64 and off.dtype == np.int64
    assert ids.tolist() == [5, 1, 5, 0, 1, 2, 7] and off.tolist() == [0, 3, 3, 6, 6, 7]
    ids, off = pack([None, []], 2)  # lists given, nothing excluded: offsets only
    assert ids is None and off.tolist() == [0, 0, 0]
    ids, off = pack((set([4]), frozenset()), 2)
    assert ids.tolist() == [4] and off.tolist() == [0, 1, 1]
    with pytest.raises(ValueError, match="2 lists for 3 queries"):
        pack([[1], [2]], 3)
    with pytest.raises(ValueError):
        pack([], 1)


class _StubIndex:
    """an AccessMethod whose `query` records its calls"""

    def __new__(cls):
        from seesaw_amd.indices.interface import AccessMethod

        class Stub(AccessMethod):
            def __init__(self):
                self.calls = []

            def query(self, *, topk, vector=None, exclude=None, **kwargs):
                self.calls.append((topk, None if vector is None else float(np.sum(vector)), exclude, kwargs))
                return {"dbidxs": np.arange(topk) + len(self.calls), "activations": None}
        return Stub()


def test_default_query_batch_is_a_loop_of_query():
    vectors = [np.full(4, 1.0), None, np.full(4, 3.0)]
    excludes = [None, {1, 2}, {9}]
    a, b = _StubIndex(), _StubIndex()
    got = a.query_batch(topk=3, vectors=vectors, excludes=excludes, shortlist_size=15)
    ref = [b.query(topk=3, vector=v, exclude=e, shortlist_size=15) for v, e in zip(vectors, excludes)]
    assert a.calls == b.calls and len(got) == 3
    for g, r in zip(got, ref):
        assert np.array_equal(g["dbidxs"], r["dbidxs"])
    c = _StubIndex()
    c.query_batch(topk=2, vectors=vectors)  # no exclusions: every query gets exclude=None
    assert [call[2] for call in c.calls] == [None, None, None]
    with pytest.raises(ValueError, match="2 entries for 3 vectors"):
        c.query_batch(topk=2, vectors=vectors, excludes=[None, None])


def test_multiscale_keeps_the_per_query_loop():
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from seesaw_amd.indices.coarse.coarse_index import CoarseIndex
    assert CoarseIndex.query_batch is not AccessMethod.query_batch
    assert "follow-up" in MultiscaleIndex.query_batch.__doc__


def test_the_multi_query_kernel_is_an_instance_of_the_row_format_template():
    """like the single-query kernels (tests/test_index_f16_cpu.py): one template over the row format, built from the
    one dot_frag / group_reduce, dispatched for both formats"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scan = open(os.path.join(root, "seesaw_amd", "csrc", "scan.hip")).read()
    m = re.search(r"template <([^>]*)>\s*__global__\s+__launch_bounds__\(256\)\s+void\s+batch_scores_kernel\s*\(", scan)
    assert m and m.group(1).startswith("class R,")
    body = re.sub(r"//[^\n]*", "", scan[m.end():scan.index("// Small index")])  # code only
    assert "dot_frag<C>(" in body and "group_reduce<V, true>(" in body
    # no arithmetic of its own on scores: no fma, no sum around an exchange
    assert not re.search(r"fma|\+\s*__shfl|__shfl\w*\([^;]*\)\s*\+", body)
    for fmt in ("F32Rows", "H16Rows"):
        assert re.search(r"launch_scan_batch_t<%s, 2, \d, \d+>" % fmt, scan), fmt
